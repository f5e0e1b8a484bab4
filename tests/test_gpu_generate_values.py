"""bh_generate_parameters at chosen QAP values (tests/qap_cases.py) against the oracle's
generate_parameters, byte for byte: the flags u != 0, v != 0 and aux e == 0 of k_r1cs_ext, the two
scans, k_r1cs_compact and the lengths read back, with 0 reached by every kind of column, -1 (whose
two device forms a carry-dropping x == k r test takes for zero) and its neighbours at the first
and the last input and aux variable, an empty b query, and a filtered element on either side of a
256-lane block edge.  Then the same circuits through the ceremony and bh_params_check, whose
filters must agree with the generator's.  Bit-exact, no tolerance."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import qap_cases as qc  # noqa: E402
import test_gpu_mpc_matrix as mm  # noqa: E402
from test_gpu_generate import _generation_still_works  # noqa: E402

pytestmark = pytest.mark.gpu

R = qc.R
UNCONSTRAINED_VARIABLE = 5
CER_TOXIC = {k: mm.TOXIC[k] for k in ("alpha", "beta", "gamma", "delta", "tau")}


def _bh():
    import bellman_hip as bh
    return bh


def _r1cs(ctx, pre):
    bh = _bh()
    r1cs = bh.R1CS.from_assembly(ctx, bh.synthesize_keypair(pre.circuit))
    sz = r1cs.sizes()
    spec = pre.spec
    assert sz["segment"] == qc.SEGMENT
    assert (sz["inputs"], sz["aux"], sz["constraints"]) == (spec["ni"], spec["na"], spec["nc"] + spec["ni"])
    # every term arrives, duplicates of a row included (A: and the appended rows'): the S + 1 and
    # S S + 1 columns really are two-segment and wave-reduced columns on the device
    terms = lambda M: sum(len(col) for col in M)
    c = pre.circuit
    assert (sz["nnz_a"], sz["nnz_b"], sz["nnz_c"]) == (terms(c.A) + spec["ni"], terms(c.B), terms(c.C))
    return r1cs


def _lengths(params):
    sz = params.sizes()
    return {k: sz[k] for k in ("ic", "l", "a", "b_g1", "b_g2")}


# ------------------------------------------------------------------ a. the QAP values themselves
@pytest.mark.parametrize("name", sorted(qc.ALL))
def test_eval_returns_the_prescribed_values(ctx, name):
    """Before the filter is blamed: u, v and the solved w come out of bh_r1cs_eval exactly."""
    spec = qc.ALL[name]
    toxic = CER_TOXIC if name in qc.CEREMONY else qc.FULL
    pre = qc.prescribe(toxic["tau"], toxic, spec)
    lag = qc.lagrange(toxic["tau"], spec["nc"] + spec["ni"])
    u, v, w = _r1cs(ctx, pre).eval(lag)
    assert (u, v, w) == (pre.u, pre.v, pre.w)


# ------------------------------------------------------------------ b. Parameters against the oracle
@pytest.mark.parametrize("name", sorted(qc.SPECS))
def test_parameters_equal_the_oracles(ctx, name):
    bh = _bh()
    pre, want, lengths = qc.expected(name)
    params = bh.Parameters.generate(ctx, _r1cs(ctx, pre), **qc.FULL)
    assert _lengths(params) == lengths == pre.lengths, (name, _lengths(params), lengths)
    assert params.write() == want


@pytest.mark.parametrize("name", ["rot01", "both_m1"])
def test_parameters_equal_the_oracles_fork_toxic_waste(ctx, name):
    bh = _bh()
    pre, want, lengths = qc.expected(name, "fork")
    params = bh.Parameters.generate(ctx, _r1cs(ctx, pre), **qc.FORK)
    assert _lengths(params) == lengths
    assert params.write() == want


# ------------------------------------------------------------------ c. the unconstrained truth table
@pytest.mark.parametrize("name", sorted(qc.UNCONSTRAINED))
def test_aux_e_zero_is_unconstrained(ctx, golden, name):
    bh = _bh()
    pre, want, _ = qc.expected(name)
    assert pre.unconstrained and want is None        # the oracle raised UnconstrainedVariable
    with pytest.raises(bh.UnconstrainedVariable) as e:
        bh.Parameters.generate(ctx, _r1cs(ctx, pre), **qc.FULL)
    assert e.value.code == UNCONSTRAINED_VARIABLE
    _generation_still_works(ctx, golden)


@pytest.mark.parametrize("name", qc.CONSTRAINED_M1)
def test_aux_e_minus_one_is_constrained(ctx, golden, name):
    bh = _bh()
    pre, want, _ = qc.expected(name)
    aux_e = pre.e[pre.spec["ni"]:]
    assert aux_e.count(R - 1) == (2 if name.endswith("twice") else 1) and 0 not in aux_e
    assert bh.Parameters.generate(ctx, _r1cs(ctx, pre), **qc.FULL).write() == want
    _generation_still_works(ctx, golden)


# ------------------------------------------------------------------ d. the three filters agree
@pytest.fixture(scope="module", params=sorted(qc.CEREMONY))
def ceremony(ctx, request):
    """A spec prescribed against the ceremony's product tau, its R1CS, the oracle's bytes and the
    ceremony's storage, matrix and Parameters."""
    bh = _bh()
    pre, want, lengths = qc.expected(request.param, CER_TOXIC)
    r1cs = _r1cs(ctx, pre)
    st = mm._round_one(ctx, mm._domain(r1cs))
    matrix = st.matrix(r1cs)
    params = bh.generate_parameters_mpc(ctx, st, matrix, mm._round_two(ctx, matrix))
    return pre, want, lengths, r1cs, st, matrix, params


def test_ceremony_matrix_has_the_oracles_lengths(ceremony):
    pre, want, lengths, r1cs, st, matrix, params = ceremony
    R1 = R - 1
    assert R1 in pre.u and R1 in pre.v
    assert (R1 in pre.e[pre.spec["ni"]:]) == (pre.spec["name"] != "cer8_uv")
    assert (len(matrix.a), len(matrix.b_g1), len(matrix.b_g2)) == (lengths["a"], lengths["b_g1"], lengths["b_g2"])
    assert lengths == pre.lengths


def test_ceremony_parameters_equal_the_oracles(ceremony):
    pre, want, lengths, r1cs, st, matrix, params = ceremony
    assert params.write() == want


def test_check_accepts_the_oracles_parameters(ctx, ceremony):
    bh = _bh()
    pre, want, lengths, r1cs, st, matrix, params = ceremony
    assert bh.Parameters.read(ctx, want).check(r1cs, st) == 0


def test_check_accepts_the_generators_parameters(ctx, ceremony):
    bh = _bh()
    pre, want, lengths, r1cs, st, matrix, params = ceremony
    mine = bh.Parameters.generate(ctx, r1cs, **CER_TOXIC)
    mask = mine.check(r1cs, st)
    assert mask == 0, (pre.spec["name"], _lengths(mine), lengths, mask)
    assert mine.write() == want


# ------------------------------------------------------------------ e. scratch budget
def test_scratch_budget_still_fits(ctx):
    bh = _bh()
    pre, want, _ = qc.expected("lanes260")
    assert bh.Parameters.generate(ctx, _r1cs(ctx, pre), **qc.FULL).write() == want
    assert ctx.scratch_report()["fits"]
