"""The step between the ceremony's rounds on the device (bh_mpc_common_matrix, bh_mpc_parameters)
against bh_generate_parameters: a ceremony of two players per round, every contribution verified on
the device, must give byte for byte the Parameters the generator gives for the products of the
players' scalars -- vk, ic, h, l, a, b_g1 and b_g2.  The completed form of
test_gpu_mpc.py::test_against_generate_parameters."""
import ctypes
import os
import random
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mpc_oracle as mo  # noqa: E402

pytestmark = pytest.mark.gpu

R = mo.R
UNEXPECTED_IDENTITY, UNCONSTRAINED_VARIABLE, INVALID_ARGUMENT = 1, 5, 10
RS = (27134, 17146)


def _bh():
    import bellman_hip as bh
    return bh


def _full(rng):
    return rng.randrange(1 << 254, R)


_rng = random.Random(20260317)
ROUND1 = [tuple(_full(_rng) for _ in range(3)) for _ in range(2)]  # (alpha, beta, tau) per player
ROUND2 = [tuple(_full(_rng) for _ in range(2)) for _ in range(2)]  # (gamma, delta) per player


def _prod(xs):
    p = 1
    for x in xs:
        p = p * x % R
    return p


TOXIC = dict(alpha=_prod(p[0] for p in ROUND1), beta=_prod(p[1] for p in ROUND1), tau=_prod(p[2] for p in ROUND1),
             gamma=_prod(p[0] for p in ROUND2), delta=_prod(p[1] for p in ROUND2))


def _status(fn, *a, **kw):
    with pytest.raises(_bh().SynthesisError) as e:
        fn(*a, **kw)
    return e.value.code


def _round_one(ctx, m):
    bh = _bh()
    st = bh.initial_common_paramters(ctx, 2 * m)
    for player in ROUND1:
        st = bh.verify_common_paramter(ctx, st, bh.mpc_common_paramters_generator(ctx, st, player))
        assert st is not None
    return st


def _round_two(ctx, matrix):
    bh = _bh()
    first = bh.initial_uncommon_paramters(ctx, matrix)
    ust = first
    for player in ROUND2:
        ust = bh.verify_uncommon_paramter(ctx, first, ust, bh.mpc_uncommon_paramters_generator(ctx, ust, player))
        assert ust is not None
    return ust


def _ceremony(ctx, r1cs):
    bh = _bh()
    m = _domain(r1cs)
    st = _round_one(ctx, m)
    matrix = st.matrix(r1cs)
    return bh.generate_parameters_mpc(ctx, st, matrix, _round_two(ctx, matrix)), st, matrix


def _domain(r1cs):
    m = 1
    while m < r1cs.sizes()["constraints"]:
        m *= 2
    return m


def _circuit_r1cs(ctx, name):
    bh = _bh()
    if name == "and":
        from oracle import circuits as cc
        return bh.R1CS.from_assembly(ctx, bh.synthesize_keypair(cc.AndDemo(None, None)))
    return bh.R1CS.chain(ctx, int(name[5:]))


@pytest.fixture(scope="module")
def chain127(ctx):
    """The 256-constraint chain and its ceremony, shared by the tests that need them."""
    r1cs = _circuit_r1cs(ctx, "chain127")
    return (r1cs,) + _ceremony(ctx, r1cs)


# ------------------------------------------------------------------ 1. against the generator
@pytest.mark.parametrize("name,m", [("and", 4), ("chain127", 256), ("chain100", 256)])
def test_ceremony_parameters_equal_the_generators(ctx, request, name, m):
    bh = _bh()
    shared = request.getfixturevalue("chain127") if name == "chain127" else None
    r1cs = shared[0] if shared else _circuit_r1cs(ctx, name)
    assert _domain(r1cs) == m
    if name == "chain100":
        assert r1cs.sizes()["constraints"] == 202  # not a power of two
    want = bh.Parameters.generate(ctx, r1cs, **TOXIC).write()
    params, st, matrix = shared[1:] if shared else _ceremony(ctx, r1cs)
    assert params.write() == want
    sz = r1cs.sizes()
    assert len(matrix.kin_g1) == len(matrix.kin_g2) == sz["inputs"]
    assert len(matrix.kout_g1) == len(matrix.kout_g2) == sz["aux"]
    assert len(matrix.h_g1) == len(matrix.h_g2) == m
    assert len(matrix.b_g1) == len(matrix.b_g2)
    assert matrix.kin_g2.group == matrix.b_g2.group == 2 and matrix.a.group == 1


# ------------------------------------------------------------------ 2. a hand-made R1CS, m = 64
def _handmade(ctx, unconstrained=False):
    """60 constraints and 2 inputs (m = 64).  aux 0: 1 100 terms in A (duplicates of (variable, row),
    35 segments: a long column); aux 1: c and r - c on one row of A (an identity that has terms);
    aux 2: no B terms; aux 5 (unconstrained only): no term anywhere."""
    bh = _bh()
    rng = random.Random(64)
    nc = 60
    asm = bh.KeypairAssembly()
    asm.alloc_input("", None)
    asm.alloc_input("", None)
    for _ in range(6 if unconstrained else 5):
        asm.alloc("", None)
    asm.num_constraints = nc
    k = lambda: rng.randrange(1, R)
    asm.at_aux[0] = [(k(), i % nc) for i in range(1100)]
    asm.ct_aux[0] = [(k(), 5)]
    c = k()
    asm.at_aux[1] = [(c, 7), (R - c, 7)]
    asm.bt_aux[1] = [(k(), 3), (k(), 59)]
    asm.at_aux[2] = [(k(), 1), (k(), 9), (0, 11)]
    asm.ct_aux[2] = [(k(), 9)]
    asm.bt_aux[3] = [(k(), i) for i in range(0, nc, 2)]
    for t in (asm.at_aux, asm.bt_aux, asm.ct_aux):
        t[4] = [(k(), rng.randrange(nc)) for _ in range(40)]
    asm.bt_inputs[0] = [(1, i) for i in range(nc)]
    asm.ct_inputs[1] = [(k(), 0), (k(), 59)]
    return bh.R1CS.from_assembly(ctx, asm)


def test_handmade_matrices(ctx):
    bh = _bh()
    r1cs = _handmade(ctx)
    sz = r1cs.sizes()
    assert (sz["constraints"], sz["segment"]) == (62, 32) and sz["nnz_a"] == 1100 + 2 + 3 + 40 + 2
    want = bh.Parameters.generate(ctx, r1cs, **TOXIC)
    params, st, matrix = _ceremony(ctx, r1cs)
    assert params.write() == want.write()
    # aux 1 is filtered from a although its column has terms; aux 2 and the inputs' appended rows stay
    assert len(matrix.a) == 2 + 3 and len(matrix.b_g1) == 1 + 3
    assert params.sizes() == want.sizes()


def test_unconstrained_variable(ctx):
    r1cs = _handmade(ctx, unconstrained=True)
    assert _status(_round_one(ctx, 64).matrix, r1cs) == UNCONSTRAINED_VARIABLE


# ------------------------------------------------------------------ 3. end to end
def test_proof_with_the_ceremonys_parameters(ctx, chain127):
    bh = _bh()
    from oracle import circuits as cc
    r1cs, params = chain127[:2]
    circuit = cc.chain_circuit(R, 127)
    proof = bh.create_proof_r1cs(ctx, r1cs, circuit, params, *RS)
    assert proof == bh.create_proof_r1cs(ctx, r1cs, circuit, bh.Parameters.generate(ctx, r1cs, **TOXIC), *RS)
    public = list(bh.assign(circuit).input_assignment)[1:]
    assert bh.verify_proof(params.vk_bytes(), proof, public)


# ------------------------------------------------------------------ 4. statuses
def test_statuses(ctx):
    bh = _bh()
    lib = bh.lib()
    r1cs = _circuit_r1cs(ctx, "and")
    m = 4
    h = ctypes.c_void_p()
    st = _round_one(ctx, m)
    assert lib.bh_mpc_common_matrix(ctx.h, None, r1cs.h, ctypes.byref(h)) == INVALID_ARGUMENT
    assert lib.bh_mpc_common_matrix(ctx.h, st.h, None, ctypes.byref(h)) == INVALID_ARGUMENT
    assert lib.bh_mpc_common_matrix(None, st.h, r1cs.h, ctypes.byref(h)) == INVALID_ARGUMENT
    # a storage of length 2m - 1
    short = bh.initial_common_paramters(ctx, 2 * m - 1)
    short = bh.verify_common_paramter(ctx, short, bh.mpc_common_paramters_generator(ctx, short, ROUND1[0]))
    assert _status(short.matrix, r1cs) == INVALID_ARGUMENT
    # tau_g1[0] is not the generator: the storage's bytes are u32 len, four points, then tau_g1
    data = bytearray(st.write())
    off = 4 + 96 + 192 + 96 + 192
    assert bytes(data[off:off + 96]) == mo.g1_bytes(mo.GEN1)
    data[off:off + 96] = mo.g1_bytes(mo.g1(2))
    assert _status(bh.CommonParamterInStorage.read(ctx, bytes(data)).matrix, r1cs) == INVALID_ARGUMENT
    # a round-two storage whose h is one short
    matrix = st.matrix(r1cs)
    h1, h2 = st.h_basis(m - 1)
    wrong = bh.initial_uncommon_paramters(ctx, matrix.kin_g1, matrix.kin_g2, matrix.kout_g1, matrix.kout_g2, h1, h2)
    assert _status(bh.generate_parameters_mpc, ctx, st, matrix, wrong) == INVALID_ARGUMENT
    good = bh.initial_uncommon_paramters(ctx, matrix)
    assert lib.bh_mpc_parameters(ctx.h, st.h, None, good.h, ctypes.byref(h)) == INVALID_ARGUMENT
    assert lib.bh_mpc_matrix_vector(matrix.h, 9, ctypes.byref(h)) == INVALID_ARGUMENT
    if bh.device_count() > 1:  # handles of another context's device
        other = bh.Context(1)
        try:
            assert lib.bh_mpc_common_matrix(other.h, st.h, r1cs.h, ctypes.byref(h)) == INVALID_ARGUMENT
            assert lib.bh_mpc_parameters(other.h, st.h, matrix.h, good.h, ctypes.byref(h)) == INVALID_ARGUMENT
        finally:
            other.close()


# ------------------------------------------------------------------ 5. scratch budget
def test_scratch_budget_still_fits(ctx):
    bh = _bh()
    r1cs = _circuit_r1cs(ctx, "and")
    st = _round_one(ctx, 4)
    matrix = st.matrix(r1cs)
    bh.generate_parameters_mpc(ctx, st, matrix, bh.initial_uncommon_paramters(ctx, matrix))
    st.tau_g1.read(0, 8)
    rep = ctx.scratch_report()
    assert rep["fits"]
