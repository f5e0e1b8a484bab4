"""Groth16 parameter generation for any R1CS on the device (bh_r1cs_*, bh_generate_parameters)
against the golden Parameters bytes, the oracle's generate_parameters, bh_chain_params and exact
integer dot products.  Bit-exact throughout."""
import ctypes
import random

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
FORK = dict(alpha=6, beta=24, gamma=6, delta=24, tau=2)


def _bh():
    import bellman_hip as bh
    return bh


def _circuit(name, witness=False):
    from oracle import circuits as cc
    if name.startswith("xor"):
        return cc.XorDemo(True, False) if witness else cc.XorDemo(None, None)
    if name.startswith("and"):
        return cc.AndDemo(True, True) if witness else cc.AndDemo(None, None)
    return cc.chain_circuit(R, int(name.rsplit("r", 1)[1]), witness=witness)


def _fx(golden, name):
    return [f for f in golden["proofs"] if f["name"] == name][0]


def _generation_still_works(ctx, golden):
    """The context is usable after an error: the m = 4 circuit generates its golden bytes."""
    bh = _bh()
    assert bh.generate_random_parameters(ctx, _circuit("and")).write().hex() == _fx(golden, "and_true_true")["params"]


# ------------------------------------------------------------------ 1. golden parity
@pytest.mark.parametrize("name", ["xor_true_false", "and_true_true", "mimc_chain_r7", "mimc_chain_r15"])
def test_golden_parity(ctx, golden, name):
    bh = _bh()
    params = bh.generate_random_parameters(ctx, _circuit(name))
    assert params.write() == bytes.fromhex(_fx(golden, name)["params"])


# ------------------------------------------------------------------ 2. full-width toxic waste
def test_full_width_toxic_waste(ctx):
    bh = _bh()
    from oracle import bellman as bm
    from oracle import circuits as cc
    toxic = cc.fr_stream(1234, 5, R)
    assert all(t.bit_length() > 200 for t in toxic)
    want = bm.params_to_bytes(bm.generate_parameters(bm.BLS12_381, _circuit("mimc_chain_r7"), *toxic))
    assert bh.generate_parameters(ctx, _circuit("mimc_chain_r7"), *toxic).write() == want


# ------------------------------------------------------------------ 3. equality with bh_chain_params
@pytest.mark.parametrize("rounds", [1, 15, 100, 5000])
def test_chain_equality(ctx, rounds):
    bh = _bh()
    r1cs = bh.R1CS.chain(ctx, rounds)
    sz = r1cs.sizes()
    assert (sz["inputs"], sz["aux"], sz["constraints"]) == (2, 2 * rounds + 1, 2 * rounds + 2)
    assert (sz["nnz_a"], sz["nnz_b"], sz["nnz_c"]) == (3 * rounds + 2, 4 * rounds, 3 * rounds)
    assert bh.Parameters.generate(ctx, r1cs, **FORK).write() == bh.Parameters.chain(ctx, rounds).write()


def test_chain_r1cs_is_the_python_assembly(ctx):
    """bh_chain_r1cs and the host synthesis of the same circuit evaluate alike."""
    bh = _bh()
    rng = random.Random(5)
    x = [rng.randrange(R) for _ in range(32)]
    native = bh.R1CS.chain(ctx, 15).eval(x)
    assert bh.R1CS.from_assembly(ctx, bh.synthesize_keypair(_circuit("mimc_chain_r15"))).eval(x) == native


# ------------------------------------------------------------------ 4. the kernel at its boundaries
def _draw(rng):
    return rng.choice([0, 1, R - 1, rng.randrange(R), rng.randrange(R)])


def _columns(rng, lengths, nc):
    return [[(_draw(rng), rng.randrange(nc)) for _ in range(k)] for k in lengths]


def _expected(columns, x, appended_from=None, ni=0):
    out = []
    for j, col in enumerate(columns):
        acc = sum(c * x[row] for c, row in col)
        if appended_from is not None and j < ni:  # the library's row input_j * 0 = 0
            acc += x[appended_from + j]
        out.append(acc % R)
    return out


def _segment(ctx):
    return _bh().R1CS.chain(ctx, 1).sizes()["segment"]


LONG = {"0": lambda S: 0, "1": lambda S: 1, "S-1": lambda S: S - 1, "S": lambda S: S, "S+1": lambda S: S + 1,
        "2S+1": lambda S: 2 * S + 1, "S*S+1": lambda S: S * S + 1}


@pytest.mark.parametrize("num_aux", [1, 63, 64, 65])
@pytest.mark.parametrize("k_expr", LONG)
def test_eval_boundaries(ctx, k_expr, num_aux):
    """One aux column of K terms in A (the first aux) and in B (the last aux) beside columns of
    0..3 terms, C entirely empty, against integer dot products."""
    bh = _bh()
    S = _segment(ctx)
    K = LONG[k_expr](S)
    rng = random.Random(1000 * K + num_aux)
    ni, nc = 2, 37
    n = ni + num_aux
    la = [rng.randrange(4) for _ in range(n)]
    lb = [rng.randrange(4) for _ in range(n)]
    la[ni] = K
    lb[n - 1] = K
    A, B, C = _columns(rng, la, nc), _columns(rng, lb, nc), [[] for _ in range(n)]
    r1cs = bh.R1CS.from_arrays(ctx, ni, num_aux, nc, *[bh.flatten_columns(m) for m in (A, B, C)])
    sz = r1cs.sizes()
    assert (sz["inputs"], sz["aux"], sz["constraints"]) == (ni, num_aux, nc + ni)
    assert (sz["nnz_a"], sz["nnz_b"], sz["nnz_c"]) == (sum(la) + ni, sum(lb), 0)
    x = [_draw(rng) for _ in range(64)]
    u, v, w = r1cs.eval(x)
    assert u == _expected(A, x, nc, ni)
    assert v == _expected(B, x)
    assert w == [0] * n


def test_eval_long_input_column_in_c(ctx):
    """ONE with 2S+1 and S*S+1 terms (a wave-reduced column) in C and B, no aux terms at all."""
    bh = _bh()
    S = _segment(ctx)
    rng = random.Random(77)
    ni, na, nc = 3, 2, 100
    n = ni + na
    A = [[] for _ in range(n)]
    B = _columns(rng, [S * S + 1, 0, 2 * S + 1, 0, 0], nc)
    C = _columns(rng, [2 * S + 1, S, 0, 0, 0], nc)
    r1cs = bh.R1CS.from_arrays(ctx, ni, na, nc, *[bh.flatten_columns(m) for m in (A, B, C)])
    x = [_draw(rng) for _ in range(128)]
    u, v, w = r1cs.eval(x)
    assert u == _expected(A, x, nc, ni)
    assert v == _expected(B, x)
    assert w == _expected(C, x)


# ------------------------------------------------------------------ 5. end to end
def test_end_to_end_xor(ctx, golden):
    bh = _bh()
    fx = _fx(golden, "xor_true_false")
    params = bh.generate_random_parameters(ctx, _circuit("xor"))
    proof = bh.create_proof(ctx, _circuit("xor", witness=True), params, 27134, 17146)
    assert proof == bytes.fromhex(fx["proof"])
    public = [int(v, 16) for v in fx["inputs"]][1:]
    assert bh.verify_proof(params.vk_bytes(), proof, public)
    assert not bh.verify_proof(params.vk_bytes(), proof, [(public[0] + 1) % R])


def test_end_to_end_chain(ctx, golden):
    bh = _bh()
    fx = _fx(golden, "mimc_chain_r15")
    params = bh.generate_random_parameters(ctx, _circuit("mimc_chain_r15"))
    proof = bh.prove_witness(ctx, params, bh.Witness.chain(ctx, 15), 27134, 17146)
    assert proof == bytes.fromhex(fx["proof"])
    assert bh.verify_proof(params.vk_bytes(), proof, [int(v, 16) for v in fx["inputs"]][1:])


# ------------------------------------------------------------------ 6. statuses
def _code(f):
    bh = _bh()
    with pytest.raises(bh.SynthesisError) as e:
        f()
    return e.value.code


def _and_r1cs(ctx):
    bh = _bh()
    return bh.R1CS.from_assembly(ctx, bh.synthesize_keypair(_circuit("and")))


@pytest.mark.parametrize("which", ["gamma", "delta"])
def test_status_unexpected_identity(ctx, golden, which):
    bh = _bh()
    toxic = dict(FORK, **{which: 0})
    assert _code(lambda: bh.Parameters.generate(ctx, _and_r1cs(ctx), **toxic)) == 1
    _generation_still_works(ctx, golden)


def test_status_unconstrained_variable(ctx, golden):
    bh = _bh()

    class Dangling:
        def synthesize(self, cs):
            _circuit("and").synthesize(cs)
            cs.alloc("never enforced", lambda: None)

    with pytest.raises(bh.UnconstrainedVariable) as e:
        bh.generate_random_parameters(ctx, Dangling())
    assert e.value.code == 5
    _generation_still_works(ctx, golden)


def test_status_poly_degree_too_large(ctx, golden):
    bh = _bh()
    empty = (np.zeros(2, dtype=np.uint64), np.zeros(0, dtype=np.uint32), np.zeros((0, 4), dtype=np.uint64))
    with pytest.raises(bh.PolynomialDegreeTooLarge) as e:
        bh.R1CS.from_arrays(ctx, 1, 0, 1 << 32, empty, empty, empty)
    assert e.value.code == 3
    _generation_still_works(ctx, golden)


def _arrays(ptr, rows, coeffs):
    bh = _bh()
    return (np.array(ptr, dtype=np.uint64), np.array(rows, dtype=np.uint32), bh.fr_to_mont(coeffs))


BAD_CREATE = {
    "ptr_not_from_zero": lambda: dict(a=_arrays([1, 1, 2], [0, 1], [1, 1])),
    "ptr_decreases": lambda: dict(a=_arrays([0, 2, 1], [0, 1], [1, 1])),
    "row_out_of_range": lambda: dict(a=_arrays([0, 1, 2], [0, 3], [1, 1])),
    "no_inputs": lambda: dict(ni=0, na=2),
    "coefficient_not_reduced": lambda: dict(
        a=(np.array([0, 1, 2], dtype=np.uint64), np.array([0, 1], dtype=np.uint32),
           np.array([[1, 0, 0, 0], [(R >> (64 * k)) & (2 ** 64 - 1) for k in range(4)]], dtype=np.uint64))),
    "null_ptr": lambda: dict(a=(None, np.zeros(2, dtype=np.uint32), np.zeros((2, 4), dtype=np.uint64))),
    "null_rows": lambda: dict(a=(np.array([0, 1, 2], dtype=np.uint64), None, np.zeros((2, 4), dtype=np.uint64))),
}


@pytest.mark.parametrize("case", sorted(BAD_CREATE))
def test_status_invalid_create(ctx, golden, case):
    bh = _bh()
    good = _arrays([0, 1, 2], [0, 2], [1, 1])
    kw = dict(ni=1, na=1, a=good, b=good, c=good)
    kw.update(BAD_CREATE[case]())
    assert _code(lambda: bh.R1CS.from_arrays(ctx, kw["ni"], kw["na"], 3, kw["a"], kw["b"], kw["c"])) == 10
    if case != "no_inputs":  # the same arrays are fine once the flaw is gone
        bh.R1CS.from_arrays(ctx, 1, 1, 3, good, good, good)
    _generation_still_works(ctx, golden)


@pytest.mark.parametrize("toxic", [dict(tau=0), dict(tau=1), dict(tau=R - 1), dict(alpha=R), dict(tau=2 ** 256 - 1),
                                   dict(delta=R + 5)], ids=lambda t: "-".join(f"{k}={v % 1000}" for k, v in t.items()))
def test_status_invalid_toxic_waste(ctx, golden, toxic):
    """tau = 0 and tau^m = 1 (m = 4: tau = 1, tau = -1) are the deliberate deviation; a word >= r
    is rejected, not reduced."""
    bh = _bh()
    assert _code(lambda: bh.Parameters.generate(ctx, _and_r1cs(ctx), **dict(FORK, **toxic))) == 10
    _generation_still_works(ctx, golden)


def test_status_null_arguments(ctx, golden):
    bh = _bh()
    r1cs = _and_r1cs(ctx)
    w = [bh.fr_canonical_words(v) for v in (6, 24, 6, 24, 2)]
    h = ctypes.c_void_p()
    for hole in range(5):
        args = [None if k == hole else w[k].ctypes.data_as(ctypes.c_void_p) for k in range(5)]
        assert bh.lib().bh_generate_parameters(ctx.h, r1cs.h, *args, ctypes.byref(h)) == 10
    assert bh.lib().bh_generate_parameters(ctx.h, None, *[x.ctypes.data_as(ctypes.c_void_p) for x in w],
                                           ctypes.byref(h)) == 10
    sz = (ctypes.c_size_t * 7)()
    assert bh.lib().bh_r1cs_sizes(None, sz) == 10
    _generation_still_works(ctx, golden)
