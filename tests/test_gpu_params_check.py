"""bh_params_check on the device: Parameters of the generator and of a real
ceremony are accepted against their circuit and round-one storage for any gamma and delta, and every
mutation -- built by splicing Parameters.write() bytes and reading them back -- is refused with
exactly the mask of the equations it breaks.  The storages are made directly, by one contribution
with the known scalars, and the Parameters by the generator, so that no group FFT runs except in the
one ceremony case."""
import ctypes
import os
import random
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mpc_oracle as mo  # noqa: E402

pytestmark = pytest.mark.gpu

R = mo.R
INVALID_ARGUMENT = 10


def _bh():
    import bellman_hip as bh
    return bh


def _full(rng):
    return rng.randrange(1 << 254, R)


# the scalars of tests/test_gpu_mpc_matrix.py
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
_rng2 = random.Random(19)
OTHER = {k: _full(_rng2) for k in TOXIC}
RHO, SIGMA = _full(_rng2), _full(_rng2)


def _handmade(ctx):
    """tests/test_gpu_mpc_matrix.py's hand-made R1CS: 60 constraints and 2 inputs (m = 64).  aux 0:
    1 100 terms in A (duplicates of (variable, row), 35 segments: a long column); aux 1: c and r - c
    on one row of A (an identity that has terms); aux 2: a zero coefficient and no B terms."""
    bh = _bh()
    rng = random.Random(64)
    nc = 60
    asm = bh.KeypairAssembly()
    asm.alloc_input("", None)
    asm.alloc_input("", None)
    for _ in range(5):
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


CIRCUITS = {"and": 4, "handmade": 64, "chain100": 256}


def _storage_of(ctx, length, scalars=TOXIC):
    """The well-formed storage of these scalars: one contribution to the initial one."""
    bh = _bh()
    st = bh.initial_common_paramters(ctx, length)
    new = bh.mpc_common_paramters_generator(ctx, st, (scalars["alpha"], scalars["beta"], scalars["tau"]))
    st = bh.verify_common_paramter_structure(ctx, st, new)
    assert st is not None
    return st


class _Shared:
    """Per circuit: the R1CS, the storage of length 2m and the generator's Parameters bytes, made once."""

    def __init__(self, ctx):
        self.ctx, self.cache = ctx, {}

    def get(self, name):
        if name not in self.cache:
            bh = _bh()
            if name == "and":
                from oracle import circuits as cc
                r1cs = bh.R1CS.from_assembly(self.ctx, bh.synthesize_keypair(cc.AndDemo(None, None)))
            elif name == "handmade":
                r1cs = _handmade(self.ctx)
            else:
                r1cs = bh.R1CS.chain(self.ctx, int(name[5:]))
            m = CIRCUITS[name]
            self.cache[name] = (r1cs, _storage_of(self.ctx, 2 * m), bh.Parameters.generate(self.ctx, r1cs, **TOXIC).write())
        return self.cache[name]


@pytest.fixture(scope="module")
def shared(ctx):
    return _Shared(ctx)


# ---- Parameters::write (groth16/mod.rs:260-290) taken apart and put together again
_VK = (("alpha_g1", 96), ("beta_g1", 96), ("beta_g2", 192), ("gamma_g2", 192), ("delta_g1", 96), ("delta_g2", 192))
_VECS = (("ic", 96), ("h", 96), ("l", 96), ("a", 96), ("b_g1", 96), ("b_g2", 192))


def _parse(data):
    p, o = {}, 0
    for name, size in _VK:
        p[name] = data[o:o + size]
        o += size
    for name, size in _VECS:
        n = int.from_bytes(data[o:o + 4], "big")
        o += 4
        p[name] = [data[o + i * size:o + (i + 1) * size] for i in range(n)]
        o += n * size
    assert o == len(data)
    return p


def _build(p):
    out = b"".join(p[name] for name, _ in _VK)
    for name, _ in _VECS:
        out += len(p[name]).to_bytes(4, "big") + b"".join(p[name])
    return out


def _swap(p, name, i, j):
    assert p[name][i] != p[name][j]
    p[name][i], p[name][j] = p[name][j], p[name][i]


def _g1_add(b, k):
    """The encoded G1 point plus k times the generator (oracle/bls12_381.py)."""
    ok, a = mo.bls.g1_from_uncompressed(b, checked=False)
    assert ok and a is not None
    return mo.g1_bytes(mo.G1.to_affine(mo.G1.add(mo.G1.from_affine(a), mo.G1.from_affine(mo.g1(k)))))


def _mask(ctx, r1cs, storage, data, rho=RHO, sigma=SIGMA):
    return _bh().Parameters.read(ctx, data).check(r1cs, storage, rho, sigma)


def _bits(*names):
    bh = _bh()
    m = 0
    for n in names:
        m |= getattr(bh, "BH_PARAMS_CHECK_" + n)
    return m


# ------------------------------------------------------------------ 1. valid Parameters are accepted
@pytest.mark.parametrize("name", list(CIRCUITS))
def test_generator_parameters_are_accepted(ctx, shared, name):
    bh = _bh()
    r1cs, storage, data = shared.get(name)
    sz = r1cs.sizes()
    m = 1
    while m < sz["constraints"]:
        m *= 2
    assert m == CIRCUITS[name] and len(storage) == 2 * m
    if name == "chain100":
        assert sz["constraints"] == 202  # not a power of two
    assert _mask(ctx, r1cs, storage, data) == 0
    # gamma and delta are free
    other = bh.Parameters.generate(ctx, r1cs, **dict(TOXIC, gamma=OTHER["gamma"], delta=OTHER["delta"]))
    assert other.write() != data
    assert other.check(r1cs, storage, RHO, SIGMA) == 0
    assert other.check(r1cs, storage) == 0  # fresh random rho and sigma
    ms = bh.last_params_check_ms()
    assert len(ms) == 3 and all(x > 0 for x in ms)


def test_handmade_sizes(ctx, shared):
    """aux 1's A column has terms and is absent; aux 2 has no B terms; the appended rows keep the inputs."""
    p = _parse(shared.get("handmade")[2])
    assert [len(p[k]) for k, _ in _VECS] == [2, 63, 5, 2 + 3, 1 + 3, 1 + 3]


def test_ceremony_parameters_are_accepted(ctx, shared):
    """A real ceremony of two players per round at m = 4 (the one case with group FFTs)."""
    bh = _bh()
    r1cs = shared.get("and")[0]
    st = bh.initial_common_paramters(ctx, 8)
    for player in ROUND1:
        st = bh.verify_common_paramter(ctx, st, bh.mpc_common_paramters_generator(ctx, st, player))
        assert st is not None
    matrix = st.matrix(r1cs)
    first = bh.initial_uncommon_paramters(ctx, matrix)
    ust = first
    for player in ROUND2:
        ust = bh.verify_uncommon_paramter(ctx, first, ust, bh.mpc_uncommon_paramters_generator(ctx, ust, player))
        assert ust is not None
    params = bh.generate_parameters_mpc(ctx, st, matrix, ust)
    assert params.check(r1cs, st, RHO, SIGMA) == 0
    # against the round-one storage before the second player, tau, alpha and beta are all others
    before = _storage_of(ctx, 8, dict(zip(("alpha", "beta", "tau"), ROUND1[0])))
    assert params.check(r1cs, before, RHO, SIGMA) == _bits("ALPHA", "BETA", "A", "B_G1", "B_G2", "H", "L", "IC")


# ------------------------------------------------------------------ 2. mutations, each with its mask
def _regenerated(which):
    def f(ctx, r1cs, p):
        return _parse(_bh().Parameters.generate(ctx, r1cs, **dict(TOXIC, **{which: OTHER[which]})).write())
    return f


def _delta_g1_spliced(ctx, r1cs, p):
    p["delta_g1"] = _regenerated("delta")(ctx, r1cs, p)["delta_g1"]
    return p


def _opposite_errors(ctx, r1cs, p):
    p["l"][0] = _g1_add(p["l"][0], 5)
    p["l"][1] = _g1_add(p["l"][1], R - 5)
    return p


def _swapper(name, i, j):
    def f(ctx, r1cs, p):
        _swap(p, name, i, j)
        return p
    return f


def _drop_l(ctx, r1cs, p):
    p["l"] = p["l"][1:]
    return p


MUTATIONS = [
    ("handmade", "a0_a1", _swapper("a", 0, 1), ("A",)),
    ("handmade", "a_last_two", _swapper("a", -2, -1), ("A",)),
    ("handmade", "b_g2_only", _swapper("b_g2", 1, 2), ("B_G2",)),
    ("handmade", "l_swapped", _swapper("l", 0, 3), ("L",)),
    ("handmade", "h_swapped", _swapper("h", 2, 61), ("H",)),
    ("chain100", "h_63_64", _swapper("h", 63, 64), ("H",)),
    ("handmade", "ic_swapped", _swapper("ic", 0, 1), ("IC",)),
    ("handmade", "other_tau", _regenerated("tau"), ("A", "B_G1", "B_G2", "H", "L", "IC")),
    ("handmade", "other_alpha", _regenerated("alpha"), ("ALPHA", "L", "IC")),
    ("handmade", "other_beta", _regenerated("beta"), ("BETA", "L", "IC")),
    ("handmade", "delta_g1_spliced", _delta_g1_spliced, ("DELTA",)),
    ("handmade", "l0_plus_P_l1_minus_P", _opposite_errors, ("L",)),
    ("and", "l_swapped_m4", _swapper("l", 0, 1), ("L",)),
    ("handmade", "l_one_dropped", _drop_l, ("SIZES",)),
]


@pytest.mark.parametrize("circuit,name,mutate,bits", MUTATIONS, ids=[m[1] for m in MUTATIONS])
def test_mutation_masks(ctx, shared, circuit, name, mutate, bits):
    r1cs, storage, data = shared.get(circuit)
    mutated = _build(mutate(ctx, r1cs, _parse(data)))
    assert mutated != data
    assert _mask(ctx, r1cs, storage, mutated) == _bits(*bits)


def test_verdict_does_not_depend_on_the_scalars(ctx, shared):
    r1cs, storage, data = shared.get("handmade")
    p = _parse(data)
    _swap(p, "l", 1, 4)
    bad = _build(p)
    for rho, sigma in ((RHO, SIGMA), (SIGMA, RHO), (2, 3), (R - 1, R - 2)):
        assert _mask(ctx, r1cs, storage, data, rho, sigma) == 0
        assert _mask(ctx, r1cs, storage, bad, rho, sigma) == _bits("L")


def test_another_circuit_of_the_same_sizes(ctx, shared):
    bh = _bh()
    r1cs, storage, data = shared.get("chain100")
    other = bh.R1CS.chain(ctx, 100, seed=8)
    assert other.sizes() == r1cs.sizes()
    params = bh.Parameters.generate(ctx, other, **TOXIC)
    assert params.sizes() == bh.Parameters.read(ctx, data).sizes()
    mask = params.check(r1cs, storage, RHO, SIGMA)
    assert mask and not mask & _bits("SIZES")
    assert params.check(other, storage, RHO, SIGMA) == 0


# ------------------------------------------------------------------ 3. statuses
def test_statuses(ctx, shared):
    bh = _bh()
    lib = bh.lib()
    r1cs, storage, data = shared.get("and")
    params = bh.Parameters.read(ctx, data)
    valid, mask = ctypes.c_int(), ctypes.c_uint32()
    words = lambda x: np.array([(x >> (64 * k)) & 0xFFFFFFFFFFFFFFFF for k in range(4)], dtype=np.uint64)
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    rho, sigma = words(RHO), words(SIGMA)

    def call(c=ctx.h, p=params.h, r=r1cs.h, s=storage.h, a=rho, b=sigma, v=ctypes.byref(valid)):
        return lib.bh_params_check(c, p, r, s, None if a is None else ptr(a), None if b is None else ptr(b), v,
                                   ctypes.byref(mask))

    assert call() == 0 and valid.value == 1 and mask.value == 0
    assert lib.bh_params_check(ctx.h, params.h, r1cs.h, storage.h, ptr(rho), ptr(sigma), ctypes.byref(valid), None) == 0
    for kw in (dict(c=None), dict(p=None), dict(r=None), dict(s=None), dict(a=None), dict(b=None), dict(v=None)):
        assert call(**kw) == INVALID_ARGUMENT
    for bad in (0, R, R + 1, (1 << 256) - 1):
        assert call(a=words(bad)) == INVALID_ARGUMENT
        assert call(b=words(bad)) == INVALID_ARGUMENT
    assert call(a=words(R - 1), b=words(R - 2)) == 0 and valid.value == 1
    # a storage of length 2m - 1
    short = _storage_of(ctx, 2 * 4 - 1)
    assert call(s=short.h) == INVALID_ARGUMENT
    with pytest.raises(bh.SynthesisError) as e:
        params.check(r1cs, short)
    assert e.value.code == INVALID_ARGUMENT
    # a longer storage serves as well
    assert params.check(r1cs, _storage_of(ctx, 11), RHO, SIGMA) == 0
    if bh.device_count() > 1:  # handles of another context's device
        other = bh.Context(1)
        try:
            assert call(c=other.h) == INVALID_ARGUMENT
        finally:
            other.close()


# ------------------------------------------------------------------ 4. scratch budget
def test_scratch_budget_still_fits(ctx, shared):
    r1cs, storage, data = shared.get("and")
    assert _mask(ctx, r1cs, storage, data) == 0
    rep = ctx.scratch_report()
    assert rep["fits"]
