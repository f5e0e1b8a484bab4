"""bh_mpc_common_check and bh_mpc_common_verify_structure on the device against
tests/mpc_structure_model.py: storages and contributions are built from chosen discrete logs (the
generator vectors of an initial storage through Bases.mul_each, the single points from the oracle),
so the model knows every equation's outcome and the device mask must equal it exactly.

Lengths: 0 to 3 for the vacuous equations, 8 for the single-element changes, 257 for a full-width
ceremony round, 4098 so that the full sums span two 4096-scalar sort tiles and the shifted sum has
4097 terms from base_offset 1."""
import ctypes
import functools
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mpc_oracle as mo  # noqa: E402
import mpc_structure_model as sm  # noqa: E402

pytestmark = pytest.mark.gpu

R = sm.R
TAU, ALPHA, BETA = (0x5AB3F1C2D4E6978877665544332211FFEEDDCCBBAA99887766554433221100FF % R,
                    0x6F0E1D2C3B4A59687786A5B4C3D2E1F00112233445566778899AABBCCDDEEFF1 % R,
                    0x1234567890ABCDEF1122334455667788)
RHO = 0x2B7E151628AED2A6ABF7158809CF4F3C762E7160F38B4DA56A784D9045190CFE % R
PLAYER = (0x3C6EF372FE94F82BE7A1B0C5D2E3F4051627384950617283A4B5C6D7E8F90A1B % R,
          0x510E527FADE682D19B05688C2B3E6C1F1F83D9ABFB41BD6B5BE0CD19137E2179 % R,
          0x243F6A8885A308D313198A2E03707344A4093822299F31D0082EFA98EC4E6C89 % R)
assert all(x.bit_length() >= 253 for x in PLAYER)
INVALID_ARGUMENT = 10


def _bh():
    import bellman_hip as bh
    return bh


@functools.lru_cache(maxsize=None)
def _pt(name, k):
    """log -> bytes of a single point (the oracle's scalar multiplication)."""
    return mo.g1_bytes(mo.g1(k)) if name.endswith("g1") else mo.g2_bytes(mo.g2(k))


def _vec(ctx, name, logs):
    """logs -> bytes of log_i * G on the device."""
    if not logs:
        return b""
    gens = getattr(_bh().initial_common_paramters(ctx, len(logs)), "tau_" + name[-2:])
    return gens.mul_each(list(logs)).read(0, len(logs))


def storage_bytes(ctx, s):
    """The bytes of bh_mpc_common_read (the layout of mpc_oracle.common_storage_bytes) from logs."""
    out = len(s["tau_g1"]).to_bytes(4, "big")
    out += b"".join(_pt(n, s[n]) for n in sm.POINTS)
    return out + b"".join(_vec(ctx, n, s[n]) for n in sm.VECTORS)


def storage(ctx, s):
    return _bh().CommonParamterInStorage.read(ctx, storage_bytes(ctx, s), checked=False)


def contrib(ctx, new, mine):
    """A CommonParamter from the logs of its results and of the player's lists."""
    out = b""
    for name in ("alpha", "beta"):
        out += _pt("g1", new[name + "_g1"]) + _pt("g2", new[name + "_g2"])
        out += _pt("g1", mine[name + "_g1"]) + _pt("g2", mine[name + "_g2"])
    for name in ("tau", "alpha_mul_tau", "beta_mul_tau"):
        cols = [_vec(ctx, name + "_g1", new[name + "_g1"]), _vec(ctx, name + "_g2", new[name + "_g2"]),
                _vec(ctx, name + "_g1", mine[name + "_g1"]), _vec(ctx, name + "_g2", mine[name + "_g2"])]
        n = len(new[name + "_g1"])
        assert [len(c) for c in cols] == [96 * n, 192 * n, 96 * n, 192 * n]
        out += n.to_bytes(4, "big")
        for i in range(n):
            out += cols[0][96 * i:96 * i + 96] + cols[1][192 * i:192 * i + 192]
            out += cols[2][96 * i:96 * i + 96] + cols[3][192 * i:192 * i + 192]
    return _bh().CommonParamter.read(ctx, out, checked=False)


def changed(s, name, i, delta):
    t = {k: (list(v) if isinstance(v, list) else v) for k, v in s.items()}
    if name in sm.POINTS:
        t[name] = (t[name] + delta) % R
    else:
        t[name][i] = (t[name][i] + delta) % R
    return t


def _raw_check(ctx, st, rho_words, want_mask=True):
    lib = _bh().lib()
    valid, mask = ctypes.c_int(-1), ctypes.c_uint32(0xFFFFFFFF)
    code = lib.bh_mpc_common_check(ctx.h, st.h, rho_words.ctypes.data_as(ctypes.c_void_p), ctypes.byref(valid),
                                   ctypes.byref(mask) if want_mask else None)
    return code, valid.value, mask.value


# ------------------------------------------------------------------ 1. well-formed storages
@pytest.mark.parametrize("n", [0, 1, 2, 3, 8, 4098])
def test_well_formed_storage_passes(ctx, n):
    bh = _bh()
    assert bh.initial_common_paramters(ctx, n).check(RHO) == 0
    s = sm.well_formed(n, TAU, ALPHA, BETA)
    assert sm.check_mask(s, RHO) == 0
    st = storage(ctx, s)
    assert len(st) == n
    assert st.check(RHO) == 0
    assert st.check() == 0  # a fresh random rho
    assert st.check(1) == 0 and st.check(R - 1) == 0
    # *valid with no mask asked for
    code, valid, _ = _raw_check(ctx, st, bh.fr_canonical_words(RHO), want_mask=False)
    assert (code, valid) == (0, 1)


@pytest.mark.parametrize("n", [8, 257])
def test_two_contribution_rounds_pass(ctx, n):
    bh = _bh()
    st = bh.initial_common_paramters(ctx, n)
    logs = sm.well_formed(n)
    for player in (PLAYER, (PLAYER[2], PLAYER[0], PLAYER[1])):
        st = bh.verify_common_paramter(ctx, st, bh.mpc_common_paramters_generator(ctx, st, player))
        assert st is not None
        logs, _ = sm.contribute(logs, *player)
        assert st.check(RHO) == 0
    # the model's logs are the device's storage
    if n == 8:
        assert st.write() == storage_bytes(ctx, logs)


# ------------------------------------------------------------------ 2. single-element changes
@pytest.fixture(scope="module")
def honest8():
    return sm.well_formed(8, TAU, ALPHA, BETA)


@pytest.mark.parametrize("i", [0, 1, 7])
@pytest.mark.parametrize("name", sm.VECTORS)
def test_one_vector_element(ctx, honest8, name, i):
    s = changed(honest8, name, i, 0xD1FF)
    want = sm.check_mask(s, RHO)
    assert want != 0
    assert storage(ctx, s).check(RHO) == want


@pytest.mark.parametrize("name", sm.POINTS)
def test_one_point(ctx, honest8, name):
    s = changed(honest8, name, None, 0xD1FF)
    want = sm.check_mask(s, RHO)
    assert want != 0
    assert storage(ctx, s).check(RHO) == want
    # length 0 evaluates the two point equations only
    s0 = changed(sm.well_formed(0, TAU, ALPHA, BETA), name, None, 0xD1FF)
    assert storage(ctx, s0).check(RHO) == sm.check_mask(s0, RHO) == want & (sm.ALPHA | sm.BETA)


def test_short_lengths(ctx):
    for n, name, i in ((1, "tau_g1", 0), (1, "alpha_mul_tau_g2", 0), (2, "tau_g1", 1), (2, "tau_g2", 1),
                       (3, "tau_g1", 2), (3, "beta_mul_tau_g1", 1)):
        s = changed(sm.well_formed(n, TAU, ALPHA, BETA), name, i, 5)
        want = sm.check_mask(s, RHO)
        assert want != 0
        assert storage(ctx, s).check(RHO) == want, (n, name, i)


@pytest.fixture(scope="module")
def honest4098(ctx):
    s = sm.well_formed(4098, TAU, ALPHA, BETA)
    return s, bytearray(storage_bytes(ctx, s))


@pytest.mark.parametrize("i", [4096, 4097])
def test_the_last_elements_of_two_tiles(ctx, honest4098, i):
    """tau_g1[4097] is in R and not in L; tau_g1[4096] is the last term of L."""
    s, data = honest4098
    t = changed(s, "tau_g1", i, 1)
    want = sm.check_mask(t, RHO)
    assert want == sm.POWERS | sm.TAU_G2 | sm.ALPHA_TAU | sm.BETA_TAU
    bad = bytearray(data)
    off = 4 + 96 + 192 + 96 + 192 + 96 * i
    bad[off:off + 96] = _pt("g1", t["tau_g1"][i])
    assert _bh().CommonParamterInStorage.read(ctx, bytes(bad), checked=False).check(RHO) == want
    # and in the G2 vector of another pair, in the second tile
    t = changed(s, "beta_mul_tau_g2", i, 1)
    bad = bytearray(data)
    off = 4 + 96 + 192 + 96 + 192 + 4098 * (96 + 192) * 2 + 4098 * 96 + 192 * i
    bad[off:off + 192] = _pt("g2", t["beta_mul_tau_g2"][i])
    assert _bh().CommonParamterInStorage.read(ctx, bytes(bad), checked=False).check(RHO) == sm.BETA_TAU_G2


# ------------------------------------------------------------------ 3. the mask is the equation
def test_cancelling_pair(ctx, honest8):
    """alpha_mul_tau_g2[5] += d and [2] -= d rho^3 cancel in S under rho and under no other base."""
    d = 0xD1FF
    s = changed(changed(honest8, "alpha_mul_tau_g2", 5, d), "alpha_mul_tau_g2", 2, -d * pow(RHO, 3, R) % R)
    assert sm.check_mask(s, RHO) == 0 and sm.check_mask(s, RHO + 1) == sm.ALPHA_TAU_G2
    st = storage(ctx, s)
    assert st.check(RHO) == 0
    assert st.check(RHO + 1) == sm.ALPHA_TAU_G2


# ------------------------------------------------------------------ 4. arguments
def test_arguments(ctx, honest8):
    bh = _bh()
    lib = bh.lib()
    st = storage(ctx, honest8)
    for bad in (0, R, R + 1, 2 ** 256 - 1):
        assert _raw_check(ctx, st, bh.fr_canonical_words(bad))[0] == INVALID_ARGUMENT
    with pytest.raises(bh.SynthesisError) as e:
        st.check(0)
    assert e.value.code == INVALID_ARGUMENT
    rho = bh.fr_canonical_words(RHO)
    p = rho.ctypes.data_as(ctypes.c_void_p)
    valid, mask, nxt = ctypes.c_int(), ctypes.c_uint32(), ctypes.c_void_p()
    assert lib.bh_mpc_common_check(None, st.h, p, ctypes.byref(valid), ctypes.byref(mask)) == INVALID_ARGUMENT
    assert lib.bh_mpc_common_check(ctx.h, None, p, ctypes.byref(valid), ctypes.byref(mask)) == INVALID_ARGUMENT
    assert lib.bh_mpc_common_check(ctx.h, st.h, None, ctypes.byref(valid), ctypes.byref(mask)) == INVALID_ARGUMENT
    assert lib.bh_mpc_common_check(ctx.h, st.h, p, None, ctypes.byref(mask)) == INVALID_ARGUMENT
    c = bh.mpc_common_paramters_generator(ctx, st, (2, 3, 5))
    args = [ctx.h, st.h, c.h, p, ctypes.byref(valid), ctypes.byref(mask), ctypes.byref(nxt)]
    for k in (0, 1, 2, 3, 4, 6):
        a = list(args)
        a[k] = None
        assert lib.bh_mpc_common_verify_structure(*a) == INVALID_ARGUMENT, k
    for bad in (0, R):
        a = list(args)
        a[3] = bh.fr_canonical_words(bad).ctypes.data_as(ctypes.c_void_p)
        assert lib.bh_mpc_common_verify_structure(*a) == INVALID_ARGUMENT
    if bh.device_count() > 1:  # handles of another context's device
        other = bh.Context(1)
        try:
            assert lib.bh_mpc_common_check(other.h, st.h, p, ctypes.byref(valid), ctypes.byref(mask)) == INVALID_ARGUMENT
            a = list(args)
            a[0] = other.h
            assert lib.bh_mpc_common_verify_structure(*a) == INVALID_ARGUMENT
        finally:
            other.close()
    # the context still works, and the timing stat is the last check's
    assert st.check(RHO) == 0
    ms = bh.last_check_ms()
    assert len(ms) == 2 and ms[0] > 0 and ms[1] > 0


# ------------------------------------------------------------------ 5. verify_structure
@pytest.mark.parametrize("n", [8, 257])
def test_honest_contribution(ctx, n):
    bh = _bh()
    st = bh.initial_common_paramters(ctx, n)
    st = bh.verify_common_paramter_structure(ctx, st, bh.mpc_common_paramters_generator(ctx, st, PLAYER), RHO)
    assert st is not None
    c = bh.mpc_common_paramters_generator(ctx, st, (PLAYER[1], PLAYER[2], PLAYER[0]))
    nxt, mask = bh.verify_common_paramter_structure(ctx, st, c, RHO, return_mask=True)
    assert mask == 0 and nxt is not None
    assert bh.verify_common_paramter_structure(ctx, st, c) is not None  # a fresh random rho
    assert nxt.write() == bh.verify_common_paramter(ctx, st, c).write()
    assert nxt.check(RHO) == 0


@pytest.fixture(scope="module")
def round8(honest8):
    new, mine = sm.contribute(honest8, *PLAYER)
    return honest8, new, mine


def _verify(ctx, old_st, new, mine, rho=RHO):
    return _bh().verify_common_paramter_structure(ctx, old_st, contrib(ctx, new, mine), rho, return_mask=True)


def test_contribution_from_logs_is_the_library_s(ctx, round8):
    bh = _bh()
    old, new, mine = round8
    st = storage(ctx, old)
    c = contrib(ctx, new, mine)
    assert c.write() == bh.mpc_common_paramters_generator(ctx, st, PLAYER).write()
    nxt, mask = bh.verify_common_paramter_structure(ctx, st, c, RHO, return_mask=True)
    assert mask == sm.verify_mask(old, new, mine, RHO) == 0
    assert nxt.write() == storage_bytes(ctx, new)


def test_factors_that_are_no_powers_are_refused(ctx, round8):
    """Tau results k_i * old_i with k_i no power sequence and "mine" lists consistent with the k_i:
    every per-element ratio proof holds, and the result is no power sequence."""
    bh = _bh()
    old, _, _ = round8
    ks = [1, 5, 6, 7, 8, 9, 10, 11]
    new, mine = sm.contribute(old, PLAYER[0], PLAYER[1], 5, factors=ks)
    st = storage(ctx, old)
    c = contrib(ctx, new, mine)
    nxt, mask = bh.verify_common_paramter_structure(ctx, st, c, RHO, return_mask=True)
    elementwise = bh.verify_common_paramter(ctx, st, c) is not None
    note = f"bh_mpc_common_verify {'accepts' if elementwise else 'refuses'} this contribution"
    assert nxt is None, note
    assert mask & sm.POWERS, note
    assert mask == sm.verify_mask(old, new, mine, RHO), note


@pytest.mark.parametrize("what,bit", [("alpha_g2", sm.ALPHA_RATIO), ("beta_g2", sm.BETA_RATIO),
                                      ("tau_g2", sm.TAU_RATIO)])
def test_wrong_mine(ctx, round8, what, bit):
    old, new, mine = round8
    bad = changed(mine, what, 1, 1)
    assert sm.verify_mask(old, new, bad, RHO) == bit
    nxt, mask = _verify(ctx, storage(ctx, old), new, bad)
    assert nxt is None and mask == bit


def test_changed_results(ctx, round8):
    old, new, mine = round8
    st = storage(ctx, old)
    for name, i in (("alpha_g1", None), ("beta_g2", None), ("tau_g1", 1), ("tau_g1", 7), ("beta_mul_tau_g2", 3)):
        bad = changed(new, name, i, 1)
        want = sm.verify_mask(old, bad, mine, RHO)
        assert want != 0
        nxt, mask = _verify(ctx, st, bad, mine)
        assert nxt is None and mask == want, (name, i)


def test_short_vector(ctx, round8):
    old, new, mine = round8
    short_new = dict(new, beta_mul_tau_g1=new["beta_mul_tau_g1"][:-1], beta_mul_tau_g2=new["beta_mul_tau_g2"][:-1],
                     alpha_g1=1)  # and a wrong alpha, which is not looked at
    short_mine = dict(mine, beta_mul_tau_g1=mine["beta_mul_tau_g1"][:-1], beta_mul_tau_g2=mine["beta_mul_tau_g2"][:-1])
    assert sm.verify_mask(old, short_new, short_mine, RHO) == sm.LENGTHS
    nxt, mask = _verify(ctx, storage(ctx, old), short_new, short_mine)
    assert nxt is None and mask == sm.LENGTHS


def test_the_rest_of_the_mine_lists_is_not_read(ctx, round8):
    """The documented difference from bh_mpc_common_verify: only alpha's, beta's and tau[1]'s g2_mine
    are read."""
    bh = _bh()
    old, new, mine = round8
    junk = dict(mine)
    for name in sm.VECTORS:
        junk[name] = [(k + 77 + i) % R if (name, i) != ("tau_g2", 1) else k for i, k in enumerate(mine[name])]
    junk["alpha_g1"], junk["beta_g1"] = 123, 456
    assert sm.verify_mask(old, new, junk, RHO) == 0
    st = storage(ctx, old)
    c = contrib(ctx, new, junk)
    nxt, mask = bh.verify_common_paramter_structure(ctx, st, c, RHO, return_mask=True)
    assert mask == 0 and nxt is not None and nxt.write() == storage_bytes(ctx, new)
    assert bh.verify_common_paramter(ctx, st, c) is None  # the per-element verifier reads them


# ------------------------------------------------------------------ 6. scratch budget
def test_scratch_budget_still_fits(ctx, honest8):
    bh = _bh()
    st = storage(ctx, honest8)
    st.check(RHO)
    bh.verify_common_paramter_structure(ctx, st, bh.mpc_common_paramters_generator(ctx, st, (2, 3, 5)), RHO)
    rep = ctx.scratch_report()
    assert rep["fits"]
    assert rep["kernels_checked"] >= 7
