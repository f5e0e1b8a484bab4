"""The MPC ceremony's parameter rounds on the device (bh_srs_mul_each / _mul_powers / _sub_range,
bh_mpc_common_*, bh_mpc_uncommon_*) against tests/mpc_oracle.py, the restatement of the reference's
groth16/mpc.rs, and against bh_generate_parameters.  Bit-exact throughout.

Sizes follow the oracle's cost (a G1 scalar multiplication about 4 ms, a G2 one about 10 ms, a
pairing about 0.7 s on the CPU): the vector lengths sit on the wave (64) and block (256) edges of the
one-lane-per-point kernels, the verdict-against-the-reference cases run at length 1."""
import os
import random
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mpc_oracle as mo  # noqa: E402

pytestmark = pytest.mark.gpu

R = mo.R
SPECIAL = [1, 2, 15, 16, 17, 2 ** 128 - 1, 2 ** 128, (R - 1) // 2, R - 2, R - 1]
FULL = [0x5AB3F1C2D4E6978877665544332211FFEEDDCCBBAA99887766554433221100FF % R,
        0x6F0E1D2C3B4A59687786A5B4C3D2E1F00112233445566778899AABBCCDDEEFF1 % R]
assert all(x.bit_length() >= 254 for x in FULL)
UNEXPECTED_IDENTITY, INVALID_ARGUMENT = 1, 10


def _bh():
    import bellman_hip as bh
    return bh


# ------------------------------------------------------------------ shared oracle data (computed once)
class _Points:
    """257 bases per group: the generator, then random 64-bit multiples of it."""

    def __init__(self):
        rng = random.Random(20240611)
        self.k = [1] + [rng.getrandbits(64) | 1 for _ in range(256)]
        self.g1 = [mo.g1(k) for k in self.k]
        self.g2 = [mo.g2(k) for k in self.k]

    def pts(self, group, n):
        return (self.g1 if group == 1 else self.g2)[:n]


@pytest.fixture(scope="module")
def points():
    return _Points()


def _curve(group):
    return mo.G1 if group == 1 else mo.G2


def _enc(group, pts):
    f = mo.g1_bytes if group == 1 else mo.g2_bytes
    return b"".join(f(p) for p in pts)


def _bases(ctx, group, pts):
    return _bh().Bases(ctx, group, _enc(group, pts))


def _scalars(n, seed):
    """n scalars below r: the special ones (all of them once n allows, rotated by n otherwise) and
    full-width random ones."""
    rng = random.Random(seed)
    s = [SPECIAL[(i + n) % len(SPECIAL)] for i in range(min(n, len(SPECIAL)))]
    while len(s) < n:
        s.append(rng.randrange(1 << 254, R))
    rng.shuffle(s)
    return s


def _status(fn, *a, **kw):
    bh = _bh()
    with pytest.raises(bh.SynthesisError) as e:
        fn(*a, **kw)
    return e.value.code


# ------------------------------------------------------------------ 1. mul_each against the oracle
@pytest.mark.parametrize("group,n", [(1, 1), (1, 2), (1, 63), (1, 64), (1, 65), (1, 257),
                                     (2, 1), (2, 2), (2, 63), (2, 64), (2, 65), (2, 257)])
def test_mul_each(ctx, points, group, n):
    pts = points.pts(group, n)
    ks = _scalars(n, 100 * group + n)
    if n >= 63:
        assert set(SPECIAL) <= set(ks)
    C = _curve(group)
    want = _enc(group, [mo.mul(C, p, k) for p, k in zip(pts, ks)])
    got = _bases(ctx, group, pts).mul_each(ks)
    assert len(got) == n and got.group == group
    assert got.to_bytes() == want


# ------------------------------------------------------------------ 2. stride 0 and nbits
@pytest.mark.parametrize("group", [1, 2])
def test_one_scalar_for_the_vector(ctx, points, group):
    n = 65
    b = _bases(ctx, group, points.pts(group, n))
    C = _curve(group)
    for k in (FULL[0], 2 ** 128 - 1, 1):
        assert b.mul_each([k]).to_bytes() == b.mul_each([k] * n).to_bytes()
    assert b.mul_each([FULL[1]]).get(64) == _enc(group, [mo.mul(C, points.pts(group, n)[64], FULL[1])])


@pytest.mark.parametrize("group", [1, 2])
def test_bit_bound(ctx, points, group):
    n = 65
    rng = random.Random(7)
    ks = [2 ** 128 - 1, 2 ** 127, 1, 2] + [rng.getrandbits(128) | 1 for _ in range(n - 4)]
    b = _bases(ctx, group, points.pts(group, n))
    C = _curve(group)
    full = _enc(group, [mo.mul(C, p, k) for p, k in zip(points.pts(group, n), ks)])
    for nbits in (None, 128, 129, 131, 132, 252, 253, 255):  # every window count rule
        assert b.mul_each(ks, nbits=nbits).to_bytes() == full, nbits
    assert _status(b.mul_each, ks, nbits=256) == INVALID_ARGUMENT
    assert _status(b.mul_each, ks, nbits=0) == INVALID_ARGUMENT
    # a scalar wider than the bound is refused, not truncated
    assert _status(b.mul_each, ks[:-1] + [2 ** 128], nbits=128) == INVALID_ARGUMENT


# ------------------------------------------------------------------ 3. mul_powers
AX = {"one": (1, 1), "small": (3, 2), "full": (FULL[0], FULL[1])}


@pytest.mark.parametrize("invert", [0, 1])
@pytest.mark.parametrize("ax", AX)
@pytest.mark.parametrize("group,n", [(1, 255), (1, 256), (1, 257), (2, 65)])
def test_mul_powers(ctx, points, group, n, ax, invert):
    a, x = AX[ax]
    pts = points.pts(group, n)
    C = _curve(group)
    want = []
    for i, p in enumerate(pts):
        k = a * pow(x, i, R) % R
        want.append(mo.mul(C, p, pow(k, -1, R) if invert else k))
    assert _bases(ctx, group, pts).mul_powers(a, x, invert).to_bytes() == _enc(group, want)


def test_mul_powers_is_make_new_tau_paramter(ctx, points):
    """The restated make_new_tau_paramter itself (u64 operands, no overflow at this length)."""
    n = 8
    g1s, g2s = points.pts(1, n), points.pts(2, n)
    for invert in (False, True):
        want = mo.make_new_tau_paramter(5, 3, g1s, g2s, invert)
        assert _bases(ctx, 1, g1s).mul_powers(5, 3, invert).to_bytes() == _enc(1, [p.g1_result for p in want])
        assert _bases(ctx, 2, g2s).mul_powers(5, 3, invert).to_bytes() == _enc(2, [p.g2_result for p in want])


# ------------------------------------------------------------------ 4. sub_range
@pytest.mark.parametrize("group,n", [(1, 1), (1, 64), (1, 65), (1, 128), (2, 65)])
def test_sub_range(ctx, points, group, n):
    pts = points.pts(group, 257)
    b = _bases(ctx, group, pts)
    C = _curve(group)
    for lo1, lo2 in ((0, n), (257 - n, 0), (3, 5) if n + 5 <= 257 else (0, 1)):
        got = b.sub_range(lo1, lo2, n)
        assert got.to_bytes() == _enc(group, [mo.sub(C, pts[lo2 + i], pts[lo1 + i]) for i in range(n)])


@pytest.mark.parametrize("group", [1, 2])
def test_sub_range_equal_points(ctx, points, group):
    pts = list(points.pts(group, 70))
    pts[69] = pts[4]  # out[4] of (0, 65, 5) would be the identity
    b = _bases(ctx, group, pts)
    assert _status(b.sub_range, 0, 65, 5) == UNEXPECTED_IDENTITY
    assert len(b.sub_range(0, 65, 4)) == 4
    assert _status(b.sub_range, 3, 3, 1) == UNEXPECTED_IDENTITY


# ------------------------------------------------------------------ 5. statuses
@pytest.mark.parametrize("group", [1, 2])
def test_statuses(ctx, points, group):
    bh = _bh()
    n = 65
    pts = points.pts(group, n)
    b = _bases(ctx, group, pts)
    ks = _scalars(n, 5)
    for at in (0, 31, n - 1):  # a zero scalar, also hidden at the end
        assert _status(b.mul_each, ks[:at] + [0] + ks[at + 1:]) == UNEXPECTED_IDENTITY
    assert _status(b.mul_each, [0]) == UNEXPECTED_IDENTITY
    for bad in (R, R + 1, 2 ** 256 - 1):
        assert _status(b.mul_each, ks[:n - 1] + [bad]) == INVALID_ARGUMENT
        assert _status(b.mul_powers, bad, 2) == INVALID_ARGUMENT
        assert _status(b.mul_powers, 2, bad) == INVALID_ARGUMENT
    assert _status(b.mul_powers, 0, 2) == UNEXPECTED_IDENTITY
    assert _status(b.mul_powers, 2, 0, True) == UNEXPECTED_IDENTITY
    # mismatched lengths
    assert _status(b.mul_each, ks[:n - 1]) == INVALID_ARGUMENT
    assert _status(b.mul_each, ks + [1]) == INVALID_ARGUMENT
    # ranges outside the vector
    assert _status(b.sub_range, 0, 33, 33) == INVALID_ARGUMENT
    assert _status(b.sub_range, 64, 0, 2) == INVALID_ARGUMENT
    # an identity among the inputs
    inf = (b"\x40" + bytes(95)) if group == 1 else (b"\x40" + bytes(191))
    w = bh.Bases(ctx, group, _enc(group, pts[:3]) + inf + _enc(group, pts[3:5]))
    assert _status(w.mul_each, [1] * 6) == UNEXPECTED_IDENTITY
    assert _status(w.mul_powers, 1, 1) == UNEXPECTED_IDENTITY
    assert _status(w.sub_range, 0, 3, 1) == UNEXPECTED_IDENTITY
    assert len(w.sub_range(0, 1, 2)) == 2  # a range that avoids it
    # the context still works
    assert b.mul_each([1] * n).to_bytes() == _enc(group, pts)


def test_ceremony_statuses(ctx):
    bh = _bh()
    st = bh.initial_common_paramters(ctx, 4)
    for bad in ((0, 2, 3), (2, 0, 3), (2, 3, 0)):
        assert _status(bh.mpc_common_paramters_generator, ctx, st, bad) == UNEXPECTED_IDENTITY
    assert _status(bh.mpc_common_paramters_generator, ctx, st, (R, 2, 3)) == INVALID_ARGUMENT
    assert _status(st.h_basis, 3) == INVALID_ARGUMENT  # 2n > len
    h1 = bh.mpc_common_paramters_generator(ctx, st, (2, 3, 5))
    nxt = bh.verify_common_paramter(ctx, st, h1)
    a, b = nxt.h_basis(2)
    assert _status(bh.initial_uncommon_paramters, ctx, nxt.tau_g1, b, a, b, a, b) == INVALID_ARGUMENT  # 4 and 2
    assert _status(bh.initial_uncommon_paramters, ctx, b, a, a, b, a, b) == INVALID_ARGUMENT  # groups swapped
    ust = bh.initial_uncommon_paramters(ctx, a, b, a, b, a, b)
    assert _status(bh.mpc_uncommon_paramters_generator, ctx, ust, (0, 1)) == UNEXPECTED_IDENTITY
    assert _status(bh.mpc_uncommon_paramters_generator, ctx, ust, (1, R)) == INVALID_ARGUMENT
    with pytest.raises(bh.SynthesisError):  # a zero z
        bh.verify_common_paramter(ctx, st, h1, z=[1, 2, 0, 4])


# ------------------------------------------------------------------ 6. the reference ceremony
COMMON_PLAYERS = [(1, 2, 1), (2, 3, 1), (3, 4, 2)]
UNCOMMON_PLAYERS = [(1, 2), (2, 3), (3, 4)]


def test_reference_ceremony(ctx):
    """mpc_common_paramters_custom_all / mpc_uncommon_paramters_custom_all (mpc.rs:864-888,
    959-991): length 8, verified after every player, byte-equal to the restatement."""
    bh = _bh()
    st, ost = bh.initial_common_paramters(ctx, 8), mo.initial_common_paramters(8)
    assert st.write() == mo.common_storage_bytes(ost)
    for player in COMMON_PLAYERS:
        c, oc = bh.mpc_common_paramters_generator(ctx, st, player), mo.mpc_common_paramters_generator(ost, player)
        assert c.write() == oc.bytes()
        st, ost = bh.verify_common_paramter(ctx, st, c), oc.to_storage_format()
        assert st is not None and st.write() == mo.common_storage_bytes(ost)
    assert len(st) == 8
    assert st.tau_g1.get(1) == mo.g1_bytes(mo.g1(2))
    assert st.alpha_mul_tau_g1.to_bytes()[:192] == mo.g1_bytes(mo.g1(6)) + mo.g1_bytes(mo.g1(12))
    assert st.beta_mul_tau_g1.to_bytes()[:192] == mo.g1_bytes(mo.g1(24)) + mo.g1_bytes(mo.g1(48))
    assert st.alpha_g1 == mo.g1_bytes(mo.g1(6)) and st.beta_g1 == mo.g1_bytes(mo.g1(24))
    # round-trips, and a corrupted point
    data = st.write()
    assert bh.CommonParamterInStorage.read(ctx, data, checked=True).write() == data
    assert bh.CommonParamterInStorage.read(ctx, data, checked=False).write() == data
    bad = bytearray(data)
    bad[4 + 576 + 96 * 3 + 95] ^= 1  # y of tau_g1[3]
    with pytest.raises(bh.SynthesisError):
        bh.CommonParamterInStorage.read(ctx, bytes(bad), checked=True)
    with pytest.raises(bh.SynthesisError):
        bh.CommonParamterInStorage.read(ctx, data[:-1], checked=True)
    # round two on the h basis and two slices of round one
    h1, h2 = st.h_basis(4)
    oh1, oh2 = mo.h_basis(ost, 4)
    assert h1.to_bytes() == _enc(1, oh1) and h2.to_bytes() == _enc(2, oh2)
    omatrix = {"front_g1": ost.alpha_mul_tau_g1[:3], "front_g2": ost.alpha_mul_tau_g2[:3],
               "back_g1": ost.beta_mul_tau_g1[:2], "back_g2": ost.beta_mul_tau_g2[:2], "h_g1": oh1, "h_g2": oh2}
    matrix = bh.initial_uncommon_paramters(ctx, *[_bases(ctx, 1 + (i & 1), omatrix[k]) for i, k in enumerate(
        ("front_g1", "front_g2", "back_g1", "back_g2", "h_g1", "h_g2"))])
    ust, oust = matrix, mo.initial_uncommon_paramters(omatrix)
    assert ust.write() == mo.uncommon_storage_bytes(oust)
    for player in UNCOMMON_PLAYERS:
        c, oc = bh.mpc_uncommon_paramters_generator(ctx, ust, player), mo.mpc_uncommon_paramters_generator(oust, player)
        assert c.write() == oc.bytes()
        ust, oust = bh.verify_uncommon_paramter(ctx, matrix, ust, c), oc.to_storage_format()
        assert ust is not None and ust.write() == mo.uncommon_storage_bytes(oust)
    assert ust.gamma_g2 == mo.g2_bytes(mo.g2(6)) and ust.delta_g1 == mo.g1_bytes(mo.g1(24))
    data = ust.write()
    assert bh.UnCommonParamterInStorage.read(ctx, data, checked=True).write() == data
    cdata = c.write()
    assert bh.UnCommonParamter.read(ctx, cdata, checked=True).write() == cdata
    bad = bytearray(data)
    bad[-1] ^= 1
    with pytest.raises(bh.SynthesisError):
        bh.UnCommonParamterInStorage.read(ctx, bytes(bad), checked=True)


# ------------------------------------------------------------------ 7. verification verdicts
PAIR = 576                       # g1_result 96 | g2_result 192 | g1_mine 96 | g2_mine 192
R1, R2, M1, M2 = 0, 96, 288, 384


def _list_at(data, j):
    """(offset of list j's first ParameterPair, its length) in a contribution's bytes."""
    o = 2 * PAIR
    for _ in range(j):
        o += 4 + int.from_bytes(data[o:o + 4], "big") * PAIR
    return o + 4, int.from_bytes(data[o:o + 4], "big")


def _put(data, off, blob):
    data[off:off + len(blob)] = blob


def _g1_at(data, off):
    return mo.bls.g1_from_uncompressed(bytes(data[off:off + 96]), checked=False)[1]


def _g2_at(data, off):
    return mo.bls.g2_from_uncompressed(bytes(data[off:off + 192]), checked=False)[1]


@pytest.fixture(scope="module")
def verdict_case(ctx):
    bh = _bh()
    st = bh.initial_common_paramters(ctx, 5)
    st = bh.verify_common_paramter(ctx, st, bh.mpc_common_paramters_generator(ctx, st, (FULL[0], 11, 7)))
    c = bh.mpc_common_paramters_generator(ctx, st, (3, FULL[1], 5))
    return st, c.write()


def _verdict(ctx, st, data, z=None):
    bh = _bh()
    z = [3 + 2 ** 127 + 1000003 * i * i for i in range(5)] if z is None else z
    return bh.verify_common_paramter(ctx, st, bh.CommonParamter.read(ctx, bytes(data), checked=False), z=z) is not None


def test_honest_contribution_is_accepted(ctx, verdict_case):
    st, data = verdict_case
    assert _verdict(ctx, st, data)
    assert _verdict(ctx, st, data, z=[1] * 5)
    assert _verdict(ctx, st, data, z=[R - 1 - i for i in range(5)])


@pytest.mark.parametrize("what", ["r1_0", "r1_2", "r1_4", "r1_beta_4", "r2", "m2", "alpha", "beta_g2", "short",
                                  "cancelling"])
def test_tampered_contribution_is_refused(ctx, verdict_case, what):
    st, honest = verdict_case
    data = bytearray(honest)
    a_off, n = _list_at(data, 1)   # alpha_mul_tau
    b_off, _ = _list_at(data, 2)   # beta_mul_tau
    assert n == 5
    if what.startswith("r1_beta"):
        _put(data, b_off + 4 * PAIR + R1, mo.g1_bytes(mo.g1(987654321)))
    elif what.startswith("r1_"):
        _put(data, a_off + int(what[3:]) * PAIR + R1, mo.g1_bytes(mo.g1(123456789 + int(what[3:]))))
    elif what == "r2":      # R2_i no longer the G2 image of R1_i
        _put(data, a_off + 1 * PAIR + R2, mo.g2_bytes(mo.g2(31337)))
    elif what == "m2":      # a wrong "mine"
        _put(data, a_off + 3 * PAIR + M2, mo.g2_bytes(mo.g2(4242)))
    elif what == "alpha":
        _put(data, R1, mo.g1_bytes(mo.g1(77)))
    elif what == "beta_g2":
        _put(data, PAIR + R2, mo.g2_bytes(mo.g2(78)))
    elif what == "short":   # beta_mul_tau one element short
        del data[b_off + 4 * PAIR:b_off + 5 * PAIR]
        _put(data, b_off - 4, (4).to_bytes(4, "big"))
    elif what == "cancelling":
        # R1_1 += D, R1_3 -= D and R2 likewise: both sums are unchanged when all z are equal
        d = 0xD1FF
        for i, sign in ((1, 1), (3, -1)):
            o = a_off + i * PAIR
            k = d * sign % R
            _put(data, o + R1, mo.g1_bytes(mo.G1.to_affine(mo.G1.add(mo.G1.from_affine(_g1_at(data, o + R1)),
                                                                      mo.G1.from_affine(mo.g1(k))))))
            _put(data, o + R2, mo.g2_bytes(mo.G2.to_affine(mo.G2.add(mo.G2.from_affine(_g2_at(data, o + R2)),
                                                                      mo.G2.from_affine(mo.g2(k))))))
        assert _verdict(ctx, st, data, z=[9] * 5)  # why the z must be independent
    assert not _verdict(ctx, st, data)


# ------------------------------------------------------------------ 8. the verdict is the reference's
# The restated per-element checks (Python pairings, one final exponentiation each) and the batched
# device verification agree, at length 1; honest and tampered are separate cases for their run time.
@pytest.fixture(scope="module")
def common_len1(ctx):
    bh = _bh()
    players = [(5, 7, 3), (FULL[0], 2, FULL[1])]
    st, ost = bh.initial_common_paramters(ctx, 1), mo.initial_common_paramters(1)
    c0, oc0 = bh.mpc_common_paramters_generator(ctx, st, players[0]), mo.mpc_common_paramters_generator(ost, players[0])
    st, ost = bh.verify_common_paramter(ctx, st, c0), oc0.to_storage_format()
    return st, ost, players[1]


@pytest.mark.parametrize("tamper", [False, True])
def test_verdict_equals_reference_common(ctx, common_len1, tamper):
    bh = _bh()
    st, ost, player = common_len1
    oc = mo.mpc_common_paramters_generator(ost, player)
    assert bh.mpc_common_paramters_generator(ctx, st, player).write() == oc.bytes()
    if tamper:
        oc.alpha_mul_tau[0].g2_mine = mo.g2(99)
    c = bh.CommonParamter.read(ctx, oc.bytes(), checked=True)
    want = mo.verify_common_paramter(ost, oc) is not None
    assert want == (not tamper)
    assert (bh.verify_common_paramter(ctx, st, c, z=[2 ** 128 - 159]) is not None) == want


@pytest.mark.parametrize("tamper", [False, True])
def test_verdict_equals_reference_uncommon(ctx, tamper):
    bh = _bh()
    omatrix = {"front_g1": [mo.g1(11)], "front_g2": [mo.g2(11)], "back_g1": [mo.g1(13)], "back_g2": [mo.g2(13)],
               "h_g1": [mo.g1(17)], "h_g2": [mo.g2(17)]}
    matrix = bh.initial_uncommon_paramters(ctx, *[_bases(ctx, 1 + (i & 1), omatrix[k]) for i, k in enumerate(
        ("front_g1", "front_g2", "back_g1", "back_g2", "h_g1", "h_g2"))])
    oust = mo.initial_uncommon_paramters(omatrix)
    player = (FULL[1], 5)
    oc = mo.mpc_uncommon_paramters_generator(oust, player)
    assert bh.mpc_uncommon_paramters_generator(ctx, matrix, player).write() == oc.bytes()
    if tamper:
        oc.l[0].g1_result = mo.g1(1234)  # kout no longer matrix / delta
    c = bh.UnCommonParamter.read(ctx, oc.bytes(), checked=True)
    want = mo.verify_uncommon_paramter(omatrix, oust, oc) is not None
    assert want == (not tamper)
    assert (bh.verify_uncommon_paramter(ctx, matrix, matrix, c, z=[2 ** 127 + 5]) is not None) == want


# ------------------------------------------------------------------ 9. against the existing generator
def _generator_case(ctx, name):
    bh = _bh()
    if name == "and":
        from oracle import circuits as cc
        return bh.R1CS.from_assembly(ctx, bh.synthesize_keypair(cc.AndDemo(None, None)))
    return bh.R1CS.chain(ctx, 127)  # 2 * 127 + 2 = 256 constraints with the input rows


@pytest.mark.parametrize("name,m", [("and", 4), ("chain", 256)])
def test_against_generate_parameters(ctx, name, m):
    """n = m, the reference's own condition: one player per round from an initial storage of
    length 2m gives generate_parameters' h query and verifying key for the same toxic waste."""
    bh = _bh()
    r1cs = _generator_case(ctx, name)
    assert r1cs.sizes()["constraints"] == m
    alpha, beta, gamma, delta, tau = FULL[0], 24, 6, FULL[1], 0x1234567890ABCDEF1122334455667788
    params = bh.Parameters.generate(ctx, r1cs, alpha=alpha, beta=beta, gamma=gamma, delta=delta, tau=tau)
    st = bh.initial_common_paramters(ctx, 2 * m)
    st = bh.verify_common_paramter(ctx, st, bh.mpc_common_paramters_generator(ctx, st, (alpha, beta, tau)))
    assert st is not None
    h1, h2 = st.h_basis(m)
    matrix = bh.initial_uncommon_paramters(ctx, st.alpha_mul_tau_g1, st.alpha_mul_tau_g2, st.beta_mul_tau_g1,
                                           st.beta_mul_tau_g2, h1, h2)
    ust = bh.verify_uncommon_paramter(ctx, matrix, matrix, bh.mpc_uncommon_paramters_generator(ctx, matrix, (gamma, delta)))
    assert ust is not None
    hq = params.vector(bh.BH_VEC_H)
    assert len(hq) == m - 1
    want = b"".join(bh.Bases.get(hq, i) for i in range(m - 1))
    assert ust.h_g1.to_bytes()[:96 * (m - 1)] == want
    vk = params.vk_bytes()  # alpha_g1 | beta_g1 | beta_g2 | gamma_g2 | delta_g1 | delta_g2 | ic
    assert st.alpha_g1 == vk[0:96] and st.beta_g1 == vk[96:192] and st.beta_g2 == vk[192:384]
    assert ust.gamma_g2 == vk[384:576] and ust.delta_g1 == vk[576:672] and ust.delta_g2 == vk[672:864]


# ------------------------------------------------------------------ 10. scratch budget
def test_scratch_budget_still_fits(ctx, points):
    b = _bases(ctx, 2, points.pts(2, 65))
    b.mul_each([FULL[0]] * 65)
    rep = ctx.scratch_report()
    assert rep["fits"]
    assert rep["kernels_checked"] >= 7  # the varbase kernels are in the list
