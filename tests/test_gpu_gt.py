"""Gt vectors on the device (csrc/gt.hip behind bh_gt_*; bellman_hip.Gt, pairing, multiexp_gt)
against the oracle's Fp12 arithmetic on powers of one pairing value (tests/gt_values.py).  Field
arithmetic is exact: every comparison is an equality of all 576 bytes per element.

Lengths sit on the edges of the 64-lane block (0, 1, 63, 64, 65, 130); chosen values stand in lanes
0, 63, 64 and n - 1.  Expected values are E^k for a few dozen distinct k, kept per k."""
import ctypes
import random

import numpy as np
import pytest

import gt_values as gv
import proof_cases as pc
from final_exp_values import SPECIAL, random_values, special_values
from oracle import bls12_381 as bls
from oracle import pairing as pr

pytestmark = pytest.mark.gpu

G1, G2 = bls.G1, bls.G2
R = gv.R
DEGENERATE = 16
ONE_BYTES = gv.gt_format(gv.ONE)
_g1_cache, _g2_cache = {}, {}


def _bh():
    import bellman_hip as bh
    return bh


def _g1(k):
    """k G1 as uncompressed bytes (k = 0: the identity), kept per scalar"""
    if k not in _g1_cache:
        _g1_cache[k] = bls.g1_to_uncompressed(G1.to_affine(G1.mul(G1.generator(), k)) if k else None)
    return _g1_cache[k]


def _g2(k):
    if k not in _g2_cache:
        _g2_cache[k] = bls.g2_to_uncompressed(G2.to_affine(G2.mul(G2.generator(), k)) if k else None)
    return _g2_cache[k]


def _bases(ctx, a, b):
    bh = _bh()
    return (bh.Bases(ctx, bh.BH_G1, b"".join(_g1(k) for k in a), checked=False),
            bh.Bases(ctx, bh.BH_G2, b"".join(_g2(k) for k in b), checked=False))


def _powers(ks):
    """gt_format of E^k for each k"""
    return b"".join(gv.gt_format(gv.power(k)) for k in ks)


def _split(blob):
    return [blob[576 * i:576 * i + 576] for i in range(len(blob) // 576)]


def _assert_elements(got, want, what):
    assert len(got) == len(want), what
    for lane, (g, w) in enumerate(zip(_split(got), _split(want))):
        assert g == w, (what, lane)


# ---------------------------------------------------------------- pairing
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 130])
def test_pairing_equals_the_power_of_the_generators_pairing(ctx, n):
    a, b = gv.tiled(n), gv.tiled(n, 5)
    g1, g2 = _bases(ctx, a, b)
    got = _bh().pairing(ctx, g1, g2)
    assert len(got) == n
    _assert_elements(got.to_bytes(), _powers(x * y for x, y in zip(a, b)), n)


def test_pairing_with_offsets_into_longer_vectors(ctx):
    g1, g2 = _bases(ctx, gv.tiled(70), gv.tiled(72, 3))
    off1, off2, n = 3, 5, 65  # pair i: the scalars at 3 + i and (5 + i) + 3, five apart as above
    got = _bh().pairing(ctx, g1, g2, off1, off2, n)
    s = gv.tiled(100)
    _assert_elements(got.to_bytes(), _powers(s[off1 + i] * s[off1 + i + 5] for i in range(n)), "offsets")
    tail = _bh().pairing(ctx, g1, g2, 69, 71, 1)
    assert tail.to_bytes() == _powers([s[69] * s[74]])


@pytest.mark.parametrize("n", [65, 130])
def test_an_identity_on_either_side_gives_one(ctx, n):
    a, b = [3] * n, [5] * n
    a[0] = 0
    b[63] = 0
    a[n - 1] = b[n - 1] = 0
    g1, g2 = _bases(ctx, a, b)
    got = _split(_bh().pairing(ctx, g1, g2).to_bytes())
    for lane in range(n):
        assert got[lane] == (ONE_BYTES if lane in (0, 63, n - 1) else _powers([15])), lane


def test_the_generators_pairing_is_the_reference_fixture(ctx):
    g1, g2 = _bases(ctx, [1], [1])
    assert _bh().pairing(ctx, g1, g2).to_bytes() == gv.fixture_bytes()


# ---------------------------------------------------------------- from_miller
def test_from_miller_equals_pairing(ctx):
    bh = _bh()
    a, b = gv.tiled(6, 1), gv.tiled(6, 6)
    g1, g2 = _bases(ctx, a, b)
    millers = [bh.multi_miller_loop(ctx, g1, g2, i, i, 1) for i in range(6)]
    want = bh.pairing(ctx, g1, g2).to_bytes()
    assert bh.Gt.from_miller(ctx, millers).to_bytes() == want
    # across the block edge: the same six values tiled over 130 lanes
    got = bh.Gt.from_miller(ctx, [millers[i % 6] for i in range(130)]).to_bytes()
    _assert_elements(got, b"".join(_split(want)[i % 6] for i in range(130)), "tiled")
    assert len(bh.Gt.from_miller(ctx, [])) == 0


def test_a_product_of_miller_values_maps_to_the_sum(ctx):
    bh = _bh()
    g1, g2 = _bases(ctx, [7, 9], [2, 16])
    product = bh.multi_miller_loop(ctx, g1, g2, 0, 0, 2)
    both = bh.pairing(ctx, g1, g2, 0, 0, 1) + bh.pairing(ctx, g1, g2, 1, 1, 1)
    assert bh.Gt.from_miller(ctx, [product]).to_bytes() == both.to_bytes() == _powers([7 * 2 + 9 * 16])


# ---------------------------------------------------------------- exponentiation
@pytest.mark.parametrize("n", [1, 63, 64, 65, 130])
def test_mul_each_every_chosen_scalar_in_every_chosen_lane(ctx, n):
    bh = _bh()
    base = bh.Gt.from_bytes(ctx, _powers([1 + (i & 1) for i in range(n)]), checked=False)
    # every rotation of the scalar list: each scalar visits lanes 0, 63, 64 and n - 1.  The list's
    # length is even, so (1 + (i & 1)) s_i takes 2 x 16 distinct values over all rotations and lengths
    for shift in range(len(gv.chosen_scalars())):
        s = gv.tiled(n, shift)
        _assert_elements((base * s).to_bytes(), _powers((1 + (i & 1)) * s[i] for i in range(n)), (n, shift))


def test_one_scalar_for_every_element(ctx):
    bh = _bh()
    n = 65
    base = bh.Gt.from_bytes(ctx, _powers(range(1, n + 1)))
    for k in (gv.chosen_scalars()[9], 0, R - 1):
        assert (base * k).to_bytes() == (base * ([k] * n)).to_bytes()
    assert (base * 0).to_bytes() == ONE_BYTES * n
    assert (base * (R - 1)).to_bytes() == (-base).to_bytes()
    assert (base * 2).to_bytes() == (base + base).to_bytes()


# ---------------------------------------------------------------- group operations
@pytest.mark.parametrize("n", [1, 64, 65, 130])
def test_add_neg_sum_and_multiexp(ctx, n):
    bh = _bh()
    ka, kb = gv.tiled(n, 2), gv.tiled(n, 7)
    va, vb = [gv.power(k) for k in ka], [gv.power(k) for k in kb]
    a = bh.Gt.from_bytes(ctx, b"".join(gv.gt_format(v) for v in va))
    b = bh.Gt.from_bytes(ctx, b"".join(gv.gt_format(v) for v in vb))
    _assert_elements((a + b).to_bytes(), b"".join(gv.gt_format(pr.f12_mul(x, y)) for x, y in zip(va, vb)), "add")
    _assert_elements((-a).to_bytes(), b"".join(gv.gt_format(gv.conj(x)) for x in va), "neg")
    assert (a + (-a)).to_bytes() == ONE_BYTES * n
    total = gv.ONE
    for x in va:
        total = pr.f12_mul(total, x)
    assert a.sum() == gv.gt_format(total)
    s = gv.tiled(n, 11)
    assert bh.multiexp_gt(ctx, a, s) == _powers([sum(k * x for k, x in zip(ka, s))])


def test_sum_of_nothing_is_one(ctx):
    bh = _bh()
    empty = bh.Gt.from_bytes(ctx, b"")
    assert len(empty) == 0 and empty.sum() == ONE_BYTES and bh.multiexp_gt(ctx, empty, []) == ONE_BYTES
    assert (empty + empty).to_bytes() == (-empty).to_bytes() == (empty * []).to_bytes() == b""


def test_bilinearity_with_the_g1_multiexp(ctx):
    """multiexp_gt(pairing(P_i, Q), s) = pairing(sum s_i P_i, Q), the left point from bh_multiexp"""
    bh = _bh()
    n = 65
    a = [k or 3 for k in gv.tiled(n, 4)]
    s = [k or 5 for k in gv.tiled(n, 9)]
    g1, g2 = _bases(ctx, a, [1] * n)
    left = bh.multiexp_gt(ctx, bh.pairing(ctx, g1, g2), s)
    point = bh.multiexp(ctx, g1, 0, None, s)
    g1s = bh.Bases(ctx, bh.BH_G1, point, checked=False)
    assert left == bh.pairing(ctx, g1s, g2, 0, 0, 1).to_bytes() == _powers([sum(x * y for x, y in zip(a, s))])


# ---------------------------------------------------------------- codec
def test_upload_then_read_is_byte_identical(ctx):
    bh = _bh()
    blob = _powers(gv.tiled(130, 1))
    for checked in (False, True):
        g = bh.Gt.from_bytes(ctx, blob, checked=checked)
        assert g.to_bytes() == blob
        assert g.read(63, 2) == blob[576 * 63:576 * 65] and g.read(129) == blob[576 * 129:] and g.read(130) == b""
    junk = b"".join(gv.gt_format(v) for v in random_values(3, seed=9))  # unchecked: any canonical value
    assert bh.Gt.from_bytes(ctx, junk, checked=False).to_bytes() == junk


@pytest.mark.parametrize("lane", [0, 63, 64, 129])
def test_a_coefficient_equal_to_p_is_an_invalid_encoding(ctx, lane):
    bh = _bh()
    good = _powers(gv.tiled(130, 1))
    for position in range(12):
        blob = bytearray(good)
        off = 576 * lane + 48 * position
        blob[off:off + 48] = gv.P.to_bytes(48, "big")
        for checked in (False, True) if position in (0, 11) else (False,):
            with pytest.raises(bh.SynthesisError) as e:
                bh.Gt.from_bytes(ctx, bytes(blob), checked=checked)
            assert e.value.code == pc.INVALID_ENCODING, (position, checked)
        blob[off:off + 48] = (gv.P - 1).to_bytes(48, "big")  # the largest canonical coefficient
        assert bh.Gt.from_bytes(ctx, bytes(blob), checked=False).read(lane, 1) == bytes(blob[576 * lane:576 * lane + 576])


@pytest.mark.parametrize("lane", [0, 63, 64, 129])
def test_checked_upload_refuses_values_outside_gt(ctx, lane):
    bh = _bh()
    good = _powers(gv.tiled(130, 1))
    assert len(bh.Gt.from_bytes(ctx, good, checked=True)) == 130
    w3 = [(0, 0)] * 3 + [(1, 0)] + [(0, 0)] * 2
    for name, v in [("zero", gv.ZERO), ("w^3", w3), ("random", gv.random_f12(6)), ("cyclotomic", gv.non_member())]:
        blob = bytearray(good)
        blob[576 * lane:576 * lane + 576] = gv.gt_format(v)
        with pytest.raises(bh.SynthesisError) as e:
            bh.Gt.from_bytes(ctx, bytes(blob), checked=True)
        assert e.value.code == pc.NOT_IN_SUBGROUP, name
        assert bh.Gt.from_bytes(ctx, bytes(blob), checked=False).read(lane, 1) == gv.gt_format(v)  # and no fault


# ---------------------------------------------------------------- the squaring formula
def test_selftest_squaring_formula_equals_the_model(ctx):
    fn = _bh().lib().bh_selftest_gt_cyclotomic_square
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    vals = [v for _, v in special_values()] + random_values(30, seed=13)
    assert len(vals) == len(SPECIAL) + 30
    batches = [vals]
    for rnd in range(len(SPECIAL) // 4):  # four chosen values per round in lanes 0, 63, 64 and 129
        batch = [vals[len(SPECIAL) + (7 * i + rnd) % 30] for i in range(130)]
        for lane, v in zip((0, 63, 64, 129), vals[4 * rnd:4 * rnd + 4]):
            batch[lane] = v
        batches.append(batch)
    for batch in batches:
        src = np.frombuffer(b"".join(gv.flat_bytes(v) for v in batch), dtype=np.uint8)
        out = np.full(576 * len(batch), 0xAA, dtype=np.uint8)
        assert fn(ctx.h, src.ctypes.data_as(ctypes.c_void_p), len(batch), out.ctypes.data_as(ctypes.c_void_p)) == 0
        for lane, (g, v) in enumerate(zip(_split(out.tobytes()), batch)):
            assert gv.flat_parse(g) == gv.cyclotomic_square_model(v), lane
    e = gv.generator_pairing()  # on a Gt element the formula is the square
    src = np.frombuffer(gv.flat_bytes(e), dtype=np.uint8)
    out = np.zeros(576, dtype=np.uint8)
    assert fn(ctx.h, src.ctypes.data_as(ctypes.c_void_p), 1, out.ctypes.data_as(ctypes.c_void_p)) == 0
    assert gv.flat_parse(out.tobytes()) == gv.power(2)


# ---------------------------------------------------------------- errors
def test_errors_create_nothing(ctx):
    bh = _bh()
    lib = bh.lib()
    g1, g2 = _bases(ctx, [1, 2, 3], [1, 2, 3])
    a = bh.Gt.from_bytes(ctx, _powers([1, 2, 3]))
    b = bh.Gt.from_bytes(ctx, _powers([1, 2]))
    sentinel = 0x5A5A

    def fails(call, code=pc.INVALID_ARGUMENT):
        h = ctypes.c_void_p(sentinel)
        assert call(ctypes.byref(h)) == code
        assert h.value == sentinel

    buf = np.zeros(576 * 3, dtype=np.uint8)
    p = buf.ctypes.data_as(ctypes.c_void_p)
    k = np.ascontiguousarray(np.stack([bh.fr_canonical_words(x) for x in (1, 2, R)]))
    kp = k.ctypes.data_as(ctypes.c_void_p)
    # null pointers
    fails(lambda h: lib.bh_gt_pairing(None, g1.h, 0, g2.h, 0, 1, h))
    fails(lambda h: lib.bh_gt_pairing(ctx.h, None, 0, g2.h, 0, 1, h))
    fails(lambda h: lib.bh_gt_pairing(ctx.h, g1.h, 0, None, 0, 1, h))
    assert lib.bh_gt_pairing(ctx.h, g1.h, 0, g2.h, 0, 1, None) == pc.INVALID_ARGUMENT
    fails(lambda h: lib.bh_gt_from_miller(ctx.h, None, 1, h))
    fails(lambda h: lib.bh_gt_upload(ctx.h, None, 1, 1, h))
    fails(lambda h: lib.bh_gt_upload(None, p, 1, 1, h))
    fails(lambda h: lib.bh_gt_add(ctx.h, a.h, None, h))
    fails(lambda h: lib.bh_gt_neg(ctx.h, None, h))
    fails(lambda h: lib.bh_gt_mul_each(ctx.h, a.h, None, 3, h))
    assert lib.bh_gt_read(None, 0, 1, p) == pc.INVALID_ARGUMENT
    assert lib.bh_gt_read(a.h, 0, 1, None) == pc.INVALID_ARGUMENT
    assert lib.bh_gt_sum(ctx.h, a.h, None) == lib.bh_gt_sum(ctx.h, None, p) == pc.INVALID_ARGUMENT
    assert lib.bh_gt_multiexp(ctx.h, a.h, None, p) == lib.bh_gt_multiexp(ctx.h, a.h, kp, None) == pc.INVALID_ARGUMENT
    assert lib.bh_gt_len(None) == 0 and lib.bh_gt_free(None) == 0
    # mismatched lengths
    fails(lambda h: lib.bh_gt_add(ctx.h, a.h, b.h, h))
    fails(lambda h: lib.bh_gt_mul_each(ctx.h, a.h, kp, 2, h))
    # a scalar equal to r
    fails(lambda h: lib.bh_gt_mul_each(ctx.h, a.h, kp, 3, h))
    assert lib.bh_gt_multiexp(ctx.h, a.h, kp, p) == pc.INVALID_ARGUMENT
    # ranges past the end
    fails(lambda h: lib.bh_gt_pairing(ctx.h, g1.h, 1, g2.h, 0, 3, h))
    fails(lambda h: lib.bh_gt_pairing(ctx.h, g1.h, 0, g2.h, 4, 0, h))
    assert lib.bh_gt_read(a.h, 2, 2, p) == lib.bh_gt_read(a.h, 4, 0, p) == pc.INVALID_ARGUMENT
    # a G2 vector where G1 is expected, and the reverse
    fails(lambda h: lib.bh_gt_pairing(ctx.h, g2.h, 0, g2.h, 0, 1, h))
    fails(lambda h: lib.bh_gt_pairing(ctx.h, g1.h, 0, g1.h, 0, 1, h))
    # a coefficient >= p among Miller values
    bad = bytearray(gv.flat_bytes(gv.ONE) * 2)
    bad[576 + 48 * 7:576 + 48 * 8] = gv.P.to_bytes(48, "big")
    src = np.frombuffer(bytes(bad), dtype=np.uint8)
    fails(lambda h: lib.bh_gt_from_miller(ctx.h, src.ctypes.data_as(ctypes.c_void_p), 2, h), pc.INVALID_ENCODING)
    # n = 0 is fine everywhere
    assert len(bh.pairing(ctx, g1, g2, 3, 3, 0)) == 0
    assert lib.bh_gt_read(a.h, 3, 0, None) == 0


def test_a_twist_point_outside_the_subgroup_is_degenerate_and_makes_no_vector(ctx):
    """A twist point of order 13 (a cofactor multiple of a seeded random twist point: 13^2 divides the
    twist's cofactor h2 and its 13-part has exponent 13) makes the second addition step divide by zero."""
    bh = _bh()
    x = -gv.X_ABS
    h2 = (x ** 8 - 4 * x ** 7 + 5 * x ** 6 - 4 * x ** 4 + 6 * x ** 3 - 4 * x ** 2 - 4 * x + 13) // 9
    rng = random.Random(13)
    q = None
    while q is None:
        xs = (rng.randrange(gv.P), rng.randrange(gv.P))
        ys = pr._fp2_sqrt(bls.Fp2Ops.add(bls.Fp2Ops.mul(bls.Fp2Ops.sqr(xs), xs), (4, 4)))
        if ys is not None:
            q = G2.to_affine(G2.mul(G2.from_affine((xs, ys)), R * h2 // 169))
    assert G2.to_affine(G2.mul(G2.from_affine(q), 13)) is None
    g1 = bh.Bases(ctx, bh.BH_G1, _g1(1), checked=False)
    g2 = bh.Bases(ctx, bh.BH_G2, bls.g2_to_uncompressed(q), checked=False)
    h = ctypes.c_void_p(0x5A5A)
    assert bh.lib().bh_gt_pairing(ctx.h, g1.h, 0, g2.h, 0, 1, ctypes.byref(h)) == DEGENERATE
    assert h.value == 0x5A5A


# ---------------------------------------------------------------- scratch budget
def test_scratch_budget_after_every_entry_point(ctx):
    bh = _bh()
    g1, g2 = _bases(ctx, [1, 2], [3, 1])
    a = bh.pairing(ctx, g1, g2)
    b = bh.Gt.from_miller(ctx, [bh.multi_miller_loop(ctx, g1, g2, 0, 0, 1)] * 2)
    c = bh.Gt.from_bytes(ctx, a.read(0, 2), checked=True)
    assert len((a + b) * [3, 4]) == 2 and len(-c) == 2 and len(c.sum()) == 576
    assert len(bh.multiexp_gt(ctx, c, [5, 6])) == 576
    a.close()
    rep = ctx.scratch_report()
    assert rep["fits"]
    assert not rep["worst_kernel"].startswith("k_gt")
    assert rep["worst_bytes_per_lane"] >= 1680
