"""The field predicates, subtractions and conversions of csrc/field.cuh against Python integers.

bh_selftest_field_misc (csrc/selftest.hip) evaluates fe_is_zero, fe_reduce_full, fe_csub<1>,
FpOps::neg_canonical, fe_sub<K> for the K of curve.cuh (1, 2, 4, 8, 16, 128), fe_add and
fe_unpack(fe_pack(x)) on caller-chosen raw limbs, for Fp and, where the library instantiates them
for Fr (is_zero, csub<1>, csub<2>, sub<2>, add, pack / unpack), for Fr.  The group law's exceptional
cases hang on fe_is_zero deciding x = k p for every k below 128 and nothing else; a transform's
output on fe_csub and fe_pack.  Everything is exact: no tolerance.
"""
import ctypes
import itertools
import random

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

P = 0x1A0111EA397FE69A4B1BA7B6434BACD764774B84F38512BF6730D2A0F6B0F6241EABFFFEB153FFFFB9FEFFFFFFFFAAAB
R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
BITS, MASK = 29, (1 << 29) - 1
NP, NR, WP, WR = 14, 9, 12, 8
SUB_K = (1, 2, 4, 8, 16, 128)
FP_OUT = 1 + 10 * NP + WP + NP
FR_OUT = 1 + 4 * NR + WR + NR
FR_TOP = 1 << (BITS * NR)       # 9 limbs hold 261 bits: fe_is_zero<Fr> sees k r only below 2^261 (k <= 70)


def _limbs(x, n):
    assert 0 <= x < 1 << (BITS * (n - 1) + 32)
    return [(x >> (BITS * i)) & MASK for i in range(n - 1)] + [x >> (BITS * (n - 1))]


def _value(ls):
    return sum(int(v) << (BITS * i) for i, v in enumerate(ls))


def _words(x, w):
    return [(x >> (32 * i)) & 0xFFFFFFFF for i in range(w)]


def _fp_cases():
    """(a, b, checks): checks names the outputs whose preconditions (a, b) meets"""
    rng = random.Random(128)
    cs = []
    for k in range(128):
        kp = k * P
        cs.append((kp, 0, {"zero": True, "reduce": 0, "csub1": 1}))
        cs.append((kp + 1, 0, {"zero": False, "reduce": 1, "csub1": 1}))
        cs.append((kp + P - 1, 0, {"zero": False, "reduce": P - 1, "csub1": 1}))
        r = rng.randrange(2, P - 1)
        cs.append((kp + r, 0, {"zero": False, "reduce": r, "csub1": 1}))
        if k:
            cs.append((kp - 1, 0, {"zero": False}))
        # the low limb still says k: only the full comparison can tell
        for j in (1, 2, rng.randrange(3, 1 << 29), 1 << (BITS * rng.randrange(1, 12))):
            cs.append((kp + (j << BITS), 0, {"zero": False}))
        # k p's low limb under the higher limbs of another multiple of p
        other = (rng.randrange(128) * P) >> BITS << BITS
        if (other | (kp & MASK)) != kp:
            cs.append((other | (kp & MASK), 0, {"zero": False}))
    for _ in range(512):
        v = rng.randrange(1, 128 * P)
        cs.append((v, 0, {"zero": v % P == 0, "reduce": v % P, "csub1": 1}))
    for a in (0, 1, P - 1, P):
        cs.append((a, 0, {"negc": (P - a) % P, "csub1": 1}))
    for _ in range(64):
        a = rng.randrange(P)
        cs.append((a, 0, {"negc": (P - a) % P}))
    # fe_sub<K>: b at K p - 1 and at 0, a at 0 and at the bounds its callers hold (products < 2p, X < 10p,
    # U2 - X1 < 18p); one case serves every K whose precondition b < K p it meets
    for K in SUB_K:
        for a, b in itertools.product((0, 1, 2 * P - 1, 10 * P - 1, 18 * P - 1, rng.randrange(18 * P)),
                                      (K * P - 1, K * P - 2, 0, 1, rng.randrange(K * P))):
            cs.append((a, b, {"sub": [k for k in SUB_K if b < k * P], "add": 1}))
    for _ in range(256):
        a, b = rng.randrange(128 * P), rng.randrange(128 * P)
        cs.append((a, b, {"sub": [k for k in SUB_K if b < k * P], "add": 1, "csub1": 1}))
    for v in [0, 1, P - 1, (1 << 384) - 1] + [1 << i for i in range(384)] + [rng.randrange(1 << 384) for _ in range(256)]:
        cs.append((v, 0, {"pack": 1}))
    return cs


def _fr_cases():
    rng = random.Random(70)
    cs = []
    for k in range(FR_TOP // R + 1):
        kr = k * R
        cs.append((kr, 0, {"zero": True, "csub1": 1, "csub2": 1}))
        cs.append((kr + 1, 0, {"zero": False, "csub1": 1, "csub2": 1}))
        if k:
            cs.append((kr - 1, 0, {"zero": False, "csub1": 1, "csub2": 1}))
        for j in (1, 2, rng.randrange(3, 1 << 20)):
            if kr + (j << BITS) < FR_TOP:
                cs.append((kr + (j << BITS), 0, {"zero": False}))
    for _ in range(512):
        v = rng.randrange(1, FR_TOP)
        cs.append((v, 0, {"zero": v % R == 0, "csub1": 1, "csub2": 1}))
    for a, b in itertools.product((0, 1, 2 * R - 1, 4 * R - 1, rng.randrange(4 * R)),
                                  (2 * R - 1, 2 * R - 2, 0, 1, rng.randrange(2 * R))):
        cs.append((a, b, {"sub2": 1, "add": 1}))
    for _ in range(256):
        cs.append((rng.randrange(8 * R), rng.randrange(2 * R), {"sub2": 1, "add": 1}))
    for v in [0, 1, R - 1, (1 << 256) - 1] + [1 << i for i in range(256)] + [rng.randrange(1 << 256) for _ in range(256)]:
        cs.append((v, 0, {"pack": 1}))
    # k r for the k whose multiple does not fit the nine limbs, less the 2^261 a comparison that drops
    # the top carry loses: all 57 are = -2^261 mod r, the device Montgomery form of -1, not zero
    for k in range(FR_TOP // R + 1, 128):
        x = k * R - FR_TOP
        assert 0 < x < FR_TOP and x % R == -FR_TOP % R
        cs.append((x, 0, {"zero": False, "csub1": 1, "csub2": 1}))
        for y in (x + 1, x - 1, x + (1 << BITS)):
            cs.append((y, 0, {"zero": False}))
    return cs


def _run(fp, fr):
    import bellman_hip as bh
    f = bh.lib().bh_selftest_field_misc
    f.restype = ctypes.c_int
    f.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    n = max(len(fp), len(fr))
    pad = lambda cs: cs + [(0, 0, {})] * (n - len(cs))
    inp = np.array([_limbs(a, NP) + _limbs(b, NP) + _limbs(x, NR) + _limbs(y, NR)
                    for (a, b, _), (x, y, _) in zip(pad(fp), pad(fr))], dtype=np.uint64).astype(np.uint32)
    out = np.zeros((n, FP_OUT + FR_OUT), dtype=np.uint32)
    assert f(0, inp.ctypes.data, n, out.ctypes.data) == 0
    return out


@pytest.fixture(scope="module")
def device_out():
    fp, fr = _fp_cases(), _fr_cases()
    return fp, fr, _run(fp, fr)


def _normalised(ls):
    return all(int(v) <= MASK for v in ls[:-1])


def test_fp_predicates_subtractions_and_packing(device_out):
    fp, _, out = device_out
    seen = {}
    for (a, b, chk), res in zip(fp, out):
        blk = lambda i: res[1 + i * NP:1 + (i + 1) * NP]
        for name in chk:
            seen[name] = seen.get(name, 0) + 1
        if "zero" in chk:
            assert bool(res[0]) == chk["zero"], hex(a)
        if "reduce" in chk:
            assert _value(blk(0)) == chk["reduce"], hex(a)
        if "csub1" in chk:
            assert _value(blk(1)) == (a - P if a >= P else a) and _normalised(blk(1)), hex(a)
        if "negc" in chk:
            assert _value(blk(2)) == chk["negc"], hex(a)
        for k in chk.get("sub", ()):
            got = blk(3 + SUB_K.index(k))
            assert _value(got) == a + k * P - b and _normalised(got), (k, hex(a), hex(b))
        if "add" in chk:
            assert _value(blk(9)) == a + b and _normalised(blk(9)), (hex(a), hex(b))
        if "pack" in chk:
            words = res[1 + 10 * NP:1 + 10 * NP + WP]
            assert [int(w) for w in words] == _words(a, WP), hex(a)
            back = res[1 + 10 * NP + WP:FP_OUT]
            assert _value(back) == a and all(int(v) <= MASK for v in back), hex(a)
    assert seen["zero"] > 128 * 8 and seen["reduce"] >= 128 * 4 and seen["pack"] > 384


def test_fr_predicates_subtractions_and_packing(device_out):
    _, fr, out = device_out
    for (x, y, chk), res in zip(fr, out[:, FP_OUT:]):
        blk = lambda i: res[1 + i * NR:1 + (i + 1) * NR]
        if "zero" in chk:
            assert bool(res[0]) == chk["zero"], hex(x)
        if "csub1" in chk:
            assert _value(blk(0)) == (x - R if x >= R else x) and _normalised(blk(0)), hex(x)
        if "csub2" in chk:
            assert _value(blk(1)) == (x - 2 * R if x >= 2 * R else x) and _normalised(blk(1)), hex(x)
        if "sub2" in chk:
            assert _value(blk(2)) == x + 2 * R - y and _normalised(blk(2)), (hex(x), hex(y))
        if "add" in chk:
            assert _value(blk(3)) == x + y and _normalised(blk(3)), (hex(x), hex(y))
        if "pack" in chk:
            words = res[1 + 4 * NR:1 + 4 * NR + WR]
            assert [int(w) for w in words] == _words(x, WR), hex(x)
            back = res[1 + 4 * NR + WR:FR_OUT]
            assert _value(back) == x and all(int(v) <= MASK for v in back), hex(x)
