"""Gt values for the tests of the target group (csrc/gt.hip): the generators' pairing in the crate's
convention, E = conj(pairing(G1, G2))^3 with oracle/pairing.py's pairing; gt_format and its inverse;
the model of the cyclotomic-squaring formula; the chosen scalars; and a cache of E^k per distinct
k (a power costs about 55 ms, a pairing 0.7 s: every expected value comes from powers of E, never
from a pairing per element).  Shared by tests/test_gt_model_cpu.py and tests/test_gpu_gt.py.  Not a
test module."""
import functools
import json
import os
import random

from oracle import bls12_381 as bls
from oracle import pairing as pr

P, R = bls.P, bls.R
F2 = pr.F2
XI = (1, 1)
ONE = pr.f12_one()
ZERO = [(0, 0)] * 6
X_ABS = 0xD201000000010000
ORDER = (5, 3, 1, 4, 2, 0)  # gt_format: the coefficients of w^5, w^3, w^1, w^4, w^2, w^0, each c1 then c0
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gt_generator.json")


def conj(f):
    return [c if k % 2 == 0 else F2.neg(c) for k, c in enumerate(f)]


def gt_format(f):
    return b"".join(int(f[k][1]).to_bytes(48, "big") + int(f[k][0]).to_bytes(48, "big") for k in ORDER)


def gt_parse(b):
    assert len(b) == 576
    f = [None] * 6
    for q, k in enumerate(ORDER):
        f[k] = (int.from_bytes(b[96 * q + 48:96 * q + 96], "big"), int.from_bytes(b[96 * q:96 * q + 48], "big"))
    return f


def flat_bytes(f):
    """the encoding of bh_miller_product: c[0].c0, c[0].c1, ..., c[5].c1"""
    return b"".join(int(x).to_bytes(48, "big") for c in f for x in c)


def flat_parse(b):
    c = [int.from_bytes(b[48 * k:48 * k + 48], "big") for k in range(12)]
    return [(c[2 * i], c[2 * i + 1]) for i in range(6)]


def fixture_bytes():
    with open(GOLDEN) as f:
        return bytes.fromhex(json.load(f)["gt"])


@functools.lru_cache(maxsize=None)
def library_pairing():
    """e0(G1 generator, G2 generator), the library's and the oracle's own convention"""
    return pr.pairing(bls.G1.to_affine(bls.G1.generator()), bls.G2.to_affine(bls.G2.generator()))


@functools.lru_cache(maxsize=None)
def generator_pairing():
    """E, the crate's pairing(G1 generator, G2 generator)"""
    c = conj(library_pairing())
    return pr.f12_mul(pr.f12_sqr(c), c)


@functools.lru_cache(maxsize=None)
def power(k):
    """E^(k mod r), kept per distinct exponent"""
    k %= R
    if k == 0:
        return ONE
    if k == 1:
        return generator_pairing()
    if k > R // 2:
        return conj(power(R - k))
    return pr.f12_pow(generator_pairing(), k)


# ---------------------------------------------------------------- the squaring model
def _f4_sqr(x, y):
    """(x + y s)^2 in Fp4 = Fp2[s]/(s^2 - xi) by three Fp2 squarings"""
    x2, y2 = F2.sqr(x), F2.sqr(y)
    return F2.add(x2, F2.mul(XI, y2)), F2.sub(F2.sub(F2.sqr(F2.add(x, y)), x2), y2)


def cyclotomic_square_model(f):
    """The formula k_gt_cyc_sqr evaluates, a polynomial map on all of Fp12: with A = c0 + c3 s,
    B = c1 + c4 s, C = c2 + c5 s, (3 A^2 - 2 conj A) + (3 s C^2 + 2 conj B) w + (3 B^2 - 2 conj C) w^2.
    Equal to f^2 exactly on the cyclotomic subgroup."""
    c0, c1, c2, c3, c4, c5 = f
    a2, b2, cc2 = _f4_sqr(c0, c3), _f4_sqr(c1, c4), _f4_sqr(c2, c5)
    tr = lambda v: F2.add(F2.add(v, v), v)  # noqa: E731
    dbl = lambda v: F2.add(v, v)  # noqa: E731
    sc = (F2.mul(XI, cc2[1]), cc2[0])  # s (x + y s) = xi y + x s
    return [F2.sub(tr(a2[0]), dbl(c0)), F2.add(tr(sc[0]), dbl(c1)), F2.sub(tr(b2[0]), dbl(c2)),
            F2.add(tr(a2[1]), dbl(c3)), F2.sub(tr(sc[1]), dbl(c4)), F2.add(tr(b2[1]), dbl(c5))]


def random_f12(seed):
    rng = random.Random(seed)
    return [(rng.randrange(P), rng.randrange(P)) for _ in range(6)]


@functools.lru_cache(maxsize=None)
def easy_part_image(seed):
    """f^((p^6 - 1)(p^2 + 1)) of a seeded random value: in the cyclotomic subgroup, not in Gt"""
    return pr.f12_pow(random_f12(seed), (P ** 6 - 1) * (P ** 2 + 1))


def non_member():
    """the chosen cyclotomic non-member: m conj(m) = 1 and m^r != 1"""
    return easy_part_image(20251021)


# ---------------------------------------------------------------- scalars
def chosen_scalars():
    """0, small ones around the window's digit edges (7, 8, 9, 15, 16), r - 1, the recoding's bias
    0x88..8 reduced below r and 0x77..7 (all digits at an extreme), 2^254, |x| and seeded random ones"""
    rng = random.Random(41)
    bias = int("8" * 64, 16)
    return [0, 1, 2, 7, 8, 9, 15, 16, R - 1, bias % R, int("7" * 64, 16) % R, 1 << 254, X_ABS] + \
        [rng.randrange(R) for _ in range(3)]


def tiled(n, shift=0):
    """n scalars tiled from the chosen ones, the list rotated by shift"""
    s = chosen_scalars()
    return [s[(i + shift) % len(s)] for i in range(n)]


def lanes_of(n):
    return sorted({l for l in (0, 63, 64, n - 1) if 0 <= l < n})
