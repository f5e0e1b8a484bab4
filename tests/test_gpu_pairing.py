"""The device multi-Miller loop (csrc/pairing_dev.hip; bh_miller_product, bh_final_exponentiation and
bh_selftest_miller_product, which forces K pairs per lane) against oracle/pairing.py's
multi_miller_loop on the same pairs, all twelve Fp coefficients.  Field arithmetic is exact, so
every comparison is an equality.

Sizes follow the oracle's cost (about 15 ms per pair's Miller loop, 0.7 s per final
exponentiation): at most about 200 pairs per case.  The shapes sit on a lane's batch edge (K - 1, K,
K + 1), the wave edge (64 K +- 1 pairs: 64 lanes, then a 65th holding one pair) and a short last
lane; the product tree on a short group, a full group, one over and a second level (7, 8, 9, 65
lanes)."""
import ctypes
import random

import numpy as np
import pytest

from oracle import bls12_381 as bls
from oracle import pairing as pr

pytestmark = pytest.mark.gpu

P, R = bls.P, bls.R
G1, G2 = bls.G1, bls.G2
ONE = pr.f12_one()
OK, INVALID_ARGUMENT, DEGENERATE = 0, 10, 16
DEV_R = pow(2, 406, P)  # the device's Montgomery radix: it holds x * 2^406 mod p


def _bh():
    import bellman_hip as bh
    return bh


# ------------------------------------------------------------------ shared oracle data (computed once)
class _Pool:
    """200 pairs (a_i G1, b_i G2), a_i = a_0 + i s and b_i = b_0 + i t for random 64-bit a_0, s, b_0, t
    (random multiples of the generators, made by repeated addition), and their scalars."""

    def __init__(self):
        rng = random.Random(20250302)
        self.a0, self.s, self.b0, self.t = (rng.getrandbits(64) | 1 for _ in range(4))
        a, b = G1.mul(G1.generator(), self.a0), G2.mul(G2.generator(), self.b0)
        sa, sb = G1.mul(G1.generator(), self.s), G2.mul(G2.generator(), self.t)
        self.pairs = []
        for _ in range(200):
            self.pairs.append((G1.to_affine(a), G2.to_affine(b)))
            a, b = G1.add(a, sa), G2.add(b, sb)
        self._want = {}

    def a(self, i):
        return (self.a0 + i * self.s) % R

    def b(self, i):
        return (self.b0 + i * self.t) % R

    def want(self, n):
        """multi_miller_loop of the first n pairs (kept: several cases share a length)"""
        if n not in self._want:
            self._want[n] = pr.multi_miller_loop(self.pairs[:n])
        return self._want[n]


@pytest.fixture(scope="module")
def pool():
    return _Pool()


def _upload(ctx, pairs):
    bh = _bh()
    g1 = bh.Bases(ctx, bh.BH_G1, b"".join(bls.g1_to_uncompressed(p) for p, _ in pairs), checked=False)
    g2 = bh.Bases(ctx, bh.BH_G2, b"".join(bls.g2_to_uncompressed(q) for _, q in pairs), checked=False)
    return g1, g2


def _selftest(ctx, g1, g2, n, K, off1=0, off2=0):
    """bh_selftest_miller_product -> (status, value or None)"""
    bh = _bh()
    f = bh.lib().bh_selftest_miller_product
    f.restype = ctypes.c_int
    f.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t,
                  ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
    out = np.full(576, 0xAA, dtype=np.uint8)
    st = f(ctx.h, g1.h, off1, g2.h, off2, n, K, out.ctypes.data_as(ctypes.c_void_p))
    return st, (bh._f12_from_bytes(out.tobytes()) if st == OK else None)


def _forced(ctx, pairs, K):
    g1, g2 = _upload(ctx, pairs)
    st, f = _selftest(ctx, g1, g2, len(pairs), K)
    assert st == OK, st
    return f


# ------------------------------------------------------------------ 1. batch, wave and lane edges
SHAPES = sorted({(K, n) for K in (1, 3) for n in (0, 1, K - 1, K, K + 1, 64 * K - 1, 64 * K + 1)} |
                {(16, n) for n in (1, 15, 16, 17, 130)})


@pytest.mark.parametrize("K,n", SHAPES)
def test_forced_k_equals_the_oracle(ctx, pool, K, n):
    assert _forced(ctx, pool.pairs[:n], K) == pool.want(n)


@pytest.mark.parametrize("lanes", [7, 8, 9, 65])
def test_product_tree(ctx, pool, lanes):
    """K = 1: one value per pair, so the tree sees `lanes` values"""
    assert _forced(ctx, pool.pairs[:lanes], 1) == pool.want(lanes)


# ------------------------------------------------------------------ 2. identities (the all-zero record)
@pytest.mark.parametrize("which", ["first_g1", "last_g2", "both_ends", "g1_side", "g2_side", "every"])
def test_identities(ctx, pool, which):
    K, n = 4, 9  # two full lanes and a lane of one pair
    ids = {"first_g1": {4: "p"}, "last_g2": {7: "q"}, "both_ends": {0: "q", 3: "p", 8: "p"},
           "g1_side": {i: "p" for i in range(0, n, 2)}, "g2_side": {i: "q" for i in range(1, n, 2)},
           "every": {i: "pq"[i & 1] for i in range(n)}}[which]
    pairs = [(None, q) if ids.get(i) == "p" else (p, None) if ids.get(i) == "q" else (p, q)
             for i, (p, q) in enumerate(pool.pairs[:n])]
    want = pr.multi_miller_loop(pairs)
    assert (want == ONE) == (which == "every")
    assert _forced(ctx, pairs, K) == want


# ------------------------------------------------------------------ 3. other inputs
def test_the_same_pair_16_times_in_one_lane(ctx, pool):
    pairs = [pool.pairs[5]] * 16
    assert _forced(ctx, pairs, 16) == pr.multi_miller_loop(pairs)


def test_negated_neighbour(ctx, pool):
    """(P, Q) next to (-P, Q): the Miller values differ, their product is one after the final
    exponentiation (bh_final_exponentiation, checked against the oracle's)"""
    bh = _bh()
    p, q = pool.pairs[9]
    pairs = [(p, q), ((p[0], (P - p[1]) % P), q)]
    f = _forced(ctx, pairs, 2)
    assert f == pr.multi_miller_loop(pairs) and f != ONE
    assert bh.final_exponentiation(f) == ONE
    single = _forced(ctx, pairs[:1], 1)
    assert bh.final_exponentiation(single) == pr.final_exponentiation(single) != ONE


def test_g1_coordinates_near_p(ctx, pool):
    """x_P and y_P whose device values (x * 2^406 mod p) have their top limb at p's: found by walking
    multiples of the generator"""
    rng = random.Random(11)
    a = G1.mul(G1.generator(), rng.getrandbits(64))
    found = []
    for _ in range(20000):
        x, y = G1.to_affine(a)
        if x * DEV_R % P >= P - P // 16 and y * DEV_R % P >= P - P // 16:
            found.append((x, y))
            if len(found) == 2:
                break
        a = G1.add(a, G1.generator())
    assert len(found) == 2
    pairs = [(found[0], pool.pairs[0][1]), (found[1], pool.pairs[1][1]), pool.pairs[2]]
    assert _forced(ctx, pairs, 2) == pr.multi_miller_loop(pairs)


# ------------------------------------------------------------------ 4. bh_miller_product
def test_offsets_into_longer_vectors(ctx, pool):
    bh = _bh()
    g1, _ = _upload(ctx, pool.pairs[:40])
    _, g2 = _upload(ctx, pool.pairs[10:60])
    # g1[3 + i] with g2[5 + i] = pool's Q[15 + i]
    pairs = [(pool.pairs[3 + i][0], pool.pairs[15 + i][1]) for i in range(20)]
    assert bh.multi_miller_loop(ctx, g1, g2, off1=3, off2=5, n=20) == pr.multi_miller_loop(pairs)
    assert bh.multi_miller_loop(ctx, g1, g2, off1=40, off2=50, n=0) == ONE


def test_arguments(ctx, pool):
    bh = _bh()
    g1, g2 = _upload(ctx, pool.pairs[:4])
    out = np.zeros(576, dtype=np.uint8)
    p = out.ctypes.data_as(ctypes.c_void_p)
    f = bh.lib().bh_miller_product
    assert f(ctx.h, g2.h, 0, g2.h, 0, 4, p) == INVALID_ARGUMENT  # group mismatch
    assert f(ctx.h, g1.h, 0, g1.h, 0, 4, p) == INVALID_ARGUMENT
    assert f(ctx.h, g1.h, 1, g2.h, 0, 4, p) == INVALID_ARGUMENT  # past the end
    assert f(ctx.h, g1.h, 0, g2.h, 5, 0, p) == INVALID_ARGUMENT  # offset out of range
    assert f(ctx.h, g1.h, 0, g2.h, 0, 4, None) == INVALID_ARGUMENT
    assert _selftest(ctx, g1, g2, 4, 0)[0] == INVALID_ARGUMENT
    assert _selftest(ctx, g1, g2, 4, 17)[0] == INVALID_ARGUMENT
    bad = np.frombuffer(P.to_bytes(48, "big") + bytes(528), dtype=np.uint8)  # a coefficient = p
    assert bh.lib().bh_final_exponentiation(bad.ctypes.data_as(ctypes.c_void_p), p) == 11
    assert bh._status_string(DEGENERATE).startswith("the Miller loop met a zero denominator")


def _closed_set(pool, n):
    """n pairs whose pairing product is one: pool-style pairs (a_i G1, b_i G2) for i < n - 1 and the
    closing pair (G1, -(sum a_i b_i) G2), so that sum a_i b_i = 0 mod r over all n"""
    a, b = G1.mul(G1.generator(), pool.a0), G2.mul(G2.generator(), pool.b0)
    sa, sb = G1.mul(G1.generator(), pool.s), G2.mul(G2.generator(), pool.t)
    pairs, acc = [], 0
    for i in range(n - 1):
        pairs.append((G1.to_affine(a), G2.to_affine(b)))
        acc += pool.a(i) * pool.b(i)
        a, b = G1.add(a, sa), G2.add(b, sb)
    pairs.append((bls.G1_GEN, G2.to_affine(G2.mul(G2.generator(), (-acc) % R))))
    return pairs


def test_a_thousand_pairs_that_multiply_to_one(ctx, pool):
    """n = 1000 through bh_miller_product (the library's own K).  The oracle's Miller loops of 1000
    pairs would take 15 s, so the reference is the set's construction (sum a_i b_i = 0 mod r, which
    the oracle's pairing_product_is_one confirms on the same construction at n = 12) and the
    oracle's final exponentiation of the device's value; one perturbed scalar must not give one."""
    bh = _bh()
    assert pr.pairing_product_is_one(_closed_set(pool, 12))
    pairs = _closed_set(pool, 1000)
    g1, g2 = _upload(ctx, pairs)
    f = bh.multi_miller_loop(ctx, g1, g2)
    assert f != ONE
    assert bh.final_exponentiation(f) == ONE
    assert pr.final_exponentiation(f) == ONE
    assert bh.pairing_product_is_one(ctx, g1, g2)
    pairs[500] = (G1.to_affine(G1.add(G1.from_affine(pairs[500][0]), G1.generator())), pairs[500][1])
    g1, g2 = _upload(ctx, pairs)
    assert not bh.pairing_product_is_one(ctx, g1, g2)


def test_bilinearity_through_the_public_names(ctx):
    """e(aP, bQ) e(-abP, Q) = 1"""
    bh = _bh()
    a, b = 0x1234567890ABCDEF1122334455667788, 0xFEDCBA0987654321AABBCCDDEEFF0011
    g1 = [G1.to_affine(G1.mul(G1.generator(), a)), G1.to_affine(G1.mul(G1.generator(), (-a * b) % R))]
    g2 = [G2.to_affine(G2.mul(G2.generator(), b)), bls.G2_GEN]
    v1, v2 = _upload(ctx, list(zip(g1, g2)))
    assert bh.pairing_product_is_one(ctx, v1, v2)
    w1, w2 = _upload(ctx, [(g1[0], g2[0]), (g1[1], g2[0])])
    assert not bh.pairing_product_is_one(ctx, w1, w2)


# ------------------------------------------------------------------ 5. a zero denominator
@pytest.fixture(scope="module")
def order13():
    """A twist point of order 13: a cofactor multiple of a random twist point.  The twist
    y^2 = x^3 + 4(1 + u) has r h2 points, h2 = (x^8 - 4x^7 + 5x^6 - 4x^4 + 6x^3 - 4x^2 - 4x + 13) / 9
    for the curve's seed x; 13^2 divides h2 and the 13-part of the group has exponent 13 (r h2 / 13
    sends every point to the identity), so r h2 / 169 sends a random point into it."""
    x = -pr.X_ABS
    h2, rem = divmod(x ** 8 - 4 * x ** 7 + 5 * x ** 6 - 4 * x ** 4 + 6 * x ** 3 - 4 * x ** 2 - 4 * x + 13, 9)
    assert rem == 0 and h2 % 169 == 0 and h2 % 2197 != 0
    rng = random.Random(13)
    while True:
        xs = (rng.randrange(P), rng.randrange(P))
        ys = pr._fp2_sqrt(bls.Fp2Ops.add(bls.Fp2Ops.mul(bls.Fp2Ops.sqr(xs), xs), (4, 4)))
        if ys is None:
            continue
        q = G2.to_affine(G2.mul(G2.from_affine((xs, ys)), R * h2 // 169))
        if q is not None:
            break
    assert G2.on_curve_affine(q) and G2.to_affine(G2.mul(G2.from_affine(q), 13)) is None
    # the loop's T runs Q, 2Q, 3Q, 6Q, 12Q = -Q and then adds Q: x_Q - x_T = 0 at the second addition
    assert bin(pr.X_ABS)[3:6] == "101"
    assert G2.to_affine(G2.mul(G2.from_affine(q), 12)) == (q[0], bls.Fp2Ops.neg(q[1]))
    return q


@pytest.mark.parametrize("K,slot", [(1, 0), (1, 2), (16, 0), (16, 15), (16, 16 + 15)])
def test_degenerate_point_is_reported(ctx, pool, order13, K, slot):
    """wherever the point sits in a batch, and whatever the other lanes hold"""
    n = 3 * K
    pairs = list(pool.pairs[:n])
    pairs[slot] = (pairs[slot][0], order13)
    g1, g2 = _upload(ctx, pairs)
    assert _selftest(ctx, g1, g2, n, K) == (DEGENERATE, None)
    bh = _bh()
    with pytest.raises(bh.PairingDegenerate):
        bh.multi_miller_loop(ctx, g1, g2)
    # beside an identity G1 point it takes no part: no step, no flag
    pairs[slot] = (None, order13)
    g1, g2 = _upload(ctx, pairs)
    assert _selftest(ctx, g1, g2, n, K) == (OK, pr.multi_miller_loop(pairs))


# ------------------------------------------------------------------ 6. scratch budget
def test_scratch_budget_keeps_its_worst_kernel(ctx, pool):
    """the pairing kernels are in the list and none of them is its worst (k_miller_steps keeps 40 B
    per lane in its private segment; the worst kernel before them, k_rowcol_final<G2>, 1 680 B)"""
    _forced(ctx, pool.pairs[:2], 1)
    rep = ctx.scratch_report()
    assert rep["fits"]
    assert not rep["worst_kernel"].startswith(("k_miller", "k_f12"))
    assert rep["worst_bytes_per_lane"] >= 1680
    assert rep["kernels_checked"] >= 10
