"""A pure-Python model of the device multi-Miller loop's grouping (csrc/pairing_dev.hip) over the
oracle's field, against oracle/pairing.py's multi_miller_loop: no library, no GPU.

The model keeps what the kernels do to the ORDER of the arithmetic and nothing else:
  * a lane owns K consecutive pairs and one Fp12 value, squared once per bit;
  * the K denominators of a step (2 y_T in a doubling, x_Q - x_T in an addition step) are inverted
    together: prefix products, one inversion, a backward pass -- so the pairs' lines reach f in
    reverse order; a pair with an identity takes part with denominator one and no line; a zero
    denominator is replaced by one and raises the flag;
  * the lanes' values are multiplied by levels, thread t of a level taking v[t], v[t + out],
    v[t + 2 out], ... with out = ceil(m / 8), until at most 64 remain, which are multiplied in order.
Field arithmetic is exact and Fp12 commutative, so the result must equal multi_miller_loop's
coefficient for coefficient; this pins the index algebra where it can be debugged without a device.
"""
import random

import pytest

from oracle import bls12_381 as bls
from oracle import pairing as pr

F2 = bls.Fp2Ops
ONE2 = (1, 0)


class Degenerate(Exception):
    pass


def _line_mul(f, l0, l2, yp):
    """f * (l0 + l2 w^2 + yp w^3), per output coefficient as f12_mul_line does"""
    out = []
    for k in range(6):
        u, w = (0, 0), (0, 0)
        for shift, l in ((0, l0), (2, l2), (3, (yp, 0))):
            j = k - shift
            prod = F2.mul(f[j % 6], l)
            if j < 0:
                w = F2.add(w, prod)
            else:
                u = F2.add(u, prod)
        out.append(F2.add(u, F2.mul(pr.XI, w)))
    return out


def _dense_mul(a, b):
    out = []
    for k in range(6):
        u, w = (0, 0), (0, 0)
        for i in range(6):
            prod = F2.mul(a[i], b[(k - i) % 6])
            if i > k:
                w = F2.add(w, prod)
            else:
                u = F2.add(u, prod)
        out.append(F2.add(u, F2.mul(pr.XI, w)))
    return out


def lane_value(pairs, flag):
    """one lane: its pairs' (P, Q) with None for an identity"""
    active = [p is not None and q is not None for p, q in pairs]
    ts = [q if a else None for (p, q), a in zip(pairs, active)]
    f = pr.f12_one()
    for bit in bin(pr.X_ABS)[3:]:
        f = _dense_mul(f, f)
        for is_add in ([False, True] if bit == "1" else [False]):
            def denom(k):
                if not active[k]:
                    return ONE2
                xt, yt = ts[k]
                d = F2.sub(pairs[k][1][0], xt) if is_add else F2.add(yt, yt)
                if d == (0, 0):
                    flag.append(k)
                    return ONE2
                return d
            prefix, acc = [], ONE2
            for k in range(len(pairs)):
                prefix.append(acc)
                acc = F2.mul(acc, denom(k))
            inv = F2.inv(acc)
            for k in reversed(range(len(pairs))):
                d = denom(k)
                dinv = F2.mul(inv, prefix[k])
                inv = F2.mul(inv, d)
                if not active[k]:
                    continue
                (xp, yp), (xq, yq) = pairs[k]
                xt, yt = ts[k]
                if is_add:
                    num, xsum = F2.sub(yq, yt), F2.add(xt, xq)
                else:
                    x2 = F2.sqr(xt)
                    num, xsum = F2.add(F2.add(x2, x2), x2), F2.add(xt, xt)
                lam = F2.mul(num, dinv)
                l0 = F2.sub(F2.mul(lam, xt), yt)
                l2 = F2.neg(F2.mul(lam, (xp, 0)))
                f = _line_mul(f, l0, l2, yp)
                x3 = F2.sub(F2.sqr(lam), xsum)
                ts[k] = (x3, F2.sub(F2.mul(lam, F2.sub(xt, x3)), yt))
    return f


def product_tree(v):
    v = list(v)
    m = len(v)
    while m > 64:
        out = (m + 7) // 8
        for t in range(out):
            acc = v[t]
            for i in range(t + out, m, out):
                acc = _dense_mul(acc, v[i])
            v[t] = acc
        m = out
    r = pr.f12_one()
    for x in v[:m]:
        r = pr.f12_mul(r, x)
    return r


def model(pairs, K):
    flag = []
    lanes = [lane_value(pairs[i:i + K], flag) for i in range(0, len(pairs), K)]
    if flag:
        raise Degenerate(flag)
    return product_tree(lanes)


# ------------------------------------------------------------------ data
@pytest.fixture(scope="module")
def pool():
    """distinct random multiples of the generators, made by repeated addition (cheap)"""
    rng = random.Random(20250301)
    g1, g2 = bls.G1, bls.G2
    a = g1.mul(g1.generator(), rng.getrandbits(64))
    b = g2.mul(g2.generator(), rng.getrandbits(64))
    sa, sb = g1.mul(g1.generator(), rng.getrandbits(64)), g2.mul(g2.generator(), rng.getrandbits(64))
    out = []
    for _ in range(40):
        out.append((g1.to_affine(a), g2.to_affine(b)))
        a, b = g1.add(a, sa), g2.add(b, sb)
    return out


def test_products_match_f12_mul(pool):
    rng = random.Random(1)
    a = [(rng.randrange(bls.P), rng.randrange(bls.P)) for _ in range(6)]
    b = [(rng.randrange(bls.P), rng.randrange(bls.P)) for _ in range(6)]
    assert _dense_mul(a, b) == pr.f12_mul(a, b)
    l0, l2, yp = b[0], b[2], b[3][0]
    assert _line_mul(a, l0, l2, yp) == pr.f12_mul(a, [l0, (0, 0), l2, (yp, 0), (0, 0), (0, 0)])


@pytest.mark.parametrize("K,n", [(1, 0), (1, 1), (1, 2), (3, 2), (3, 3), (3, 4), (3, 7), (16, 15), (16, 16),
                                 (16, 17), (5, 23)])
def test_model_equals_multi_miller_loop(pool, K, n):
    pairs = pool[:n]
    assert model(pairs, K) == pr.multi_miller_loop(pairs)


def test_identities_in_a_batch(pool):
    K = 4
    for ids in ({0: "p"}, {3: "q"}, {0: "q", 3: "p"}, {k: "p" for k in range(8)}):
        pairs = [(None, q) if ids.get(i) == "p" else (p, None) if ids.get(i) == "q" else (p, q)
                 for i, (p, q) in enumerate(pool[:8])]
        assert model(pairs, K) == pr.multi_miller_loop(pairs)
    assert model([(None, None)] * 5, K) == pr.f12_one()


def test_repeated_pair_and_negation(pool):
    p, q = pool[0]
    assert model([(p, q)] * 16, 16) == pr.multi_miller_loop([(p, q)] * 16)
    pairs = [(p, q), ((p[0], (-p[1]) % bls.P), q)]
    f = model(pairs, 2)
    assert f == pr.multi_miller_loop(pairs)
    assert f != pr.f12_one() and pr.f12_is_one(pr.final_exponentiation(f))


def test_product_tree_levels():
    rng = random.Random(5)
    small = [[(rng.randrange(bls.P), rng.randrange(bls.P)) for _ in range(6)] for _ in range(9)]
    for m in (1, 7, 8, 9, 64, 65, 73, 513):  # a short group, a full one, one over, two and three levels
        v = [small[i % 9] for i in range(m)]
        want = pr.f12_one()
        for x in v:
            want = pr.f12_mul(want, x)
        assert product_tree(v) == want, m


def test_zero_denominator_is_flagged(pool):
    """y_T = 0 makes the first doubling divide by zero: the model raises instead of returning a value,
    whatever the other pairs of the batch and the other lanes hold"""
    p, q = pool[0]
    bad = ((5, 7), (0, 0))
    for K, slot in ((1, 0), (4, 0), (4, 3)):
        pairs = list(pool[:2 * K])
        pairs[slot] = (p, bad)
        with pytest.raises(Degenerate):
            model(pairs, K)
