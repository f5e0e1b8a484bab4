"""The NTT's butterflies, reductions and store paths (csrc/ntt_butterfly.cuh) on chosen raw limbs.

A transform test feeds k_ntt_pass canonical scalars; after the conversion to Montgomery form every
intermediate value is pseudo-random, so whether an operand sits at 2r - 1, a limb-wise difference
is negative before its bias, or a limb sits at its maximum is left to chance.
bh_selftest_ntt_butterfly (csrc/selftest_ntt.hip) runs each device function on the raw 9-limb
operands given here, one launch per kind, and every output is checked against Python integers:

  (a) its value is congruent mod r to the butterfly's definition (a Montgomery product carries the
      factor 2^-261);
  (b) its value is below the bound the code documents;
  (c) limbs 0..7 are at most 2^29 - 1 (every output here is called normalised or carried);
  (d) its integer value, read from all nine 32-bit limbs, equals the exact value the arithmetic
      gives: REDC is deterministic, so mont() below yields the exact representative of every
      product and the model predicts each output as an integer, not only as a residue.  A limb
      that wrapped where the code does not announce it shows as a value off by a multiple of 2^29.

Operands are the contract's maxima and edges in every position, crossed with each other; the
products that cannot be chosen directly (u2, u3 of the DIF step; t0, t1, s0, s1 of the DIT step)
are steered to both ends of their range by solving for a preimage under mont() on the CPU
(_product_ends, _sliver_pairs)."""
import ctypes
import random

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
BITS, MASK, NL = 29, (1 << 29) - 1, 9
RR = 1 << (BITS * NL)                    # the Montgomery radix 2^261
RI = pow(RR, -1, R)
NEG_RINV = (-pow(R, -1, RR)) % RR         # -r^-1 mod 2^261
TOP = 8 * BITS                            # bit position of the top limb
R8 = R >> TOP
T2R = (2 * R) >> TOP                      # the top limb of 2r
ONE = RR % R                              # Montgomery form of 1

(DIF2, DIF2_UNIT, DIT2, DIT2_UNIT, DIF4, DIF4_UNIT, DIT4, DIT4_UNIT, QREDUCE, NORM, STORE_PLAIN, STORE_SCALARS,
 STORE_PRODUCT) = range(13)
N_IN = {DIF2: 3, DIF2_UNIT: 3, DIT2: 3, DIT2_UNIT: 3, DIF4: 7, DIF4_UNIT: 7, DIT4: 7, DIT4_UNIT: 7, QREDUCE: 1,
        NORM: 1, STORE_PLAIN: 3, STORE_SCALARS: 3, STORE_PRODUCT: 3}
N_OUT = {DIF2: 18, DIF2_UNIT: 18, DIT2: 18, DIT2_UNIT: 18, DIF4: 36, DIF4_UNIT: 36, DIT4: 36, DIT4_UNIT: 36,
         QREDUCE: 9, NORM: 9, STORE_PLAIN: 9, STORE_SCALARS: 8, STORE_PRODUCT: 9}


def _limbs(x):
    """normalised limbs of x < 2^264 (the top limb takes what is left)"""
    assert 0 <= x < 1 << (TOP + 32)
    return [(x >> (BITS * i)) & MASK for i in range(8)] + [x >> TOP]


def _value(ls):
    return sum(int(v) << (BITS * i) for i, v in enumerate(ls))


def mont(a, b):
    """fe_mul<FrCfg> exactly: (a b + m r) / 2^261 with m = -a b / r mod 2^261 (the m_k of the column
    walk are m's 29-bit digits whatever the operands' limbs were, as long as no column overflows)"""
    t = a * b
    return (t + (t * NEG_RINV % RR) * R) >> (BITS * NL)


def csub2(x):
    return x - 2 * R if x >= 2 * R else x


def qred(x):
    """fr_qreduce with the exact quotient floor(x8 / (r8 + 1))"""
    return x - ((x >> TOP) // (R8 + 1)) * R


def _run(kind, cases):
    """cases: lists of N_IN[kind] operands, each an integer (normalised here) or a list of 9 raw limbs"""
    import bellman_hip as bh
    f = bh.lib().bh_selftest_ntt_butterfly
    f.restype = ctypes.c_int
    f.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    rows = [sum(((_limbs(x) if isinstance(x, int) else list(x)) for x in c), []) for c in cases]
    inp = np.array(rows, dtype=np.uint32)
    assert inp.shape == (len(cases), N_IN[kind] * NL)
    out = np.full((len(cases), N_OUT[kind]), 0xFFFFFFFF, dtype=np.uint32)
    assert f(0, kind, inp.ctypes.data, len(cases), out.ctypes.data) == 0
    return out


def _check(res, k, want, residue, bound, ctx):
    """output k of one case: (a) residue, (b) bound, (c) normalised limbs, (d) the exact integer"""
    ls = res[k * NL:(k + 1) * NL]
    got = _value(ls)
    assert got % R == residue % R, ("residue", k, ctx)
    assert got < bound, ("bound", k, ctx)
    assert all(int(v) <= MASK for v in ls[:8]), ("limbs", k, ctx)
    assert got == want, ("value", k, ctx)


def _twiddles(rng):
    from oracle import bls12_381 as bls
    tw = [ONE, R - 1, 1, 0]
    for lg in (1, 2, 3, 10, 17, 32):   # omega_{2^lg}, and a power of it, in Montgomery form
        w = pow(bls.FR_ROOT_OF_UNITY, 1 << (bls.FR_S - lg), R)
        tw += [w * RR % R, pow(w, 3, R) * RR % R]
    return tw + [rng.randrange(R) for _ in range(12)]


def _specials(bound, rng, n_random):
    """values < bound (a multiple of 2r, or 2^232 for 'top limb zero'), normalised: the ends, r's
    neighbours, every low limb at its maximum, a single non-zero limb at each position, random"""
    top = (bound - 1) >> TOP
    low_full = (1 << TOP) - 1
    s = [0, 1, R - 1, R, R + 1, bound - 1, bound - R, low_full, ((top - 1) << TOP) | low_full if top else low_full,
         top << TOP]
    s += [MASK << (BITS * i) for i in range(8)] + [1 << (BITS * i) for i in range(NL)]
    s += [rng.randrange(bound) for _ in range(n_random)]
    assert all(0 <= v < bound for v in s)
    return s


def _product_ends(rng, tw, bound, floor=0):
    """(a, w, t) with floor <= a < bound (a multiple of r), a twiddle w < r and mont(a, w) == t, for
    t at the ends of the product's range.  mont(a, w) = (a w + m r) / 2^261 with 0 <= m < 2^261 is
    the one representative t of a w 2^-261 with a w / 2^261 in (t - r, t], so the range is
    [0, r + bound r / 2^261): 0 and 1 need a small a w (the twiddles 0 and 1), r - 1, r and r + 1
    come from any representative, and the top end from a in [bound - r, bound) against
    t = r + floor((bound - r) w / 2^261) - 1, within r / 70 of the supremum."""
    A = bound // R
    assert bound == A * R and A < 70

    def rep(residue, lo):       # the smallest representative >= lo
        a = residue % R
        return a + (max(lo - a, 0) + R - 1) // R * R

    ends = [(rep(0, floor), 0, 0), (rep(ONE, floor), 1, 1)]
    if floor == 0:
        ends.append((0, tw[-1], 0))
    for w in (R - 1, tw[4], rng.randrange(R >> 1, R)):
        wi = pow(w, -1, R)
        ends += [(rep(t * RR * wi, max(floor, 1)), w, t) for t in (R - 1, R, R + 1)]
        t = R + (((A - 1) * R * w) >> (BITS * NL)) - 1
        ends.append((t * RR * wi % R + (A - 1) * R, w, t))
    for a, w, t in ends:
        assert floor <= a < bound and w < R and mont(a, w) == t, (hex(a), hex(w), hex(t))
    return ends


def _sliver_pairs(rng, cap=64, want=4):
    """(a, w, t) with a < 2r, mont(a, w) == t and t in [T2R 2^232, 2r), where t's top limb equals
    2r's.  No twiddle w < r reaches it (mont(a, w) < r + a r / 2^261 < 1.32 r for a < 22r), so w is a
    wide factor < 2^261 with normalised limbs, which fe_mul takes (a w < 2^261 r keeps t < 2r) but
    no twiddle table holds.  A seeded search with a cap: which of t, t - r the REDC lands on
    depends on a w / 2^261."""
    lo = T2R << TOP
    found = []
    targets = [lo, 2 * R - 1] + [lo + rng.randrange(2 * R - lo) for _ in range(cap - 2)]
    for t in targets:
        w = rng.randrange(RR * 8 // 10, RR * 95 // 100)
        a = t * RR * pow(w, -1, R) % R + R
        if mont(a, w) == t:
            found.append((a, w, t))
        if len(found) == want:
            break
    return found


# ---------------------------------------------------------------- radix-2
def _r2_cases(rng):
    tw = _twiddles(rng)
    sp = _specials(2 * R, rng, 24)
    cases = [(2 * R - 1, 0, ONE), (0, 2 * R - 1, ONE), (2 * R - 1, 2 * R - 1, R - 1)]
    for i, v in enumerate(sp):
        u = sp[(3 * i + 1) % len(sp)]
        for j, (x, y) in enumerate(((v, v), (v, u), (u, v))):    # difference zero, and both signs
            cases.append((x, y, tw[(i + j) % len(tw)]))
    for i, w in enumerate(tw):                                   # every twiddle against the maxima
        cases += [(0, 2 * R - 1, w), (2 * R - 1, 0, w), (sp[i % len(sp)], 2 * R - 1, w)]
    # DIT: the product t = y w at both ends of its range
    for y, w, _ in _product_ends(rng, tw, 2 * R):
        cases += [(0, y, w), (2 * R - 1, y, w), ((1 << TOP) - 1, y, w)]
    cases += [(rng.randrange(2 * R), rng.randrange(2 * R), rng.randrange(R)) for _ in range(256)]
    return cases


def test_radix2_butterflies():
    rng = random.Random(1729)
    cases = _r2_cases(rng)
    outs = {k: _run(k, cases) for k in (DIF2, DIF2_UNIT, DIT2, DIT2_UNIT)}
    for i, (x, y, w) in enumerate(cases):
        c = ("r2", i, hex(x), hex(y), hex(w))
        _check(outs[DIF2][i], 0, csub2(x + y), x + y, 2 * R, c)
        _check(outs[DIF2][i], 1, mont(x + 4 * R - y, w), (x - y) * w * RI, 2 * R, c)
        t = mont(y, w)
        assert t < 2 * R and t % R == y * w * RI % R
        _check(outs[DIT2][i], 0, x + t, x + y * w * RI, 4 * R, c)
        _check(outs[DIT2][i], 1, x + 2 * R - t, x - y * w * RI, 4 * R, c)
        for kind in (DIF2_UNIT, DIT2_UNIT):     # the twiddle is not read
            _check(outs[kind][i], 0, csub2(x + y), x + y, 2 * R, c)
            _check(outs[kind][i], 1, csub2(x + 2 * R - y), x - y, 2 * R, c)


# ---------------------------------------------------------------- radix-4, DIF
def _dif4_model(x, wa0, wa1, wb, unit):
    s02, s13 = x[0] + x[2], x[1] + x[3]
    u2, u3 = mont(x[0] + 4 * R - x[2], wa0), mont(x[1] + 4 * R - x[3], wa1)
    assert u2 < 2 * R and u3 < 2 * R
    y0, y2 = qred(s02 + s13), csub2(u2 + u3)
    if unit:
        return [y0, qred(s02 + 8 * R - s13), y2, qred(u2 + 4 * R - u3)], u2, u3
    return [y0, mont(s02 + 8 * R - s13, wb), y2, mont(u2 + 4 * R - u3, wb)], u2, u3


def _dif4_cases(rng):
    tw = _twiddles(rng)
    sp = _specials(2 * R, rng, 16)
    hi = 2 * R - 1
    cases = []
    # outer pairs and the inner sums s02 - s13: most negative, zero, maximal
    for w in (ONE, R - 1, tw[4], tw[-1]):
        cases += [([0, hi, 0, hi], w, w, w), ([hi, 0, hi, 0], w, w, w), ([hi, hi, hi, hi], w, w, w),
                  ([0, 0, 0, 0], w, w, w), ([hi, hi, 0, 0], w, w, w), ([0, 0, hi, hi], w, w, w),
                  ([hi, 0, 0, hi], w, w, w), ([0, hi, hi, 0], w, w, w)]
    for i, v in enumerate(sp):
        a, b, c = sp[(i + 1) % len(sp)], sp[(3 * i + 2) % len(sp)], sp[(5 * i + 3) % len(sp)]
        for j, x in enumerate(([v, v, v, v], [v, a, b, c], [a, v, c, b], [b, c, v, a], [c, b, a, v])):
            cases.append((x, tw[(i + j) % len(tw)], tw[(2 * i + j + 1) % len(tw)], tw[(3 * i + j + 2) % len(tw)]))
    # u2 - u3 at its ends: each product steered to 0, 1, r - 1, r, r + 1 and the top of its range
    # through the operand x0 + 4r - x2 (in (2r, 6r)), every end against every other
    ends = _product_ends(rng, tw, 6 * R, floor=2 * R + 1)

    def split(op):      # operand = x0 + 4r - x2 with x0, x2 < 2r
        d = op - 4 * R
        return (d, 0) if d >= 0 else (0, -d)
    for a2, w2, _ in ends:
        for a3, w3, _ in ends:
            (x0, x2), (x1, x3) = split(a2), split(a3)
            cases.append(([x0, x1, x2, x3], w2, w3, tw[(len(cases)) % len(tw)]))
    for _ in range(256):
        cases.append(([rng.randrange(2 * R) for _ in range(4)], rng.randrange(R), rng.randrange(R), rng.randrange(R)))
    return cases, ends


def test_radix4_dif_butterfly():
    rng = random.Random(4104)
    cases, ends = _dif4_cases(rng)
    assert {t for _, _, t in ends} >= {0, 1, R - 1, R, R + 1} and max(t for _, _, t in ends) > R + 5 * R // 71
    flat = [x + [wa0, wa1, wb] for x, wa0, wa1, wb in cases]
    outs = {k: _run(k, flat) for k in (DIF4, DIF4_UNIT)}
    seen = set()
    for i, (x, wa0, wa1, wb) in enumerate(cases):
        c = ("dif4", i, [hex(v) for v in x], hex(wa0), hex(wa1), hex(wb))
        d02, d13 = (x[0] - x[2]) * wa0 * RI, (x[1] - x[3]) * wa1 * RI
        for kind, unit in ((DIF4, False), (DIF4_UNIT, True)):
            want, u2, u3 = _dif4_model(x, wa0, wa1, wb, unit)
            f = 1 if unit else wb * RI
            residues = [sum(x), (x[0] + x[2] - x[1] - x[3]) * f, d02 + d13, (d02 - d13) * f]
            for k in range(4):
                _check(outs[kind][i], k, want[k], residues[k], 2 * R, c + (kind,))
        seen.add((u2 < u3, u2 == u3, u2 > u3))
        seen.add((u2, u3) if 0 in (u2, u3) else None)
    # the inner difference u2 - u3 was negative, zero and positive, and most negative and maximal
    assert {(True, False, False), (False, True, False), (False, False, True)} <= seen
    top = max(t for _, _, t in ends)
    assert (0, top) in seen and (top, 0) in seen


# ---------------------------------------------------------------- radix-4, DIT
def _dit4_model(x, wa, wb0, wb1, unit):
    if unit:
        a0, a1 = csub2(x[0] + x[1]), csub2(x[0] + 2 * R - x[1])
        p2, p3 = csub2(x[2] + x[3]), csub2(x[2] + 2 * R - x[3])
        t0 = t1 = None
    else:
        t0, t1 = mont(x[1], wa), mont(x[3], wa)
        assert t0 < 2 * R and t1 < 2 * R
        a0, a1, p2, p3 = x[0] + t0, x[0] + 2 * R - t0, x[2] + t1, x[2] + 4 * R - t1
    s0, s1 = mont(p2, wb0), mont(p3, wb1)
    assert s0 < 2 * R and s1 < 2 * R
    return [a0 + s0, a1 + s1, a0 + 2 * R - s0, a1 + 2 * R - s1], t0, (a0, s0)


def _dit4_cases(rng, j, n_random):
    """(x, wa, wb0, wb1, wide): inputs < B = 2r(j + 1), the contract of the step at position j of
    its pass; wide marks a factor >= r where a twiddle stands (_sliver_pairs)"""
    B = 2 * R * (j + 1)
    tw = _twiddles(rng)
    sp = _specials(B, rng, 6)
    cases = []
    for w in (ONE, R - 1, tw[6]):
        cases += [([B - 1] * 4, w, w, w), ([0] * 4, w, w, w), ([0, B - 1, 0, B - 1], w, w, w),
                  ([B - 1, 0, B - 1, 0], w, w, w)]
    for i, v in enumerate(sp):
        a, b, c = sp[(i + 1) % len(sp)], sp[(3 * i + 2) % len(sp)], sp[(5 * i + 3) % len(sp)]
        for k, x in enumerate(([v, v, v, v], [v, a, b, c], [a, v, c, b], [b, c, v, a], [c, b, a, v])):
            cases.append((x, tw[(i + k + j) % len(tw)], tw[(2 * i + k + 1) % len(tw)], tw[(3 * i + k + 2) % len(tw)]))
    # every product at the ends of its range against x0 (and so a0, a1) at the ends of its own:
    # t0 = x1 wa and t1 = x3 wa; s0 = (x2 + t1) wb0 and s1 = (x2 + 4r - t1) wb1 with x3 = 0 (t1 = 0)
    small = [0, 1, (1 << TOP) - 1, rng.randrange(1 << TOP)]
    for x1, wa, _ in _product_ends(rng, tw, B):
        for x0 in small + [B - 1]:
            cases.append(([x0, x1, rng.randrange(B), x1], wa, tw[len(cases) % len(tw)], tw[(len(cases) + 5) % len(tw)]))
    for x2, wb0, _ in _product_ends(rng, tw, B):
        cases += [([x0, 0, x2, 0], ONE, wb0, tw[len(cases) % len(tw)]) for x0 in small + [B - 1]]
    for p3, wb1, _ in _product_ends(rng, tw, B + 4 * R, floor=4 * R):
        cases += [([x0, 0, p3 - 4 * R, 0], ONE, tw[len(cases) % len(tw)], wb1) for x0 in small + [B - 1]]
    for _ in range(n_random):
        cases.append(([rng.randrange(B) for _ in range(4)], rng.randrange(R), rng.randrange(R), rng.randrange(R)))
    cases = [c + (False,) for c in cases]
    # a product in the sliver where its top limb equals 2r's, under x0 (a0) < 2^232: the top limb of
    # a1 = x0 + 2r - t0 (of a0 + 2r - s0 before lw_norm) goes below zero and wraps
    for a, w, _ in _sliver_pairs(rng):
        for x0 in small:
            cases.append(([x0, a, rng.randrange(B), 0], w, tw[len(cases) % len(tw)], tw[(len(cases) + 5) % len(tw)], True))
            cases.append(([x0, 0, a, 0], ONE, w, tw[len(cases) % len(tw)], True))
    return cases


@pytest.fixture(scope="module")
def dit4_runs():
    """every step position's cases in one launch per kind"""
    rng = random.Random(8128)
    cases = [(j,) + c for j in range(9) for c in _dit4_cases(rng, j, 24)]
    unit = [c for c in cases if c[0] == 0 and not c[5]]
    flat = [[x + [wa, wb0, wb1] for _, x, wa, wb0, wb1, _ in cs] for cs in (cases, unit)]
    return cases, _run(DIT4, flat[0]), unit, _run(DIT4_UNIT, flat[1])


def test_radix4_dit_butterfly_keeps_the_lazy_bound_at_every_step(dit4_runs):
    """Inputs < 2r(j + 1) give outputs < 2r(j + 3) for every step position j = 0..8 of a pass, each
    at its input maximum.  A pass starts from values < 2r and its steps chain (a radix-2 first stage
    gives < 4r, the contract at j = 1), so the whole-pass bound '< 22r after 10 stages' follows by
    induction from these cases: no single transform has to reach it by chance.

    The top-limb wrap ntt_dit4 tolerates in a1 needs t0's top limb to equal 2r's.  With a twiddle
    < r that cannot happen: t0 = x1 wa 2^-261 < r + x1 r / 2^261 < 1.26 r for x1 < 18r, and the
    directed search over in-contract operands confirms no wrap (asserted below).  The wrap is
    therefore driven with wide factors (>= r, _sliver_pairs), which fe_mul accepts and no twiddle
    table holds, so that the tolerance stays covered."""
    cases, out, _, _ = dit4_runs
    wraps = pre_norm_wraps = 0
    assert ((R + (18 * R * R >> (BITS * NL)) + 1) >> TOP) < T2R      # t0's top limb stays below 2r's
    for i, (j, x, wa, wb0, wb1, wide) in enumerate(cases):
        c = ("dit4", i, j, [hex(v) for v in x], hex(wa), hex(wb0), hex(wb1))
        assert max(x) < 2 * R * (j + 1) and (wide or max(wa, wb0, wb1) < R)
        want, t0, (a0, s0) = _dit4_model(x, wa, wb0, wb1, False)
        t0r, t1r = x[1] * wa * RI, x[3] * wa * RI
        residues = [(x[0] + t0r) + (x[2] + t1r) * wb0 * RI, (x[0] - t0r) + (x[2] - t1r) * wb1 * RI,
                    (x[0] + t0r) - (x[2] + t1r) * wb0 * RI, (x[0] - t0r) - (x[2] - t1r) * wb1 * RI]
        for k in range(4):
            _check(out[i], k, want[k], residues[k], 2 * R * (j + 3), c)
        # a1's top limb: x0's + FrBias<2, 1>'s (2r's minus 1) - t0's, negative before the carried sums
        wrap = (x[0] >> TOP) + T2R - 1 - (t0 >> TOP) < 0
        pre_norm_wrap = (a0 >> TOP) + T2R - 1 - (s0 >> TOP) < 0
        assert wide or not (wrap or pre_norm_wrap), c
        wraps += wrap
        pre_norm_wraps += pre_norm_wrap
    # the deliberate wrap stays covered (the search is seeded and capped; none found is a finding)
    assert wraps >= 1, "no case made a1's top limb wrap"
    assert pre_norm_wraps >= 1, "no case made y2's top limb wrap before lw_norm"


def test_radix4_dit_butterfly_with_the_unit_twiddle(dit4_runs):
    """unit_a is only reached at global stage 0, on freshly loaded values: inputs < 2r, outputs < 4r"""
    _, _, cases, out = dit4_runs
    assert len(cases) > 100
    for i, (j, x, wa, wb0, wb1, _) in enumerate(cases):
        c = ("dit4 unit", i, [hex(v) for v in x], hex(wb0), hex(wb1))
        want, _, _ = _dit4_model(x, wa, wb0, wb1, True)
        residues = [(x[0] + x[1]) + (x[2] + x[3]) * wb0 * RI, (x[0] - x[1]) + (x[2] - x[3]) * wb1 * RI,
                    (x[0] + x[1]) - (x[2] + x[3]) * wb0 * RI, (x[0] - x[1]) - (x[2] - x[3]) * wb1 * RI]
        for k in range(4):
            _check(out[i], k, want[k], residues[k], 4 * R, c)


# ---------------------------------------------------------------- fr_qreduce, lw_norm
def test_qreduce_runs_the_fp64_quotient_at_every_multiple_boundary():
    """The device's __builtin_fma at every top limb next to a multiple of r8 + 1, which
    tests/test_ntt_reduction_math.py only restates on the host.  (Dropping the 0.5 * inv addend of
    the fma cannot fail here or anywhere: the rounded 1 / (r8 + 1) lies above the true quotient, so
    the quotient is exact without it -- profiles/ntt_butterfly_mutations.txt, m3.)"""
    rng = random.Random(2606)
    d = R8 + 1
    low_full = (1 << TOP) - 1
    cases = []
    for k in range((1 << BITS) // d + 1):
        for x8 in (k * d - 1, k * d, k * d + 1):
            if 0 <= x8 < 1 << BITS:
                cases += [(x8 << TOP) | low for low in (0, low_full, rng.randrange(1 << TOP))]
    assert len(cases) > 3 * 3 * 70
    cases += [RR - 1, 0, R - 1, R, 2 * R - 1, 2 * R, 22 * R - 1, 12 * R - 1] + [rng.randrange(RR) for _ in range(512)]
    out = _run(QREDUCE, [[x] for x in cases])
    for x, res in zip(cases, out):
        want = qred(x)
        assert 0 <= want < 2 * R
        _check(res, 0, want, x, 2 * R, ("qreduce", hex(x)))


def test_norm_carries_unnormalised_limbs():
    """lw_norm at its call sites' limb maximum 5 * 2^29 - 3 (value mod 2^264 kept, limbs 0..7
    normalised), and with a top limb that wrapped below zero under a non-negative value"""
    rng = random.Random(31)
    big = 5 * (1 << BITS) - 3
    cases = [[0] * 9, [MASK] * 9, [big] * 8 + [0], [big] * 8 + [MASK - 8], [big] * 8 + [0xFFFFFFFF],
             [MASK] * 8 + [0xFFFFFFFF], [0] * 8 + [0xFFFFFFFF]]
    cases += [[rng.randrange(big + 1) for _ in range(8)] + [rng.randrange(1 << BITS)] for _ in range(256)]
    cases += [[rng.choice((0, MASK, MASK + 1, big)) for _ in range(8)] + [rng.choice((0, 0xFFFFFFFE, 7))]
              for _ in range(128)]
    out = _run(NORM, [[c] for c in cases])
    for c, res in zip(cases, out):
        assert _value(res) == _value(c) % (1 << (TOP + 32)), c
        assert all(int(v) <= MASK for v in res[:8]), c


# ---------------------------------------------------------------- store paths
LAZY, HAS_SUB = 1, 2


def _flags(f):
    return [f] + [0] * 8


def test_plain_store_reduces_a_lazy_value_and_subtracts():
    rng = random.Random(77)
    xs = [0, 1, R, 2 * R - 1, 2 * R, 2 * R + 1, 22 * R - 1, 22 * R - R, RR - 1] + [rng.randrange(22 * R) for _ in range(64)]
    subs = [0, 1, R, 2 * R - 1] + [rng.randrange(2 * R) for _ in range(4)]
    cases = []
    for x in xs:
        cases.append((x, 0, LAZY))
        cases += [(x, s, LAZY | HAS_SUB) for s in subs]
        if x < 2 * R:       # a post-scaled or DIF value: no reduction
            cases.append((x, 0, 0))
            cases += [(x, s, HAS_SUB) for s in subs]
    out = _run(STORE_PLAIN, [[x, s, _flags(f)] for x, s, f in cases])
    for (x, s, f), res in zip(cases, out):
        want = qred(x) if f & LAZY else x
        assert want < 2 * R
        if f & HAS_SUB:
            want = csub2(want + 2 * R - s)
        _check(res, 0, want, x - s if f & HAS_SUB else x, 2 * R, ("plain", hex(x), hex(s), f))


def test_scalars_epilogue_is_canonical_after_one_subtraction():
    """x < 22r (a bare DIT value) plus 2r - sub stays < 24r < 2^261, so x 2^-261 <= r and one
    conditional subtraction gives the canonical scalar; a multiple of r gives exactly 0"""
    rng = random.Random(78)
    cases = [(R * k, 0, 0) for k in range(22)] + [(R * k, 0, HAS_SUB) for k in range(22)]
    cases += [(22 * R - 1, 0, 0), (22 * R - 1, 0, HAS_SUB), (22 * R - 1, 2 * R - 1, HAS_SUB), (0, 2 * R - 1, HAS_SUB),
              (0, R, HAS_SUB), (R - 1, R - 1, HAS_SUB), (1, 0, 0), (ONE, 0, 0), (RR - 1, 0, 0)]
    cases += [(rng.randrange(22 * R), 0, 0) for _ in range(128)]
    cases += [(rng.randrange(22 * R), rng.randrange(2 * R), HAS_SUB) for _ in range(128)]
    out = _run(STORE_SCALARS, [[x, s, _flags(f)] for x, s, f in cases])
    for (x, s, f), res in zip(cases, out):
        got = sum(int(w) << (32 * i) for i, w in enumerate(res))
        v = x + 2 * R - s if f & HAS_SUB else x
        assert v < RR
        assert got == v * RI % R, ("scalars", hex(x), hex(s), f)      # canonical: the residue itself, < r
    assert all(not out[i].any() for i in range(44))                    # x = r k: exactly 0


def test_product_epilogue_ends_below_2r():
    rng = random.Random(79)
    tw = _twiddles(rng)
    pas = [0, 1, R, 2 * R - 1, (1 << TOP) - 1] + [rng.randrange(2 * R) for _ in range(8)]
    xs = [0, 1, 22 * R - 1, 21 * R, ((22 * R - 1) >> TOP << TOP) - 1] + [rng.randrange(22 * R) for _ in range(8)]
    cases = [(pa, x, tw[(i + 3 * j) % len(tw)]) for i, pa in enumerate(pas) for j, x in enumerate(xs)]
    cases += [(2 * R - 1, 22 * R - 1, k) for k in tw]
    out = _run(STORE_PRODUCT, [list(c) for c in cases])
    for (pa, x, k), res in zip(cases, out):
        p = mont(pa, x)
        assert p < 2 * R
        _check(res, 0, mont(p, k), pa * x * k * RI * RI, 2 * R, ("product", hex(pa), hex(x), hex(k)))
