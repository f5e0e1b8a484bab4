"""Worst column sums of every Montgomery product form of csrc/field.cuh (pure-Python model).

With carry-seeded columns (BH_COLUMN_CHAIN) every partial sum of a 64-bit column accumulator is
fenced by an assumption that it differs from bh_column_fence = 2^64 - 1 (the signed accumulator of
fe2_mul_kara: from 2^63 - 1).  The assumption must never be false, so for each form the model walks
the columns exactly as the device code does, with every operand limb at its maximum, and asserts the
largest value an accumulator (or an unfenced partial Karatsuba sum) can hold stays below the fence
and below 2^64.  All partial sums of a column grow monotonically towards the column's final value
(after the signed difference of the Karatsuba forms), so the extremes are the column ends.

Limb maxima: 29-bit limbs (every limb, the top one included: a superset of the documented operand
bound < 128p, and of Fr's < 2^261), 30-bit limbs for fe_sqr's doubled operand and the Karatsuba
sums; fe2_mul_sub_kara's operands are < 2^386 (its documented bound), i.e. a top limb < 2^9.  The
modulus limbs are read from csrc/constants.h; a reduction factor m_k is any 29-bit value."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BITS = 29
MASK = (1 << BITS) - 1
FENCE = (1 << 64) - 1           # bh_column_fence
FENCE_SIGNED = (1 << 63) - 1    # what col_fence_signed compares a signed accumulator with


def _modulus(cfg):
    src = open(os.path.join(ROOT, "bellman-mpc_amd", "csrc", "constants.h")).read()
    body = src[src.index("struct %s {" % cfg):]
    limbs = re.search(r"uint32_t P\[(\d+)\] = \{([^}]*)\}", body)
    p = [int(x, 16) for x in limbs.group(2).split(",")]
    assert len(p) == int(limbs.group(1))
    return p


FP, FR = _modulus("FpCfg"), _modulus("FrCfg")


def _pairs(k, n):
    return range(max(0, k - n + 1), min(k, n - 1) + 1)


def _colsum(k, la, lb):
    return sum(la[i] * lb[k - i] for i in _pairs(k, len(la)))


def _mp(k, p):
    """largest sum of m_i * P[k - i] over the m's already known in column k, then m_k * P[0]"""
    n = len(p)
    before = sum(MASK * p[k - i] for i in range(max(0, k - n + 1), k if k < n else n))
    return before, (MASK * p[0] if k < n else 0)


def _walk_unsigned(p, products, p0_one=False):
    """products(k) -> largest sum of operand products in column k; returns the largest accumulator"""
    n, acc, worst = len(p), 0, 0
    for k in range(2 * n - 1):
        before, own = _mp(k, p)
        acc += products(k) + before
        if k < n and p0_one:            # Fr: acc rounded up to a multiple of 2^29, no product
            worst = max(worst, acc + MASK)
            acc = (acc + MASK) >> BITS
            continue
        acc += own
        worst = max(worst, acc)
        acc >>= BITS
    return worst


def test_fp_product_columns_stay_below_the_fence():
    n = len(FP)
    full, dbl = [MASK] * n, [2 * MASK] * n
    forms = {
        "fe_mul": lambda k: _colsum(k, full, full),
        # cross products once against 2a, the diagonal against a
        "fe_sqr": lambda k: sum((full[i] * dbl[k - i]) if i < k - i else (full[i] * full[i] if i == k - i else 0)
                                for i in _pairs(k, n)),
        "fe_mul2": lambda k: 2 * _colsum(k, full, full),
        "fe_from_mont": lambda k: MASK if k < n else 0,
    }
    for name, products in forms.items():
        worst = _walk_unsigned(FP, products)
        assert worst < FENCE and worst < 1 << 64, name
    assert _walk_unsigned(FP, forms["fe_mul"]) < 1 << 63
    assert _walk_unsigned(FP, forms["fe_mul2"]) < 3 << 62


def test_fr_product_columns_stay_below_the_fence():
    n = len(FR)
    assert FR[0] == 1
    full, dbl = [MASK] * n, [2 * MASK] * n
    forms = {
        "fe_mul": lambda k: _colsum(k, full, full),
        "fe_sqr": lambda k: sum((full[i] * dbl[k - i]) if i < k - i else (full[i] * full[i] if i == k - i else 0)
                                for i in _pairs(k, n)),
        "fe_mul2": lambda k: 2 * _colsum(k, full, full),
        "fe_from_mont": lambda k: MASK if k < n else 0,
    }
    for name, products in forms.items():
        for p0_one in (True, False):    # fe_mul and fe_from_mont take the rounding path, the others m_k * P[0]
            worst = _walk_unsigned(FR, products, p0_one)
            assert worst < FENCE and worst < 1 << 63, name


def test_fp2_karatsuba_product_columns_stay_below_the_fences():
    """fe2_mul_kara: acc1 (unsigned) takes t2 - t0 - t1 = sum a0 b1 + a1 b0 >= 0; acc0 (signed) takes
    t0 - t1 in [-sum a1 b1, sum a0 b0]; t2 sums 30-bit x 30-bit products on its own."""
    n = len(FP)
    full, dbl = [MASK] * n, [2 * MASK] * n
    assert max(_colsum(k, dbl, dbl) for k in range(2 * n - 1)) < FENCE          # t2, unfenced, must not wrap
    assert _walk_unsigned(FP, lambda k: 2 * _colsum(k, full, full)) < FENCE       # acc1
    lo = hi = 0
    worst_lo = worst_hi = 0
    for k in range(2 * n - 1):
        before, own = _mp(k, FP)
        s = _colsum(k, full, full)
        lo, hi = lo - s, hi + s + before + own     # m*p terms are >= 0: lo keeps none of them
        worst_lo, worst_hi = min(worst_lo, lo), max(worst_hi, hi)
        lo, hi = lo >> BITS, hi >> BITS            # arithmetic shift (floor), as on the device
    assert worst_hi < FENCE_SIGNED and worst_hi < 1 << 63
    assert worst_lo >= -(1 << 63)
    # the ranges stated in field.cuh
    assert worst_lo > -(1 << 62) and worst_hi < (1 << 63) - (1 << 60)


def test_fp2_lazy_karatsuba_product_columns_stay_below_the_fence():
    """fe2_mul_sub_kara: biased unsigned accumulators, BIAS = 28 * 2^58; each half adds a difference of
    two products' column sums, in (-2S, 2S) for S = the largest column sum of one product of operands
    < 2^386; the carry is floor((acc - BIAS) / 2^29)."""
    n = len(FP)
    bias = 7 << 60
    lim = [MASK] * (n - 1) + [(1 << 9) - 1]
    lim2 = [2 * x for x in lim]
    assert max(_colsum(k, lim2, lim2) for k in range(2 * n - 1)) < FENCE          # t2, u2 on their own
    lo = hi = 0
    worst_lo, worst_hi = bias, bias
    for k in range(2 * n - 1):
        before, own = _mp(k, FP)
        s = 2 * _colsum(k, lim, lim)               # half 0: t0 + u1 at most; half 1: a0 b1 + a1 b0 at most
        lo, hi = lo - s, hi + s + before + own
        worst_lo, worst_hi = min(worst_lo, bias + lo), max(worst_hi, bias + hi)
        lo, hi = lo >> BITS, hi >> BITS
    assert worst_lo >= 0
    assert worst_hi < FENCE and worst_hi < 1 << 64
    assert worst_hi < 611 * (1 << 58) // 10     # "< 61.1 * 2^58" in field.cuh


# ---------------------------------------------------------------- the NTT's unnormalised operands
# csrc/ntt_butterfly.cuh hands fe_mul<FrCfg> limb-wise sums and differences (lw_add, lw_sub<K, J>)
# whose limbs exceed 29 bits: the largest operands that product ever sees.

def _kp(p, k):
    """KP<C, K>::make(): K * p in normalised limbs"""
    out, carry = [], 0
    for limb in p:
        t = limb * k + carry
        out.append(t & MASK)
        carry = t >> BITS
    assert carry == 0
    return out


def _fr_bias(k, j):
    """FrBias<K, J>::make(): K * r with J * 2^29 lent to every limb below the top by the limb above"""
    n = len(FR)
    out = []
    for i, c in enumerate(_kp(FR, k)):
        if i < n - 1:
            c += j << BITS
        if i > 0:
            c -= j
        assert 0 <= c < 1 << 32
        out.append(c)
    return out


def _fr_value(limbs):
    return sum(v << (BITS * i) for i, v in enumerate(limbs))


def _top(v):
    return v >> (BITS * (len(FR) - 1))


def _ntt_operand_maxima():
    """per-limb maxima of every limb-wise expression the butterflies hand to fe_mul<FrCfg>; a
    normalised value < K r has limbs 0..7 <= MASK and a top limb <= top(K r - 1)"""
    r = _fr_value(FR)
    n = len(FR)

    def norm(k):
        return [MASK] * (n - 1) + [_top(k * r - 1)]

    def add(a, b):
        return [x + y for x, y in zip(a, b)]

    def sub(k, j, a, b):
        bias = _fr_bias(k, j)
        # no limb of the subtrahend exceeds the bias: limbs below the top are sums of J normalised limbs
        assert all(bias[i] >= b[i] for i in range(n)), (k, j)
        return add(a, bias)     # the subtrahend at zero
    two = norm(2)
    s = add(two, two)                           # s02, s13: lw_add of two normalised values < 2r
    return {
        "dif lw_sub<4,1>(x, y)": sub(4, 1, two, two),
        "dif lw_sub<8,2>(s02, s13)": sub(8, 2, s, s),
        "dit a0 / p2 = lw_add(x, t), x < 18r": add(norm(18), two),
        "dit p3 = lw_sub<4,1>(x, t), x < 18r": sub(4, 1, norm(18), two),
        "dit a1 = lw_sub<2,1>(x, t), x < 18r": add(norm(18), _fr_bias(2, 1)),    # not a product operand
    }


def test_fr_bias_keeps_the_value_and_covers_its_subtrahend():
    r = _fr_value(FR)
    for k, j in ((2, 1), (4, 1), (8, 2)):
        bias = _fr_bias(k, j)
        assert _fr_value(bias) == k * r
        assert all(b >= j * MASK for b in bias[:-1])
        # the top limb covers a subtrahend < (K / 2) r, except FrBias<2, 1> against a product whose
        # top limb equals 2r's (ntt_dit4's a1: the wrap the carried sums undo)
        assert bias[-1] >= _top((k // 2) * r - 1) - (1 if (k, j) == (2, 1) else 0)


def test_ntt_operand_columns_stay_below_the_fence():
    """fe_mul<FrCfg> of each limb-wise operand against a factor with 29-bit limbs (a twiddle, and a
    superset of it: every limb at 2^29 - 1)"""
    n = len(FR)
    twiddle = [MASK] * n
    worst = {}
    for name, limbs in _ntt_operand_maxima().items():
        if "a1" in name:
            continue
        assert max(limbs) <= 5 * (1 << BITS) - 3, name
        worst[name] = _walk_unsigned(FR, lambda k, la=limbs: _colsum(k, la, twiddle), p0_one=True)
        assert worst[name] < FENCE, (name, worst[name])
    # the margin is real and under half a bit: every limb at 5 * 2^29 stays inside, at 2^32 - 1 it does not
    assert max(worst.values()) <= _walk_unsigned(FR, lambda k: _colsum(k, [5 << BITS] * n, twiddle), True) < FENCE
    assert _walk_unsigned(FR, lambda k: _colsum(k, [(1 << 32) - 1] * n, twiddle), True) > FENCE
    assert max(worst.values()) < 2 ** 63.4      # the figure quoted in ntt_butterfly.cuh


def test_lw_norm_inputs_plus_carry_fit_32_bits():
    """lw_norm adds the carry to each limb in 32 bits: at its call sites (ntt_dif4's unit branch,
    ntt_dit4's y2 and y3) no limb plus the carry into it reaches 2^32"""
    m = _ntt_operand_maxima()
    bias21 = _fr_bias(2, 1)
    sites = {
        "dif y1": m["dif lw_sub<8,2>(s02, s13)"],
        "dif y3": m["dif lw_sub<4,1>(x, y)"],
        "dit y2": [a + b for a, b in zip(m["dit a0 / p2 = lw_add(x, t), x < 18r"], bias21)],
        "dit y3": [a + b for a, b in zip(m["dit a1 = lw_sub<2,1>(x, t), x < 18r"], bias21)],
    }
    for name, limbs in sites.items():
        carry = 0
        for v in limbs:
            assert v + carry < 1 << 32, name
            carry = (v + carry) >> BITS
        assert max(limbs[:-1]) <= 5 * (1 << BITS) - 3, name
