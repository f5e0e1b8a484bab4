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
