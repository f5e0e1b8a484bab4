"""Every Montgomery product form of csrc/field.cuh against Python integers, in both column forms.

bh_selftest_field_products (csrc/selftest.hip) evaluates, on caller-chosen raw limbs, fe_mul,
fe_sqr, fe_mul2, fe_from_mont (Fp), fe2_mul_kara, fe2_mul_sub_kara (Fp2) and fe_mul (Fr), once with
split column chains and a merge add per column and once with carry-seeded column chains
(BH_COLUMN_CHAIN).  Only the association order of exact 64-bit sums differs between the two, so
their limbs must be identical; the values are checked modulo p or r.  One launch of a few
workgroups covers zero and one, p - 1, p, 2p - 1, 127p + (p - 1), every limb at 2^29 - 1 where a
form's bound allows it, a single non-zero limb at each position, and 4 096 random values.

The Fr product also takes the NTT's unnormalised operands (csrc/ntt_butterfly.cuh): a normalised
value plus a bias K r whose limbs carry J 2^29 lent from the limb above, limb-wise, with limbs up to
5 * 2^29 - 3 and values up to 26r - 1, against a factor below r."""
import ctypes
import random

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

P = 0x1A0111EA397FE69A4B1BA7B6434BACD764774B84F38512BF6730D2A0F6B0F6241EABFFFEB153FFFFB9FEFFFFFFFFAAAB
R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
BITS, MASK = 29, (1 << 29) - 1
NP, NR = 14, 9
RP, RR = 1 << (BITS * NP), 1 << (BITS * NR)
LAZY_MAX = (1 << 386) - 1       # fe2_mul_sub_kara: operands < 2^386
N_IN, N_OUT = 8 * NP + 2 * NR, 8 * NP + NR


def _limbs(x, n):
    assert 0 <= x < 1 << (BITS * n)
    return [(x >> (BITS * i)) & MASK for i in range(n)]


def _value(ls):
    return sum(int(v) << (BITS * i) for i, v in enumerate(ls))


def _cases():
    rng = random.Random(2922)
    fp = [0, 1, P - 1, P, 2 * P - 1, 127 * P + (P - 1), RP - 1] + [MASK << (BITS * i) for i in range(NP)]
    fp += [1 << (BITS * i) for i in range(NP)]
    fr = [0, 1, R - 1, R, 2 * R - 1, 7 * R + (R - 1), RR - 1] + [MASK << (BITS * i) for i in range(NR)]
    fr += [1 << (BITS * i) for i in range(NR)]
    lazy = [min(v, LAZY_MAX) for v in fp] + [LAZY_MAX]
    cases = []
    # every special value in every operand position at least once, against every other special value
    for i, v in enumerate(fp):
        w, x, y = fp[(i + 1) % len(fp)], fp[(3 * i + 2) % len(fp)], fp[(5 * i + 3) % len(fp)]
        for a, b, c, d in ((v, v, v, v), (v, w, x, y), (w, v, y, x), (x, y, v, w), (y, x, w, v)):
            e, f, g, h = (min(t, LAZY_MAX) for t in (a, b, c, d))
            cases.append(([a, b, c, d, e, f, g, h], [fr[i % len(fr)], fr[(2 * i + 1) % len(fr)]]))
    for i, v in enumerate(fr):
        cases.append(([fp[i % len(fp)]] * 4 + [lazy[-1]] * 4, [v, v]))
        cases.append(([fp[i % len(fp)]] * 4 + [lazy[i % len(lazy)]] * 4, [fr[(i + 3) % len(fr)], v]))
    for _ in range(4096):
        ops = [rng.randrange(128 * P) for _ in range(4)] + [rng.randrange(1 << 386) for _ in range(4)]
        cases.append((ops, [rng.randrange(8 * R) for _ in range(2)]))
    # Fr: unnormalised left operands (raw limbs) against a factor below r
    low_full = (1 << (BITS * (NR - 1))) - 1
    factors = [0, 1, R - 1, RR % R, low_full] + [rng.randrange(R) for _ in range(3)]
    for k, j in ((2, 1), (4, 1), (8, 2)):
        bias = _fr_bias(k, j)
        top = (26 - k) * R - 1                      # the value stays <= 26r - 1
        vals = [0, 1, R, top, low_full, (top >> (BITS * (NR - 1)) << (BITS * (NR - 1))) - 1]
        vals += [rng.randrange(top + 1) for _ in range(10)]
        for v in vals:
            for m in range(1, j + 1):               # a sum of m <= J normalised values, limb-wise
                parts = [v - (m - 1) * (v // m)] + [v // m] * (m - 1)
                x = [sum(t) for t in zip(bias, *(_limbs(q, NR) for q in parts))]
                assert _value(x) == v + k * R < 26 * R and max(x) <= 5 * (1 << BITS) - 3
                cases += [([0] * 8, [x, f]) for f in factors]
    # the largest limbs the butterflies produce: every low limb of both summands at 2^29 - 1, plus FrBias<8, 2>
    x = [2 * a + b for a, b in zip(_limbs(low_full, NR), _fr_bias(8, 2))]
    assert 9 << (BITS - 1) < max(x) <= 5 * (1 << BITS) - 3 and _value(x) < 26 * R
    cases += [([0] * 8, [x, f]) for f in factors]
    return cases


def _fr_bias(k, j):
    """FrBias<K, J> of csrc/ntt_butterfly.cuh: K r, each limb below the top with J 2^29 lent by the limb above"""
    kr = _limbs(k * R, NR)
    return [kr[i] + ((j << BITS) if i < NR - 1 else 0) - (j if i > 0 else 0) for i in range(NR)]


def _run(cases):
    import bellman_hip as bh
    f = bh.lib().bh_selftest_field_products
    f.restype = ctypes.c_int
    f.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    inp = np.array([sum((_limbs(x, NP) for x in fp), []) +
                    sum((_limbs(x, NR) if isinstance(x, int) else list(x) for x in fr), []) for fp, fr in cases],
                   dtype=np.uint32)
    assert inp.shape == (len(cases), N_IN)
    out = np.zeros((len(cases), 2, N_OUT), dtype=np.uint32)
    assert f(0, inp.ctypes.data, len(cases), out.ctypes.data) == 0
    return out


def test_every_product_form_matches_integers_and_both_column_forms_agree():
    cases = _cases()
    out = _run(cases)
    # limb for limb: split chains (form 0) against carry-seeded chains (form 1)
    assert np.array_equal(out[:, 0, :], out[:, 1, :])
    rpi, rri = pow(RP, -1, P), pow(RR, -1, R)
    for (fp, fr), res in zip(cases, out[:, 1, :]):
        a, b, c, d, e, f, g, h = fp
        x, y = (v if isinstance(v, int) else _value(v) for v in fr)
        got = [_value(res[k * NP:(k + 1) * NP]) for k in range(8)]
        in_bound = max(a, b, c, d) < 128 * P
        want = [a * b * rpi, a * a * rpi, (a * b + c * d) * rpi, a * rpi]
        for k in range(4):
            assert got[k] % P == want[k] % P, (k, fp)
            assert all(int(v) <= MASK for v in res[k * NP:(k + 1) * NP - 1]), (k, fp)
            if in_bound:
                assert got[k] < 2 * P, (k, fp)
        if in_bound:    # fe2_mul_kara's sign fix-up is argued for operands < 128p
            assert got[4] % P == (a * c - b * d) * rpi % P and got[4] < 2 * P, fp
            assert got[5] % P == (a * d + b * c) * rpi % P and got[5] < 2 * P, fp
        # (e + f u)(g + h u) - (h + e u)(f + g u)
        assert got[6] % P == ((e * g - f * h) - (h * f - e * g)) * rpi % P and got[6] < 2 * P, fp
        assert got[7] % P == ((e * h + f * g) - (h * g + e * f)) * rpi % P and got[7] < 2 * P, fp
        s = _value(res[8 * NP:])
        assert s % R == x * y * rri % R, fr
        if max(x, y) < 8 * R:
            assert s < 2 * R, fr
        if x < 26 * R and y < R:    # the NTT's rule: an operand below 26r times a factor below r (26 r^2 < 2^261 r)
            assert s < 2 * R, fr
