"""bh_srs_fft, the group-valued FFT of a device point vector (csrc/group_fft.hip), against the
oracle curve's own point FFT and against the closed form of the Lagrange basis.  Bit-exact.

Sizes: n = 2 is one stage with every w = 1, n = 8 the first with three distinct twiddles, 512 (G1)
and 64 (G2) more than one workgroup, and 2^20 the smallest n at which one stage's multiplications
span two chunks (VB_WIN_CHUNK = 2^18 butterflies of a stage's 2^19)."""
import os
import random
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mpc_oracle as mo  # noqa: E402
from oracle import bellman as bm  # noqa: E402

pytestmark = pytest.mark.gpu

R = mo.R
TAU = 0x5AB3F1C2D4E6978877665544332211FFEEDDCCBBAA99887766554433221100FF % R
assert TAU.bit_length() >= 254
UNEXPECTED_IDENTITY, INVALID_ARGUMENT = 1, 10


def _bh():
    import bellman_hip as bh
    return bh


def _curve(group):
    return mo.G1 if group == 1 else mo.G2


def _enc(group, pts):
    f = mo.g1_bytes if group == 1 else mo.g2_bytes
    return b"".join(f(p) for p in pts)


def _bases(ctx, group, pts):
    return _bh().Bases(ctx, group, _enc(group, pts))


def _gen(group, k):
    return mo.g1(k) if group == 1 else mo.g2(k)


def _omega(n):
    return bm.EvaluationDomain(bm.BLS12_381, [0] * n).omega


def _status(fn, *a, **kw):
    with pytest.raises(_bh().SynthesisError) as e:
        fn(*a, **kw)
    return e.value.code


def _add(C, a, b):
    return C.to_affine(C.add(C.from_affine(a), C.from_affine(b)))


def _point_fft(C, pts, omega):
    """best_fft (domain.rs:192-228) over the oracle's points, recursively: X[k] = E[k] + w^k O[k],
    X[k + n/2] = E[k] - w^k O[k]"""
    n = len(pts)
    if n == 1:
        return list(pts)
    ev = _point_fft(C, pts[0::2], omega * omega % R)
    od = _point_fft(C, pts[1::2], omega * omega % R)
    out = [None] * n
    for k in range(n // 2):
        t = mo.mul(C, od[k], pow(omega, k, R))
        out[k] = _add(C, ev[k], t)
        out[k + n // 2] = mo.sub(C, ev[k], t)
    return out


# ------------------------------------------------------------------ 1. against the oracle's point FFT
@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("group,n", [(1, 2), (1, 4), (1, 8), (2, 2), (2, 4), (2, 8)])
def test_against_the_oracle_point_fft(ctx, group, n, inverse):
    rng = random.Random(31 * n + group)
    C = _curve(group)
    pts = [_gen(group, rng.randrange(1, R)) for _ in range(n)]
    omega = _omega(n)
    if inverse:
        ninv = pow(n, -1, R)
        want = [mo.mul(C, p, ninv) for p in _point_fft(C, pts, pow(omega, -1, R))]
    else:
        want = _point_fft(C, pts, omega)
    got = _bases(ctx, group, pts).fft(inverse)
    assert len(got) == n and got.group == group
    assert got.to_bytes() == _enc(group, want)


# ------------------------------------------------------------------ 2. the Lagrange basis of tau^i G
def _lagrange(n, tau, j):
    """L_j(tau) = (tau^n - 1) omega^j / (n (tau - omega^j))"""
    wj = pow(_omega(n), j, R)
    return (pow(tau, n, R) - 1) * wj % R * pow(n * (tau - wj) % R, -1, R) % R


def _powers(ctx, group, n, tau):
    bh = _bh()
    gen = mo.g1_bytes(mo.GEN1) if group == 1 else mo.g2_bytes(mo.GEN2)
    return bh.Bases(ctx, group, gen * n, checked=False).mul_powers(1, tau)


@pytest.mark.parametrize("group,n", [(1, 512), (2, 64)])
def test_ifft_of_powers_is_the_lagrange_basis(ctx, group, n):
    x = _powers(ctx, group, n, TAU)
    lag = x.ifft()
    want = [_gen(group, _lagrange(n, TAU, j)) for j in range(n)]
    assert lag.read(0, n) == _enc(group, want)
    assert lag.fft().read(0, n) == x.read(0, n)


def test_one_stage_spans_two_chunks(ctx):
    n = 1 << 20
    x = _powers(ctx, 1, n, TAU)
    lag = x.ifft()
    assert lag.fft().read(0, n) == x.read(0, n)
    rng = random.Random(5)
    idx = [0, 1, n // 2 - 1, n // 2, n - 1] + [rng.randrange(n) for _ in range(11)]
    for j in idx:
        assert lag.get(j) == mo.g1_bytes(mo.g1(_lagrange(n, TAU, j))), j


# ------------------------------------------------------------------ 3. identities
def test_all_points_equal(ctx):
    assert _status(_powers(ctx, 1, 4, 1).fft) == UNEXPECTED_IDENTITY
    assert _status(_powers(ctx, 1, 4, 1).ifft) == UNEXPECTED_IDENTITY


@pytest.mark.parametrize("group", [1, 2])
def test_two_point_cases(ctx, group):
    C = _curve(group)
    p = _gen(group, 0x1234567)
    neg = C.to_affine(C.neg(C.from_affine(p)))
    assert _status(_bases(ctx, group, [p, neg]).fft) == UNEXPECTED_IDENTITY  # (O, 2P)
    assert _status(_bases(ctx, group, [p, p]).fft) == UNEXPECTED_IDENTITY    # the doubling case: (2P, O)
    q = mo.mul(C, p, 3)
    want = [mo.mul(C, p, 4), mo.mul(C, p, R - 2)]
    assert _bases(ctx, group, [p, q]).fft().to_bytes() == _enc(group, want)


# ------------------------------------------------------------------ 4. statuses
def test_statuses(ctx):
    bh = _bh()
    pts = [mo.g1(k) for k in (3, 5, 7)]
    assert _status(_bases(ctx, 1, pts).fft) == INVALID_ARGUMENT
    assert _status(_bases(ctx, 1, pts[:1]).fft) == INVALID_ARGUMENT
    assert _status(_bases(ctx, 1, pts).ifft) == INVALID_ARGUMENT
    import ctypes
    h = ctypes.c_void_p()
    lib = bh.lib()
    assert lib.bh_srs_fft(ctx.h, None, 0, ctypes.byref(h)) == INVALID_ARGUMENT
    assert lib.bh_srs_fft(None, _bases(ctx, 1, pts[:2]).h, 0, ctypes.byref(h)) == INVALID_ARGUMENT
    assert lib.bh_srs_fft(ctx.h, _bases(ctx, 1, pts[:2]).h, 0, None) == INVALID_ARGUMENT
    if bh.device_count() > 1:  # a handle from another context's device
        other = bh.Context(1)
        try:
            b = _bases(other, 1, pts[:2])
            assert lib.bh_srs_fft(ctx.h, b.h, 0, ctypes.byref(h)) == INVALID_ARGUMENT
            del b
        finally:
            other.close()


# ------------------------------------------------------------------ 5. scratch budget
def test_scratch_budget_counts_the_new_kernels(ctx):
    _bases(ctx, 2, [mo.g2(3), mo.g2(5)]).fft()
    rep = ctx.scratch_report()
    assert rep["fits"]
    # the 17 kernels of the transform and the matrix product (group_fft_kernels) on top of the 51
    # the list held before them
    assert rep["kernels_checked"] >= 51 + 17
