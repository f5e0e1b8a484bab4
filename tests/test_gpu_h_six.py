"""The six-transform H block (run_h_vector / run_h_final, csrc/api.hip) against the unchanged
ten-call path on the resident EvaluationDomain and against the oracle.

The fused pipeline drops c's coset round trip: h = icoset_fft(A o B / Z) - ifft(c) / Z
(tests/test_h_identity_cpu.py pins the identity on the oracle).  Every input here is random and
does NOT satisfy a*b = c, so h depends on c' = ifft(c)/Z in every coefficient.

Sizes: m = 1, 2 (launch_ntt's one-element branch, a one-stage pass), 4, 32, and the pass split of
launch_ntt (ceil(L / 10) passes of at most 10 stages): 2^10 is the largest one-pass size, 2^11
the smallest two-pass size, 2^21 the smallest three-pass size.

bh.compute_h goes through bh_compute_h, which runs run_h_final WITHOUT hout (h left
bit-reversed in the a|b|c buffer, permuted and downloaded by the caller): every case below
covers that path.  The path with hout (canonical scalars from the storing pass) is the one
bh_prove, bh_prove_witness and bh_compute_h_scalars use; the proof and h-scalars tests of
test_gpu_parity.py cover it."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
R_TOP = 0x73EDA753299D7D48  # r's top 64-bit limb: a top limb below it keeps the value below r

ONE_PASS_MAX, TWO_PASS_MIN, THREE_PASS_MIN = 1 << 10, 1 << 11, 1 << 21


def _bh():
    import bellman_hip as bh
    return bh


def _random_fr(rng, n):
    """(n,4) uint64 words of n field elements below r (bls12_381 Montgomery words: any value
    below r is one)."""
    x = rng.integers(0, 1 << 64, size=(n, 4), dtype=np.uint64)
    x[:, 3] = rng.integers(0, R_TOP, size=n, dtype=np.uint64)
    return x


def _abc(n, seed):
    rng = np.random.default_rng(seed)
    return tuple(_random_fr(rng, n) for _ in range(3))


def _h_fused(ctx, A, B, C):
    """bh_compute_h into an array (Montgomery words, canonical), as bench.py's domain_leg calls it."""
    bh = _bh()
    n = A.shape[0]
    m = ctypes.c_size_t()
    bh._check(bh._lib.bh_domain_size(n, ctypes.byref(m), None))
    h = np.zeros((max(m.value - 1, 1), 4), dtype=np.uint64)
    hl = ctypes.c_size_t()
    bh._check(bh._lib.bh_compute_h(ctx.h, bh._ptr(A), bh._ptr(B), bh._ptr(C), n, bh._ptr(h), ctypes.byref(hl)),
              "bh_compute_h")
    assert hl.value == m.value - 1
    return h[: hl.value]


def _h_resident(ctx, A, B, C):
    """The ten calls of prover.rs:210-231 on the resident EvaluationDomain (what
    bh.compute_h_resident issues), h read back as an array."""
    bh = _bh()
    da, db, dc = (bh.ResidentEvaluationDomain(ctx, x) for x in (A, B, C))
    try:
        for d in (da, db, dc):
            d.ifft()
            d.coset_fft()
        da.mul_assign(db)
        da.sub_assign(dc)
        da.divide_by_z_on_coset()
        da.icoset_fft()
        return da.as_mont(da.m - 1).copy()
    finally:
        for d in (da, db, dc):
            d.close()


def _h_oracle(A, B, C):
    bh = _bh()
    from oracle import bellman as bm
    E = bm.BLS12_381
    da, db, dc = (bm.EvaluationDomain(E, bh.fr_from_mont(x)) for x in (A, B, C))
    for d in (da, db, dc):
        d.ifft()
        d.coset_fft()
    da.mul_assign(db)
    da.sub_assign(dc)
    da.divide_by_z_on_coset()
    da.icoset_fft()
    return [int(v) for v in da.coeffs[: len(da.coeffs) - 1]]


def _unsatisfied(A, B, C):
    bh = _bh()
    k = min(A.shape[0], 4)
    a, b, c = (bh.fr_from_mont(x[:k]) for x in (A, B, C))
    return any(x * y % R != z for x, y, z in zip(a, b, c))


@pytest.mark.parametrize("m", [1, 2, 4, 32, ONE_PASS_MAX, TWO_PASS_MIN, THREE_PASS_MIN])
def test_compute_h_equals_ten_call_resident_path(ctx, m):
    bh = _bh()
    A, B, C = _abc(m, 600 + m.bit_length())
    assert _unsatisfied(A, B, C)
    got = _h_fused(ctx, A, B, C)
    want = _h_resident(ctx, A, B, C)
    assert got.shape == want.shape == (m - 1, 4)
    assert np.array_equal(got, want), (m, int(np.argmax((got != want).any(axis=1))))
    if m <= TWO_PASS_MIN:  # the public list-of-ints calls themselves (host conversion per element)
        h = bh.compute_h(ctx, A, B, C)
        assert h == bh.compute_h_resident(ctx, A, B, C)
        assert h == bh.fr_from_mont(got)
        if m <= ONE_PASS_MAX:
            assert h == _h_oracle(A, B, C)


@pytest.mark.parametrize("n", [TWO_PASS_MIN - 3, TWO_PASS_MIN // 2 + 1])
def test_compute_h_zero_padded_tail(ctx, n):
    """n < m: a, b, c are zero-padded to the domain (m = 2^11 for both n)."""
    bh = _bh()
    A, B, C = _abc(n, 700 + n)
    assert _unsatisfied(A, B, C)
    got = _h_fused(ctx, A, B, C)
    want = _h_resident(ctx, A, B, C)
    assert got.shape == want.shape == (TWO_PASS_MIN - 1, 4)
    assert np.array_equal(got, want), (n, int(np.argmax((got != want).any(axis=1))))
    # padding by hand gives the same h
    pad = lambda X: np.concatenate([X, np.zeros((TWO_PASS_MIN - n, 4), dtype=np.uint64)])
    assert np.array_equal(got, _h_fused(ctx, pad(A), pad(B), pad(C)))
    assert bh.compute_h(ctx, A, B, C) == bh.compute_h_resident(ctx, A, B, C)
