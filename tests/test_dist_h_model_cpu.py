"""tests/dist_h_model.py (the integer model of csrc/dist_h.hip that tests/test_gpu_dist_h.py holds
the kernels to) against oracle/bellman.py's compute_h, at the two smallest eligible sizes of every
rank count: C = 2 and C = 4 elements per chunk.  No GPU.

The oracle truncates h to m - 1 coefficients; the model keeps the one at k = m - 1 (the device writes
it into the slot hidx marks -1), which top_coefficient restates directly from the polynomials."""
import random

import pytest

import dist_h_model as dm

SHAPES = [(N, 2 * (N.bit_length() - 1) + 1 + d) for N in (2, 4, 8, 16) for d in (0, 1)]
KINDS = ("random", "satisfied", "all_r_minus_1", "c_only", "c_zero")


def _oracle_h(a, b, c):
    from oracle import bellman as bm
    return [int(v) for v in bm.compute_h(bm.BLS12_381, a, b, c)]


@pytest.mark.parametrize("N,L", SHAPES)
def test_pipeline_equals_the_oracle_and_its_stages_chain(N, L):
    sh = dm.Shape(N, L)
    assert (sh.m, sh.C) == (1 << L, 2 << (L - 2 * (N.bit_length() - 1) - 1))
    rng = random.Random(1000 * N + L)
    for kind in KINDS:
        a, b, c = dm.make_inputs(kind, sh.m, rng)
        trace = {}
        shares = dm.pipeline(sh, a, b, c, trace)
        h = dm.assemble(sh, shares)
        assert h[:sh.m - 1] == _oracle_h(a, b, c), (N, L, kind)
        # the coefficient the oracle drops: zero exactly when the quotient has degree m - 2
        top = dm.top_coefficient(a, b, c)
        assert h[sh.m - 1] == top, (N, L, kind)
        assert (top != 0) == (kind in ("random", "c_only", "c_zero")), (N, L, kind)
        # each stage alone, on the pipeline's own intermediate buffers, gives the pipeline's result
        for r in range(N):
            out, cprime = dm.stage0(sh, r, trace["recv1"][r])
            assert out == trace["out"][r][:2 * sh.M] and cprime == trace["cprime"][r], (N, L, kind, r)
            assert dm.stage1(sh, r, trace["recv3"][r], cprime) == shares[r], (N, L, kind, r)
        if kind == "c_only":            # h = -c' in every slot
            for r in range(N):
                assert shares[r][0] == [(-v) % dm.R for v in trace["cprime"][r]], (N, L, r)


@pytest.mark.parametrize("N,L", SHAPES + [(2, 9), (4, 12), (16, 16)])
def test_index_sets_partition_the_domain(N, L):
    sh = dm.Shape(N, L)
    seen = bytearray(sh.m)
    for r in range(N):
        for slot in range(sh.M):
            k = dm.index_of(sh, r, slot)
            assert 0 <= k < sh.m and not seen[k], (N, L, r, slot)
            seen[k] = 1
    assert all(seen)
    # k = m - 1 is the last rank's last slot
    assert dm.index_of(sh, N - 1, sh.M - 1) == sh.m - 1


def test_hidx_marks_only_the_last_ranks_last_slot():
    sh = dm.Shape(4, 5)
    zero = [0] * sh.M
    for r in range(sh.N):
        _, hidx = dm.stage1(sh, r, zero, zero)
        want = [dm.index_of(sh, r, s) for s in range(sh.M)]
        if r == sh.N - 1:
            want[-1] = -1
        assert hidx == want


def test_eligibility_is_the_devices():
    for N in range(0, 40):
        for L in range(0, 12):
            pow2 = N in (2, 4, 8, 16)
            assert dm.eligible(N, L) == (pow2 and (1 << L) // (N * N) >= 2), (N, L)


def test_ifft_inverts_evaluation():
    rng = random.Random(5)
    for L in (0, 1, 3, 6):
        n = 1 << L
        coeffs = [rng.randrange(dm.R) for _ in range(n)]
        w = pow(dm.ROOT_OF_UNITY, 1 << (32 - L), dm.R)
        assert dm.ifft(dm.dft(coeffs, w)) == coeffs
