"""The distributed H kernels (csrc/dist_h.hip: k_gather_class, k_dist_mid<N>, k_dist_final<N> with
small_dft<N> and geometric<N>, and the host phases) on chosen inputs, rank by rank.

bh_selftest_dist_h runs the whole pipeline with N virtual ranks on one context and returns every
rank's hbuf and hidx as the kernels left them; bh_selftest_dist_stage runs one rank's k_dist_mid
(stage 0) or k_dist_final (stage 1) on packed words used exactly as given.  Everything is compared
with tests/dist_h_model.py (which tests/test_dist_h_model_cpu.py holds to the oracle), with the oracle
itself, or with bh_compute_h; field arithmetic is exact, so every assertion is an equality or an exact
bound.

Pipeline shapes: every rank count at its two smallest sizes (C = 2 and 4 elements per chunk: one
wave of k_dist_mid holds lanes of all three vectors, k_dist_final's grid is shorter than a wave),
C = 128 (3 C = 1.5 blocks), C = 256, a two-pass local NTT (M = 2^11) and 16 ranks at C = 256.  The
slot hidx marks -1 (k = m - 1, the coefficient create_proof drops) is checked against the model: it
is non-zero whenever a o b != c leaves a quotient of degree m - 1.

Stage operands: the contract's ends (0, 2r - 1, r and its neighbours) in chosen positions over the
source rank s, so that x[0], which geometric() never multiplies, and the first butterfly's
u + 2r - t sit at their extremes; values at or above 2r are outside the contract and never fed."""
import ctypes
import functools
import random

import numpy as np
import pytest

import dist_h_model as dm

pytestmark = pytest.mark.gpu

R = dm.R
RI = pow(1 << 261, -1, R)       # packed device words are Montgomery residues, radix 2^261
OK, INVALID = 0, 10


def _bh():
    import bellman_hip as bh
    return bh


def _lg(N):
    return N.bit_length() - 1


EDGE = [(N, 2 * _lg(N) + 1 + d) for N in (2, 4, 8, 16) for d in (0, 1)]
PIPELINE_SHAPES = EDGE + [(2, 9), (2, 10), (4, 12), (2, 12), (16, 16)]
ORACLE_MAX = 1 << 10            # above it the reference is bh_compute_h


# ------------------------------------------------------------------ words
def _words(values):
    """ints below 2^256 -> (n, 8) uint32, little endian"""
    raw = b"".join(int(v).to_bytes(32, "little") for v in values)
    return np.frombuffer(raw, dtype=np.uint32).reshape(-1, 8).copy()


def _ints(words):
    raw = np.ascontiguousarray(words, dtype=np.uint32).tobytes()
    return [int.from_bytes(raw[i:i + 32], "little") for i in range(0, len(raw), 32)]


def _not_below(words, bound):
    """indices of the (n, 8) uint32 values that are >= bound, compared limb by limb from the top"""
    w = np.ascontiguousarray(words, dtype=np.uint32).reshape(-1, 8)
    lim = _words([bound])[0]
    less = np.zeros(len(w), dtype=bool)
    decided = np.zeros(len(w), dtype=bool)
    for i in range(7, -1, -1):
        less |= ~decided & (w[:, i] < lim[i])
        decided |= w[:, i] != lim[i]
    return np.flatnonzero(~less)


def _where(sh, rank, slot):
    t, u = divmod(int(slot), sh.C)
    return "N=%d L=%d rank=%d t=%d u=%d" % (sh.N, sh.L, rank, t, u)


# ------------------------------------------------------------------ the entry points
def _pipeline(ctx, A, B, C, N, h=None, idx=None):
    """bh_selftest_dist_h -> (status, hbuf words (N, M, 8), hidx (N, M))"""
    f = _bh().lib().bh_selftest_dist_h
    f.restype = ctypes.c_int
    f.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int,
                  ctypes.c_void_p, ctypes.c_void_p]
    m = next(x for x in (A, B, C) if x is not None).shape[0]
    M = max(m // max(N, 1), 1)
    h = np.full((max(N, 1), M, 8), 0xFFFFFFFF, dtype=np.uint32) if h is None else h
    idx = np.full((max(N, 1), M), -7, dtype=np.int32) if idx is None else idx
    ptr = lambda x: None if x is None or x is False else x.ctypes.data
    st = f(ctx.h, ptr(A), ptr(B), ptr(C), m, N, ptr(h), ptr(idx))
    return st, h, idx


def _stage(ctx, L, N, rank, stage, recv, cprime, out=None, out2=None):
    """bh_selftest_dist_stage -> (status, out, out2); False for a buffer passes a null pointer"""
    f = _bh().lib().bh_selftest_dist_stage
    f.restype = ctypes.c_int
    f.argtypes = [ctypes.c_void_p] + [ctypes.c_int] * 4 + [ctypes.c_void_p] * 4
    M = max((1 << L) // max(N, 1), 1)
    if out is None:
        out = np.full((2 * M if stage == 0 else M, 8), 0xFFFFFFFF, dtype=np.uint32)
    if out2 is None:
        out2 = np.full((M, 8), 0xFFFFFFFF, dtype=np.uint32) if stage == 0 else np.full(M, -7, dtype=np.int32)
    ptr = lambda x: None if x is None or x is False else x.ctypes.data
    st = f(ctx.h, L, N, rank, stage, ptr(recv), ptr(cprime), ptr(out), ptr(out2))
    return st, out, out2


# ------------------------------------------------------------------ pipeline
@functools.lru_cache(maxsize=None)
def _case(m, kind):
    """inputs of one kind at size m, shared by every rank count of that size: ints, the library's
    Montgomery words, and the model's coefficient at k = m - 1"""
    rng = random.Random("%d %s" % (m, kind))
    if kind.startswith("onehot"):
        _, i, j = kind.split(":")
        a, b, c = dm.one_hot_inputs(m, int(i), int(j), rng)
    else:
        a, b, c = dm.make_inputs(kind, m, rng)
    mont = tuple(_bh().fr_to_mont(x) for x in (a, b, c))
    return (a, b, c), mont, dm.top_coefficient(a, b, c)


@functools.lru_cache(maxsize=None)
def _reference(ctx, m, kind):
    """h[0 .. m - 2] as canonical words (m - 1, 8): the oracle's up to 2^10, bh_compute_h's above"""
    bh = _bh()
    (a, b, c), (A, B, C), _ = _case(m, kind)
    if m <= ORACLE_MAX:
        from oracle import bellman as bm
        E = bm.BLS12_381
        da, db, dc = (bm.EvaluationDomain(E, list(x)) for x in (a, b, c))
        for d in (da, db, dc):
            d.ifft()
            d.coset_fft()
        da.mul_assign(db)
        da.sub_assign(dc)
        da.divide_by_z_on_coset()
        da.icoset_fft()
        h = [int(v) for v in da.coeffs[:m - 1]]
    else:
        out = np.zeros((m - 1, 4), dtype=np.uint64)
        hl = ctypes.c_size_t()
        bh._check(bh._lib.bh_compute_h(ctx.h, bh._ptr(A), bh._ptr(B), bh._ptr(C), m, bh._ptr(out), ctypes.byref(hl)),
                  "bh_compute_h")
        assert hl.value == m - 1
        h = bh.fr_from_mont(out)
    return _words(h)


def _check_pipeline(ctx, N, L, kind):
    sh = dm.Shape(N, L)
    m, M, C = sh.m, sh.M, sh.C
    _, (A, B, Cc), top = _case(m, kind)
    st, h, idx = _pipeline(ctx, A, B, Cc, N)
    assert st == OK, (N, L, kind, st)
    # hidx[rank][t C + u] == t M + rank C + u, except one -1 at the last rank's last slot
    slot = np.arange(M, dtype=np.int64)
    want = (slot // C * M + slot % C)[None, :] + (np.arange(N, dtype=np.int64) * C)[:, None]
    want[N - 1, M - 1] = -1
    bad = np.argwhere(idx != want)
    assert len(bad) == 0, ("hidx", kind, _where(sh, *bad[0]), int(idx[tuple(bad[0])]))
    # the non-negative indices over all ranks are exactly 0 .. m - 2, each once
    flat = idx.ravel()
    assert np.array_equal(np.sort(flat[flat >= 0]), np.arange(m - 1)) and int((flat == -1).sum()) == 1, (N, L, kind)
    # every scalar is canonical
    bad = _not_below(h, R)
    assert len(bad) == 0, ("scalar >= r", kind, _where(sh, *divmod(int(bad[0]), M)))
    # h by index equals the reference
    hw = h.reshape(-1, 8)
    by_k = np.zeros((m, 8), dtype=np.uint32)
    by_k[np.where(flat < 0, m - 1, flat)] = hw
    ref = _reference(ctx, m, kind)
    bad = np.flatnonzero((by_k[:m - 1] != ref).any(axis=1))
    if len(bad):
        k = int(bad[0])
        rank, slot_k = divmod(int(np.flatnonzero(flat == k)[0]), M)
        raise AssertionError(("h differs at k=%d" % k, kind, _where(sh, rank, slot_k), len(bad)))
    # the coefficient at k = m - 1, in the slot marked -1
    got_top = _ints(h[N - 1, M - 1])[0]
    assert got_top == top, ("h[m - 1]", kind, _where(sh, N - 1, M - 1), hex(got_top), hex(top))
    return got_top


@pytest.mark.parametrize("kind", dm.INPUT_KINDS)
@pytest.mark.parametrize("N,L", PIPELINE_SHAPES)
def test_pipeline_rank_by_rank(ctx, N, L, kind):
    top = _check_pipeline(ctx, N, L, kind)
    # a quotient of degree m - 1 (a o b != c) leaves a non-zero coefficient the proofs never show;
    # a satisfied witness, and a = b = c = r - 1 (constants: a b - c = 2), leave zero
    assert (top != 0) == (kind in ("random", "c_only", "c_zero")), (N, L, kind, hex(top))


@pytest.mark.parametrize("pos", ["0", "1", "N-1", "N", "m-1"])
@pytest.mark.parametrize("N,L", EDGE)
def test_pipeline_one_hot(ctx, N, L, pos):
    """a is one-hot at `pos`, b random, c one-hot at another index: every residue class but one
    gathers zeros, and the hot element sits on a chunk's or the domain's edge"""
    m = 1 << L
    i = {"0": 0, "1": 1, "N-1": N - 1, "N": N, "m-1": m - 1}[pos]
    j = (i + m // 2 + 1) % m
    _check_pipeline(ctx, N, L, "onehot:%d:%d" % (i, j))


# ------------------------------------------------------------------ stages
TWO_R = 2 * R
HI = TWO_R - 1
N_RANDOM = 4
# a pattern gives lane u's value for every source rank s
PATTERNS = [
    lambda s, rng: HI,                              # all 2r - 1
    lambda s, rng: 0,                               # all 0
    lambda s, rng: HI if s & 1 else 0,              # alternating, both phases
    lambda s, rng: 0 if s & 1 else HI,
    lambda s, rng: HI if s == 0 else 0,             # only x[0], which geometric() passes through
    lambda s, rng: 0 if s == 0 else HI,
    lambda s, rng: (R - 1, R, R + 1)[s % 3],        # r's neighbours in rotation
    lambda s, rng: (R + 1, R - 1, R)[s % 3],
] + [lambda s, rng: rng.randrange(TWO_R)] * N_RANDOM
P = len(PATTERNS)
# c' for stage 1, per slot: the contract's ends and r's neighbours, then random
CPRIME = [lambda rng: 0, lambda rng: R, lambda rng: HI, lambda rng: R - 1, lambda rng: R + 1, lambda rng: 1,
          lambda rng: rng.randrange(TWO_R)]
STAGE_SHAPES = [(N, 2 * _lg(N) + 1) for N in (2, 4, 8, 16)] + [(N, 2 * _lg(N) + 4) for N in (2, 4, 8, 16)]


def _ranks(N):
    return sorted({0, 1, N - 1})


def _column(pattern, N, rng):
    col = [PATTERNS[pattern](s, rng) for s in range(N)]
    assert all(0 <= v < TWO_R for v in col)
    return col


@pytest.mark.parametrize("N,L", STAGE_SHAPES)
def test_stage0_keeps_the_bound_and_the_residue(ctx, N, L):
    """k_dist_mid: every word string it stores (a's and b's rows, c') is below 2r, the bound the
    next phase's loads rely on, and congruent to the model mod r.  Lane u of launch `rnd` takes
    pattern (u + rnd C) mod P for a, shifted by 3 and 7 for b and c, so a wave's lanes of the three
    vectors differ and every pattern reaches every vector."""
    sh = dm.Shape(N, L)
    M, C = sh.M, sh.C
    assert C == (2 if L == 2 * _lg(N) + 1 else 16)
    rng = random.Random(100 * N + L)
    for rank in _ranks(N):
        for rnd in range(-(-P // C)):
            recv = [None] * (3 * M)
            for vec in range(3):
                for u in range(C):
                    col = _column((u + rnd * C + (0, 3, 7)[vec]) % P, N, rng)
                    for s in range(N):
                        recv[vec * M + s * C + u] = col[s]
            st, out, cp = _stage(ctx, L, N, rank, 0, _words(recv), None)
            assert st == OK
            want_out, want_cp = dm.stage0(sh, rank, recv)
            for name, words, want in (("out", out, want_out), ("cprime", cp, want_cp)):
                bad = _not_below(words, TWO_R)
                assert len(bad) == 0, (name + " >= 2r", rnd, "vec=%d" % (bad[0] // M), _where(sh, rank, bad[0] % M))
                got = _ints(words)
                for i, (g, w) in enumerate(zip(got, want)):
                    # the row index d of `out` stands where t does in the message
                    assert g % R == w, (name, rnd, "vec=%d" % (i // M), _where(sh, rank, i % M), hex(g))


@pytest.mark.parametrize("N,L", STAGE_SHAPES)
def test_stage1_is_canonical_and_exact(ctx, N, L):
    """k_dist_final: hbuf is the model's value exactly (so below r) and hidx the slot's global
    index.  Every pattern meets every c' choice: lane configurations (pattern, c') are dealt to the
    lanes launch after launch; c' rotates with t inside a lane, so c' = 0, r and 2r - 1 meet both
    v = 0 (the all-zero pattern) and large v."""
    sh = dm.Shape(N, L)
    M, C = sh.M, sh.C
    rng = random.Random(200 * N + L)
    configs = [(p, k) for p in range(P) for k in range(len(CPRIME))]
    for rank in _ranks(N):
        for first in range(0, len(configs), C):
            recv, cprime = [0] * M, [0] * M
            for u in range(C):
                p, k = configs[(first + u) % len(configs)]
                col = _column(p, N, rng)
                for s in range(N):
                    recv[s * C + u] = col[s]
                for t in range(N):
                    cprime[t * C + u] = CPRIME[(k + t) % len(CPRIME)](rng)
            assert all(0 <= v < TWO_R for v in cprime)
            st, hbuf, hidx = _stage(ctx, L, N, rank, 1, _words(recv), _words(cprime))
            assert st == OK
            want_h, want_idx = dm.stage1(sh, rank, recv, cprime)
            got = _ints(hbuf)
            for slot in range(M):
                # the model is linear: on the raw words it gives 2^261 times the scalar
                assert got[slot] == want_h[slot] * RI % R, ("hbuf", first, _where(sh, rank, slot), hex(got[slot]))
                assert got[slot] < R
                assert int(hidx[slot]) == want_idx[slot], ("hidx", first, _where(sh, rank, slot), int(hidx[slot]))
            assert (np.asarray(want_idx) == -1).sum() == (1 if rank == N - 1 else 0)


def test_stage_patterns_cover_what_they_claim():
    rng = random.Random(0)
    cols = [_column(p, 4, rng) for p in range(P)]
    assert [HI] * 4 in cols and [0] * 4 in cols and [0, HI, 0, HI] in cols and [HI, 0, HI, 0] in cols
    assert [HI, 0, 0, 0] in cols and [0, HI, HI, HI] in cols and [R - 1, R, R + 1, R - 1] in cols
    assert sum(1 for c in cols if len(set(c)) == 4 and not set(c) & {0, HI, R - 1, R, R + 1}) >= 4
    assert {f(rng) for f in CPRIME[:3]} == {0, R, HI}


# ------------------------------------------------------------------ statuses
def test_invalid_arguments_and_scratch_budget(ctx):
    bh = _bh()
    z = lambda m: np.zeros((m, 4), dtype=np.uint64)
    w = lambda n: np.zeros((n, 8), dtype=np.uint32)
    # rank counts that are not 2, 4, 8 or 16
    for N in (1, 3, 32):
        m = 1 << 12
        assert _pipeline(ctx, z(m), z(m), z(m), N)[0] == INVALID, N
        for stage in (0, 1):
            assert _stage(ctx, 12, N, 0, stage, w(3 * m), w(m))[0] == INVALID, (N, stage)
    for N in (2, 4, 8, 16):
        L = 2 * _lg(N)          # one element per chunk: not eligible
        m, M = 1 << L, (1 << L) // N
        assert _pipeline(ctx, z(m), z(m), z(m), N)[0] == INVALID, N
        assert _pipeline(ctx, z(m + 1), z(m + 1), z(m + 1), N)[0] == INVALID, N     # m not a power of two
        for stage in (0, 1):
            assert _stage(ctx, L, N, 0, stage, w(3 * M), w(M))[0] == INVALID, (N, stage)
            # eligible (L + 1), but the rank or the stage is not
            assert _stage(ctx, L + 1, N, N, stage, w(6 * M), w(2 * M))[0] == INVALID, (N, stage)
            assert _stage(ctx, L + 1, N, -1, stage, w(6 * M), w(2 * M))[0] == INVALID, (N, stage)
        assert _stage(ctx, L + 1, N, 0, 2, w(6 * M), w(2 * M))[0] == INVALID, N
        assert _stage(ctx, L + 1, N, 0, -1, w(6 * M), w(2 * M))[0] == INVALID, N
    # null buffers
    m, M = 1 << 5, 1 << 4
    for k in range(3):
        abc = [z(m), z(m), z(m)]
        abc[k] = None
        assert _pipeline(ctx, abc[0], abc[1], abc[2], 2)[0] == INVALID, k
    assert _pipeline(ctx, z(m), z(m), z(m), 2, h=False)[0] == INVALID
    assert _pipeline(ctx, z(m), z(m), z(m), 2, idx=False)[0] == INVALID
    for stage in (0, 1):
        assert _stage(ctx, 5, 2, 0, stage, None, w(M))[0] == INVALID
        assert _stage(ctx, 5, 2, 0, stage, w(3 * M), w(M), out=False)[0] == INVALID
        assert _stage(ctx, 5, 2, 0, stage, w(3 * M), w(M), out2=False)[0] == INVALID
    assert _stage(ctx, 5, 2, 0, 1, w(M), None)[0] == INVALID      # stage 1 reads cprime; stage 0 does not
    assert _stage(ctx, 5, 2, 0, 0, w(3 * M), None)[0] == OK
    f = bh.lib().bh_selftest_dist_stage
    assert f(None, 5, 2, 0, 0, w(3 * M).ctypes.data, None, w(2 * M).ctypes.data, w(M).ctypes.data) == INVALID
    # the self-tests launch kernels the scratch budget already lists: it still fits
    assert ctx.scratch_report()["fits"]
