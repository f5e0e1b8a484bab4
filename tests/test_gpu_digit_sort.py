"""The layer between a caller's scalars and the accumulation kernels, against tests/digit_sort_model.py.

csrc/selftest.hip drives the host functions of msm.h unchanged on host arrays: sort_entries +
max_span (bh_selftest_digit_sort), derive_sorted (bh_selftest_derive_sorted), exclusive_scan and
its device-bounded form (bh_selftest_scan), scalars_prepare and density_index.  Every output starts
as 0xFF bytes and every comparison is exact: counts, offsets (with offsets[nbt] and a shard's
offsets[bk_hi]), each bucket's entries as a multiset (the order inside a bucket comes from LDS
atomics), the entries past offsets[nbt], and the maximum of the span words.

Scalars (digit_sort_model.patterns, per c, then random ones): every window raw 2^(c-1), every
window 2^(c-1) + 1, the two alternating around 2^(c-1), all ones, 0, 1, r - 1, r - 2.  The test
asserts from the model that a digit of exactly +2^(c-1), a zero digit that carries out and (where
c does not divide 32: for c = 2, 4, 8, 16 no window crosses a word) a window across two 32-bit
words with a carry coming in all occur in every vector of 255 scalars or more.

Geometry of the shapes (W windows, NB = 2^(c-1), nbt buckets, P partitions of `bins` buckets):

  plain  c   W    NB     nbt      P     bins   what it is the smallest case of
         2   128  2      256      256   1      most windows; every window crosses no word
         4   64   8      512      512   1
         8   32   128    4096     4096  1      nbt = 4096: the last shape with one bucket per partition
         9   29   256    7424     3712  2      lo_bits 1; nbt no multiple of a power of two
         13  20   4096   81920    2560  32     windows across words; P < 4096
         16  16   32768  524288   4096  128    P = 4096 with 128 bins
  table  13  20   4096   4096     4096  1      nbt = 4096 with shared buckets
         14  19   8192   8192     4096  2
         16  16   32768  32768    4096  8      shards of 1024 buckets = 128 partitions
         20  13   2^19   2^19     4096  128    the 2^22 prover's window
         22  12   2^21   2^21     4096  512    (not reachable through bh_ctx_set_window)
         24  11   2^23   2^23     4096  2048   2048 bins; the shard granule is the partition width

n = 1, 255, 4095, 4096, 4097 and 3 * 4096 + 17 put the tile edges of the 4096-scalar tiles and
several tiles per partition under each shape; index maps have about half density, -1 runs over
two whole 256-thread strides and over a whole tile, and base indices in no order.

For a bucket shard the library writes counts[b] for bk_lo <= b < bk_hi and offsets[b] for
bk_lo <= b <= bk_hi and b = nbt, counted from offsets[bk_lo] = 0, and nothing else: the other
words keep their 0xFF fill.  That is what the code does, pinned here; the consumers read only
the shard's range.

Scalar preparation, mode 2: fe_from_mont of the packed value r is exactly r (r + (2^261 - 1) r =
2^261 r), the one input below 2r for which the conditional subtraction after it acts; the test
asserts this from the model and includes it.
"""
import ctypes
import functools
import random

import numpy as np
import pytest

import digit_sort_model as m

pytestmark = pytest.mark.gpu

INVALID = 10                       # BH_ERR_INVALID_ARGUMENT
FF = m.UNSET
NS = [1, 255, 4095, 4096, 4097, 3 * 4096 + 17]
PLAIN_C = [2, 4, 8, 9, 13, 16]
TABLE_C = [13, 14, 16, 20]
SORT_CASES = ([(0, c, n) for c in PLAIN_C for n in NS] + [(1, c, n) for c in TABLE_C for n in NS]
              + [(1, 22, 4097), (1, 24, 4097)])
MAX_SPAN_BLOCKS = 256


@functools.lru_cache(maxsize=None)
def _lib():
    import bellman_hip as bh
    lib = bh.lib()
    I, U, S, P, L = ctypes.c_int, ctypes.c_uint32, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_int64
    for name, args in {
        "bh_selftest_digit_sort": [I, P, S, P, U, I, I, U, U, U, P, P, P, P, P],
        "bh_selftest_derive_sorted": [I, P, S, P, S, I, U, U, P, S, S, S, P, P, P],
        "bh_selftest_scan": [I, P, S, L, P],
        "bh_selftest_scalars_prepare": [I, P, S, I, I, P],
        "bh_selftest_density_index": [I, P, S, U, P],
    }.items():
        f = getattr(lib, name)
        f.restype, f.argtypes = I, args
    return lib


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


class Run:
    pass


def device_sort(words, idx, base_offset, c, pre, S, bk_lo=0, bk_hi=0, fill=0):
    """bh_selftest_digit_sort -> a Run (status, entries, counts, offsets, span words)"""
    n = words.shape[0]
    W, NB, Wb, nbt = m.geometry(max(c, 2), pre) if 2 <= c <= 24 else (1, 1, 1, 1)
    r = Run()
    r.fill = fill
    r.entries = np.full(max(n * W, 1), fill, dtype=np.uint32)
    r.counts = np.full(nbt, fill, dtype=np.uint32)
    r.offsets = np.full(nbt + 1, fill, dtype=np.uint32)
    span = np.full(MAX_SPAN_BLOCKS, fill, dtype=np.uint32)
    nspan = ctypes.c_uint32(0)
    words = np.ascontiguousarray(words, dtype=np.uint32)
    idx32 = None if idx is None else np.ascontiguousarray(idx, dtype=np.int32)
    r.status = _lib().bh_selftest_digit_sort(0, _p(words), n, _p(idx32), base_offset, c, pre, bk_lo, bk_hi, S,
                                             _p(r.entries), _p(r.counts), _p(r.offsets), _p(span),
                                             ctypes.byref(nspan))
    r.entries = r.entries[:n * W]
    r.span, r.span_all = span[:nspan.value], span
    return r


def check_sort(r, want, c, pre, S, entries=True):
    """a Run against the model's Sorted, everything the device returned"""
    W, NB, Wb, nbt = m.geometry(c, pre)
    assert r.status == 0
    lo, hi = np.flatnonzero(want.written_counts)[[0, -1]] + [0, 1]
    total = want.total
    assert (r.counts[lo:hi] == want.counts[lo:hi]).all()
    assert (r.offsets[lo:hi + 1] == want.offsets[lo:hi + 1]).all()
    assert r.offsets[nbt] == total and r.offsets[lo] == 0 and r.offsets[hi] == total
    assert (r.counts[~want.written_counts] == FF).all() and (r.offsets[~want.written_offsets] == FF).all()
    if entries:
        bucket, entry = m.by_bucket(r.entries, r.offsets, lo, hi)
        assert len(entry) == total and (bucket == want.bucket).all() and (entry == want.entry).all()
        assert (r.entries[total:] == FF).all()
    assert len(r.span) == min(MAX_SPAN_BLOCKS, max(1, (hi - lo + 255) // 256))
    assert int(r.span.max()) == m.span_model(want.counts[lo:hi], want.offsets[lo:hi], S)
    assert (r.span_all[len(r.span):] == r.fill).all()      # (the host array's own fill: not written)


@functools.lru_cache(maxsize=None)
def _words(c, n):
    w = m.to_words(m.scalar_vector(c, n, random.Random(100 * c + n)))
    w.setflags(write=False)
    return w


def _index_map(n, W, seed):
    """about half the scalars present, the chosen patterns among them; absent runs over two whole
    256-thread strides and over the second tile; base indices a random injection"""
    rng = np.random.RandomState(seed)
    present = rng.random_sample(n) < 0.5
    present[:8] = True
    present[256:768] = False
    present[4096:8192] = False
    M = min(4 * n + 16, (1 << 31) // W)
    return np.where(present, rng.permutation(M)[:n], -1).astype(np.int32)


def _assert_classes(words, c, rows=None):
    """the conditions the chosen scalars exist for, read from the model's digits"""
    d, cin, cout = m.digits_array(words if rows is None else words[rows], c)
    W, half = d.shape[1], 1 << (c - 1)
    assert (cout == 0).all()
    assert (d == half).any(), "no digit of exactly +2^(c-1)"
    assert ((d == 0) & (cin == 1)).any(), "no zero digit that carries out"
    if 32 % c:
        straddle = np.array([(w * c) // 32 != (w * c + c - 1) // 32 for w in range(W)])
        assert (cin[:, straddle] == 1).any(), "no carry into a window across two words"


@pytest.mark.parametrize("pre,c,n", SORT_CASES)
def test_digit_sort(pre, c, n):
    words = _words(c, n)
    W, NB, Wb, nbt = m.geometry(c, pre)
    # without a map, base indices from 7: S = 3 in full, S = 256 for its span words
    want = m.sort_model(words, None, 7, c, pre)
    check_sort(device_sort(words, None, 7, c, pre, 3), want, c, pre, 3)
    check_sort(device_sort(words, None, 7, c, pre, 256), want, c, pre, 256, entries=False)
    # through an index map: S = 16
    idx = _index_map(n, W, 7 * c + n)
    wanti = m.sort_model(words, idx, 0, c, pre)
    check_sort(device_sort(words, idx, 0, c, pre, 16), wanti, c, pre, 16)
    if n >= 255:
        _assert_classes(words, c)
        _assert_classes(words, c, idx >= 0)
        for s, S in ((want, 3), (wanti, 16)):
            off, cnt = s.offsets[:nbt].astype(np.int64), s.counts.astype(np.int64)
            assert ((cnt > 0) & ((off + cnt) % S == 0)).any(), "no bucket ends on a segment boundary"
            assert ((cnt > 0) & (off > 0) & (off % S == 0)).any(), "no bucket starts on a segment boundary"
    if n > 4096:
        assert (idx[4096:min(n, 8192)] == -1).all() and (idx[256:768] == -1).all()


def test_digit_sort_of_nothing():
    words = np.zeros((0, 8), dtype=np.uint32)
    r = device_sort(words, None, 0, 13, 1, 16, fill=FF)
    assert r.status == 0 and (r.counts == 0).all() and (r.offsets == 0).all() and (r.span == 0).all()
    # scalars that are all zero or all absent have no entries either
    words = np.zeros((300, 8), dtype=np.uint32)
    check_sort(device_sort(words, None, 0, 8, 0, 3), m.sort_model(words, None, 0, 8, 0), 8, 0, 3)
    idx = np.full(4097, -1, dtype=np.int32)
    check_sort(device_sort(_words(13, 4097), idx, 0, 13, 1, 3), m.sort_model(_words(13, 4097), idx, 0, 13, 1), 13, 1, 3)


@pytest.mark.parametrize("pre,c", [(0, 8), (0, 13), (1, 13), (1, 16)])
def test_one_scalar_repeated(pre, c):
    """one bucket per window takes every entry: 4100 of them, more than a tile and than the
    partition's 256-thread strides"""
    k = random.Random(c).randrange(m.R)
    words = np.repeat(m.to_words([k]), 4100, axis=0)
    want = m.sort_model(words, None, 3, c, pre)
    assert want.counts.max() >= 4100
    check_sort(device_sort(words, None, 3, c, pre, 16), want, c, pre, 16)
    assert m.span_model(want.counts, want.offsets, 16) >= 4100 // 16


def _granule(c):
    return max(1024, (1 << (c - 1)) >> 12)


@pytest.mark.parametrize("c,N", [(c, N) for c in (16, 20, 24) for N in (2, 3, 8)])
def test_bucket_shards(c, N):
    n = 4097
    words = _words(c, n)
    W, NB, Wb, nbt = m.geometry(c, 1)
    G = _granule(c)
    bounds = [(NB * k // N) // G * G for k in range(N + 1)]
    assert bounds[0] == 0 and bounds[-1] == NB and all(a < b for a, b in zip(bounds, bounds[1:]))
    full = m.sort_model(words, None, 0, c, 1)
    total = 0
    for lo, hi in zip(bounds, bounds[1:]):
        want = m.sort_model(words, None, 0, c, 1, lo, hi)
        assert (want.counts[lo:hi] == full.counts[lo:hi]).all()
        check_sort(device_sort(words, None, 0, c, 1, 16, lo, hi), want, c, 1, 16)
        total += want.total
    assert total == full.total


@pytest.mark.parametrize("c", [16, 20, 24])
def test_empty_bucket_shard(c):
    """a shard into whose range no digit falls: zero counts and offsets over the range"""
    words = _words(c, 3)
    G, NB = _granule(c), 1 << (c - 1)
    full = m.sort_model(words, None, 0, c, 1)
    empty = [g for g in range(1, NB // G - 1) if not full.counts[g * G:(g + 1) * G].any()]
    assert empty
    lo = empty[0] * G
    want = m.sort_model(words, None, 0, c, 1, lo, lo + G)
    assert want.total == 0
    r = device_sort(words, None, 0, c, 1, 3, lo, lo + G)
    check_sort(r, want, c, 1, 3)
    assert (r.counts[lo:lo + G] == 0).all() and (r.offsets[lo:lo + G + 1] == 0).all() and (r.entries == FF).all()


# ------------------------------------------------------------------ derived sorts
def device_derive(src, nbt, pre, W, src_off, idx, b0, b1, Emax, fill=0):
    r = Run()
    r.entries = np.full(Emax, fill, dtype=np.uint32)
    r.counts = np.full(nbt, fill, dtype=np.uint32)
    r.offsets = np.full(nbt + 1, fill, dtype=np.uint32)
    se = np.ascontiguousarray(src.entries, dtype=np.uint32)
    so = np.ascontiguousarray(src.offsets, dtype=np.uint32)
    idx32 = np.ascontiguousarray(idx, dtype=np.int32)
    assert len(se) == Emax
    r.status = _lib().bh_selftest_derive_sorted(0, _p(se), Emax, _p(so), nbt, pre, W, src_off, _p(idx32), len(idx32),
                                                b0, b1, _p(r.entries), _p(r.counts), _p(r.offsets))
    return r


def _derive_maps(n, W, seed):
    rng = np.random.RandomState(seed)
    M = min(4 * n + 16, (1 << 31) // W)
    perm = rng.permutation(M)[:n].astype(np.int32)
    none = np.full(n, -1, dtype=np.int32)
    first, last = none.copy(), none.copy()
    first[0], last[n - 1] = 11, 5
    return {"half": _index_map(n, W, seed + 1), "all": perm, "none": none, "first": first, "last": last}


@pytest.mark.parametrize("pre,c,shard", [(0, 9, None), (0, 2, None), (1, 13, None), (1, 16, None),
                                         (1, 16, (3 * 1024, 20 * 1024)), (1, 20, (0, 1024 * 100))],
                         ids=["plain-9", "plain-2", "table-13", "table-16", "table-16-shard", "table-20-shard"])
def test_derived_sort(pre, c, shard):
    n, src_off = 4097, 1000
    words = _words(c, n)
    W, NB, Wb, nbt = m.geometry(c, pre)
    lo, hi = shard or (0, 0)
    src = device_sort(words, None, src_off, c, pre, 16, lo, hi)
    check_sort(src, m.sort_model(words, None, src_off, c, pre, lo, hi), c, pre, 16)
    Emax = n * W
    for name, idx in _derive_maps(n, W, c).items():
        ent, cnt, off = m.derive_model(src.entries, src.offsets, nbt, idx, pre, W, src_off, lo, hi)
        r = device_derive(src, nbt, pre, W, src_off, idx, lo, hi, Emax)
        assert r.status == 0, name
        # the stable compaction of that source array, element for element; nothing written past it
        assert (r.entries[:len(ent)] == ent).all() and (r.entries[len(ent):] == FF).all(), name
        assert (r.counts == cnt).all() and (r.offsets == off).all(), name
        # ... and the sort the device gives for the sparser map itself
        want = m.sort_model(words, idx, 0, c, pre, lo, hi)
        direct = device_sort(words, idx, 0, c, pre, 16, lo, hi)
        check_sort(direct, want, c, pre, 16)
        b0, b1 = (lo, hi) if shard else (0, nbt)
        assert (r.counts[b0:b1] == direct.counts[b0:b1]).all(), name
        assert (r.offsets[b0:b1 + 1] == direct.offsets[b0:b1 + 1]).all() and r.offsets[nbt] == direct.offsets[nbt], name
        got, exp = m.by_bucket(r.entries, r.offsets, b0, b1), m.by_bucket(direct.entries, direct.offsets, b0, b1)
        assert (got[0] == exp[0]).all() and (got[1] == exp[1]).all(), name
        if name == "none":
            assert r.offsets[nbt] == 0 and (r.entries == FF).all()


# ------------------------------------------------------------------ scans
def device_scan(x, dn=None):
    x = np.ascontiguousarray(x, dtype=np.uint32)
    out = np.zeros(max(len(x), 1), dtype=np.uint32)
    st = _lib().bh_selftest_scan(0, _p(x) if len(x) else None, len(x), -1 if dn is None else dn,
                                 _p(out) if len(x) else None)
    assert st == 0
    return out[:len(x)]


@pytest.mark.parametrize("n", [0, 1, 1023, 1024, 1025, (1 << 20) - 1, 1 << 20, (1 << 20) + 1])
def test_exclusive_scan(n):
    """three levels of tiles at 2^20 + 1; running sums far past 2^32; the bounded form leaves
    every word past *dn as it was (0xFF here: a sum that took one in would show it)"""
    x = np.random.RandomState(n & 0xFFFF).randint(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32)
    if n > 2:
        assert len(set(x[:64].tolist())) > 1
    if n > 8:
        assert int(x.astype(np.uint64).sum()) > 1 << 32
    assert (device_scan(x) == m.scan_model(x)).all()
    for dn in sorted({0, 1023, 1024, n - 1, n, n + 5}):
        if dn < 0:
            continue
        y = x.copy()
        y[dn + 1:] = FF
        got = device_scan(y, dn)
        assert (got == m.scan_model(y, dn)).all(), dn
        assert (got[dn + 1:] == FF).all(), dn


# ------------------------------------------------------------------ density index
@pytest.mark.parametrize("n", [1, 63, 64, 65, 64 * 1024 + 1])
def test_density_index(n):
    nw = (n + 63) // 64
    rng = np.random.RandomState(n)
    words = rng.randint(0, 1 << 63, size=nw, dtype=np.uint64) * np.uint64(2) + rng.randint(0, 2, size=nw).astype(np.uint64)
    words[0] |= np.uint64(1) | np.uint64(1 << 63)
    if nw > 8:
        words[3], words[4], words[5] = np.uint64(0xFFFFFFFFFFFFFFFF), np.uint64(0), np.uint64(0xFFFFFFFFFFFFFFFF)
        words[1024 // 64 * 4 - 1] = np.uint64(0xFFFFFFFFFFFFFFFF)
    words[-1] = np.uint64(0xFFFFFFFFFFFFFFFF)        # the bits past n are set and must not count
    idx = np.full(n, 0x55555555, dtype=np.int32)
    assert _lib().bh_selftest_density_index(0, _p(words), n, 12345, _p(idx)) == 0
    want = m.density_model(words, n, 12345)
    assert (idx == want).all()
    assert want[0] == 12345 and (n < 64 or want[63] >= 12346)


# ------------------------------------------------------------------ scalar preparation
def _prepare_inputs(mode, n, rng):
    r = m.R
    if mode == 0:
        special = [0, r - 1, r, r + 1, 2 * r - 1, 2 * r, 2 * r + 1, (1 << 256) - 1]
        bound = 1 << 256
    elif mode == 1:
        special = [0, pow(2, 256, r), r - 1, 1, pow(2, 256, r) * 5 % r]
        bound = r
    else:
        special = [0, r, r + 1, 2 * r - 1, r - 1, pow(2, 261, r), pow(2, 261, r) + r]
        bound = 2 * r
    vals = [rng.randrange(bound) for _ in range(n)]
    if n >= 2 * len(special):
        for k, s in enumerate(special):
            vals[(k * 37 + 5) % n] = s       # (distinct slots: 37 is odd and n a power of two or larger)
        assert all(s in vals for s in special)
    return vals


def _device_prepare(vals, mode, log_perm):
    words = m.to_words(vals)
    out = np.zeros_like(words)
    assert _lib().bh_selftest_scalars_prepare(0, _p(words), len(vals), mode, log_perm, _p(out)) == 0
    return out


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_scalars_prepare(mode):
    rng = random.Random(40 + mode)
    if mode == 0:
        assert (1 << 256) - 1 >= 2 * m.R        # needs both subtractions
    if mode == 2:
        # the packed value r comes out of the Montgomery reduction as exactly r
        mm = (-m.R * pow(m.R, -1, 1 << 261)) % (1 << 261)
        assert (m.R + mm * m.R) >> 261 == m.R and (m.R + mm * m.R) % (1 << 261) == 0
    for log_perm, n in [(0, 100)] + [(lp, 1 << lp) for lp in range(1, 13)]:
        vals = _prepare_inputs(mode, n, rng)
        want = m.prepare_model(vals, mode, log_perm)
        assert all(v < m.R for v in want)
        got = _device_prepare(vals, mode, log_perm)
        assert (got == m.to_words(want)).all(), (mode, log_perm)
    if mode == 0:
        special = [0, m.R - 1, m.R, m.R + 1, 2 * m.R - 1, 2 * m.R, 2 * m.R + 1, (1 << 256) - 1]
        assert m.from_words(_device_prepare(special, 0, 0)) == [0, m.R - 1, 0, 1, m.R - 1, 0, 1, (1 << 256) - 1 - 2 * m.R]


# ------------------------------------------------------------------ argument validation
def test_invalid_arguments_are_refused():
    AB = 0xABABABAB
    words = _words(16, 255)

    def refused(r):
        return r.status == INVALID and (r.counts == AB).all() and (r.offsets == AB).all() and (r.entries == AB).all()

    # shard bounds: not on the granule, past NB, empty, without a table, on 1024 where c = 24 needs 2048
    for c, pre, lo, hi in [(16, 1, 512, 2048), (16, 1, 1024, 1536), (16, 1, 0, 32768 + 1024), (16, 1, 2048, 2048),
                           (16, 1, 2048, 1024), (16, 0, 1024, 2048), (24, 1, 1024, 4096), (24, 1, 2048, 4096 + 1024)]:
        assert refused(device_sort(_words(c, 255), None, 0, c, pre, 16, lo, hi, fill=AB)), (c, pre, lo, hi)
    assert device_sort(_words(24, 255), None, 0, 24, 1, 16, 2048, 4096, fill=AB).status == 0
    # window sizes
    for c in (1, 25, 0, -3):
        assert device_sort(words, None, 0, c, 0, 16, fill=AB).status == INVALID
        assert device_sort(words, None, 0, c, 1, 16, fill=AB).status == INVALID
    # segment length, base indices
    assert refused(device_sort(words, None, 0, 16, 0, 0, fill=AB))
    for bad in (-2, (1 << 31) // 16, (1 << 31) - 1):
        idx = np.arange(255, dtype=np.int32)
        idx[77] = bad
        assert refused(device_sort(words, idx, 0, 16, 1, 16, fill=AB)), bad
    idx[77] = (1 << 31) // 16 - 1
    assert device_sort(words, idx, 0, 16, 1, 16, fill=AB).status == 0
    assert refused(device_sort(words, None, (1 << 31) // 16 - 254, 16, 1, 16, fill=AB))
    # the derive entry: offsets that decrease, a count past the capacity, a base outside the map
    c, pre, n = 13, 1, 255
    W, NB, Wb, nbt = m.geometry(c, pre)
    src = device_sort(_words(c, n), None, 50, c, pre, 16)
    assert src.status == 0
    idx = np.arange(n, dtype=np.int32)

    def derive(entries=None, offsets=None, idx=idx, src_off=50, b0=0, b1=0):
        s = Run()
        s.entries = src.entries if entries is None else entries
        s.offsets = src.offsets if offsets is None else offsets
        r = device_derive(s, nbt, pre, W, src_off, idx, b0, b1, n * W, fill=AB)
        return r.status, (r.counts == AB).all() and (r.offsets == AB).all() and (r.entries == AB).all()

    assert derive()[0] == 0
    b = int(np.flatnonzero(src.counts)[0])
    off = src.offsets.copy()
    off[b + 1] = off[b] - 1 if off[b] else off[b + 2] + 1
    assert derive(offsets=off) == (INVALID, True)
    off = src.offsets.copy()
    off[nbt] = n * W + 1
    assert derive(offsets=off) == (INVALID, True)
    ent = src.entries.copy()
    ent[0] = (50 + n) * W
    assert derive(entries=ent) == (INVALID, True)
    ent[0] = 49 * W + (W - 1)
    assert derive(entries=ent) == (INVALID, True)
    assert derive(src_off=51) == (INVALID, True)
    assert derive(b0=5, b1=4) == (INVALID, True) and derive(b1=nbt + 1) == (INVALID, True)
    bad = idx.copy()
    bad[3] = -2
    assert derive(idx=bad) == (INVALID, True)
    # the others
    x = np.zeros(4, dtype=np.uint32)
    assert _lib().bh_selftest_scan(0, _p(x), (1 << 21) + 1, -1, _p(x)) == INVALID
    assert _lib().bh_selftest_scan(0, _p(x), 4, -2, _p(x)) == INVALID
    assert _lib().bh_selftest_scalars_prepare(0, _p(x), 4, 3, 0, _p(x)) == INVALID
    assert _lib().bh_selftest_scalars_prepare(0, _p(x), 4, 0, 3, _p(x)) == INVALID
    assert _lib().bh_selftest_density_index(0, _p(x), (1 << 17) + 1, 0, _p(x)) == INVALID
