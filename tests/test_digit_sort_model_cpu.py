"""What vouches for tests/digit_sort_model.py, the reference of tests/test_gpu_digit_sort.py.

Every property here is checked without reference to how the model computes: the digits of a scalar
must reconstruct it, the entries of the sort must reconstruct every scalar from their bucket ids
alone, a derived sort must equal the sort run directly with the sparser map, and disjoint bucket
shards must add up to the unsharded sort -- for every window size 2 .. 24 (the sorts with plain
windows up to 20, where the library stops too), over 0, 1, r - 1, r - 2, (r +- 1) / 2, the chosen
patterns of the GPU test (digits of +2^(c-1), carries out of zero digits, carries across 32-bit
words) and random scalars.
"""
import functools
import random

import numpy as np
import pytest

import digit_sort_model as m

CS = list(range(2, 25))
# plain windows (pre = 0) have W * 2^(c-1) buckets and the library takes them up to c = 20
# (bh_ctx_set_window); the shared buckets of a window table go to c = 24
SORT_CS = [(c, pre) for c in CS for pre in (0, 1) if pre or c <= 20]
N_RANDOM = 2000


@functools.lru_cache(maxsize=None)
def _scalars(c):
    rng = random.Random(1000 + c)
    return (list(m.patterns(c).values()) + [(m.R + 1) // 2, (m.R - 1) // 2]
            + [rng.randrange(m.R) for _ in range(N_RANDOM)])


def _powers(c, W):
    return np.array([1 << (c * w) for w in range(W)], dtype=object)


@pytest.mark.parametrize("c", CS)
def test_digits_reconstruct_the_scalar(c):
    ks = _scalars(c)
    W, half = (256 + c - 1) // c, 1 << (c - 1)
    d, cin, cout = m.digits_array(m.to_words(ks), c)
    assert d.shape == (len(ks), W)
    assert (np.abs(d) <= half).all()
    assert (cout == 0).all(), "a carry leaves the top window"
    assert (d.astype(object) @ _powers(c, W) == np.array(ks, dtype=object)).all()
    # the scalar form, as written in digit_at, and the array form agree
    for i in list(range(12)) + list(range(len(ks) - 40, len(ks))):
        dd, carry = m.digits(ks[i], c)
        assert carry == 0 and dd == d[i].tolist()
        assert sum(x << (c * w) for w, x in enumerate(dd)) == ks[i]
        raw = [(ks[i] >> (c * w)) & ((1 << c) - 1) for w in range(W)]
        assert cin[i, 0] == 0 and all(cin[i, w + 1] << c == raw[w] + cin[i, w] - dd[w] for w in range(W - 1))


@pytest.mark.parametrize("c", CS)
def test_patterns_meet_their_conditions(c):
    """each class the GPU test relies on occurs for every c (a straddling window needs c not
    dividing 32)"""
    W, half = (256 + c - 1) // c, 1 << (c - 1)
    p = m.patterns(c)
    assert all(k < m.R for k in p.values())
    d, cin, _ = m.digits_array(m.to_words(list(p.values())), c)
    row = dict(zip(p, range(len(p))))
    assert (d[row["half"], :W - 2] == half).all()
    assert (d[row["half+1"], 0] == -(half - 1)) and (d[row["half+1"], 1:W - 2] == -(half - 2)).all()
    assert (d[row["alternating"], 1:W - 2:2] == half).all()
    assert ((d[row["ones"]] == 0) & (cin[row["ones"]] == 1)).sum() >= W - 3
    if 32 % c:
        straddle = np.array([(w * c) // 32 != (w * c + c - 1) // 32 for w in range(W)])
        assert (cin[:, straddle] == 1).any()


def _reconstruct(s, c, pre, n, base_offset):
    """the scalars back from a Sorted's (bucket, entry) pairs: sum of +-(b + 1) * 2^(c w)"""
    W, NB, _, _ = m.geometry(c, pre)
    v = s.entry & (m.NEG - 1)
    sign = np.where(s.entry & m.NEG, -1, 1)
    if pre:
        base, w, b = v // W, v % W, s.bucket
    else:
        base, w, b = v, s.bucket // NB, s.bucket % NB
    D = np.zeros((n, W), dtype=np.int64)
    hits = np.zeros((n, W), dtype=np.int64)
    np.add.at(D, (base - base_offset, w), sign * (b + 1))
    np.add.at(hits, (base - base_offset, w), 1)
    assert hits.max() <= 1, "two entries for one (scalar, window)"
    return D.astype(object) @ _powers(c, W)


@pytest.mark.parametrize("c,pre", SORT_CS)
def test_sorted_entries_reconstruct_every_scalar(c, pre):
    ks = _scalars(c)
    s = m.sort_model(ks, None, 77, c, pre)
    _, _, _, nbt = m.geometry(c, pre)
    assert len(s.counts) == nbt and s.total == len(s.entry) == int(s.counts.sum())
    assert (np.diff(s.offsets.astype(np.int64)) == s.counts).all() and s.offsets[0] == 0
    assert (np.diff(s.bucket) >= 0).all()
    assert (_reconstruct(s, c, pre, len(ks), 77) == np.array(ks, dtype=object)).all()


def _maps(n, rng):
    half = np.array([rng.randrange(3 * n) if rng.random() < 0.5 else -1 for _ in range(n)], dtype=np.int64)
    first = np.full(n, -1, dtype=np.int64)
    first[0] = 5
    return {"half": half, "all": np.arange(n, dtype=np.int64)[::-1].copy(), "none": np.full(n, -1, dtype=np.int64),
            "first": first}


@pytest.mark.parametrize("c,pre", SORT_CS)
def test_derived_sort_equals_direct_sort(c, pre):
    ks = _scalars(c)[:400]
    W, NB, _, nbt = m.geometry(c, pre)
    words = m.to_words(ks)
    src = m.sort_model(words, None, 19, c, pre)
    for name, idx in _maps(len(ks), random.Random(c)).items():
        want = m.sort_model(words, idx, 0, c, pre)
        ent, cnt, off = m.derive_model(src.entry, src.offsets, nbt, idx, pre, W, 19)
        assert (cnt == want.counts).all() and (off == want.offsets).all(), name
        bucket, entry = m.by_bucket(ent, off, 0, nbt)
        assert (bucket == want.bucket).all() and (entry == want.entry).all(), name
    # a bucket range of the source alone
    if pre and NB >= 8:
        lo, hi = NB // 4, NB // 4 + NB // 2
        shard = m.sort_model(words, None, 19, c, 1, lo, hi)
        idx = _maps(len(ks), random.Random(c))["half"]
        want = m.sort_model(words, idx, 0, c, 1, lo, hi)
        ent, cnt, off = m.derive_model(shard.entry, shard.offsets, nbt, idx, 1, W, 19, lo, hi)
        assert (cnt[lo:hi] == want.counts[lo:hi]).all() and (off[lo:hi + 1] == want.offsets[lo:hi + 1]).all()
        assert off[nbt] == want.total and (cnt[:lo] == m.UNSET).all() and (off[hi + 1:nbt] == m.UNSET).all()
        bucket, entry = m.by_bucket(ent, off, lo, hi)
        assert (bucket == want.bucket).all() and (entry == want.entry).all()


@pytest.mark.parametrize("c", CS)
def test_shards_add_up_to_the_unsharded_sort(c):
    ks = _scalars(c)[:600]
    words = m.to_words(ks)
    _, NB, _, nbt = m.geometry(c, 1)
    full = m.sort_model(words, None, 3, c, 1)
    bounds = sorted({0, NB // 5, NB // 2, NB // 2 + 1 if NB > 2 else NB, NB})
    parts = [m.sort_model(words, None, 3, c, 1, lo, hi) for lo, hi in zip(bounds, bounds[1:])]
    assert sum(p.total for p in parts) == full.total
    assert (np.concatenate([p.bucket for p in parts]) == full.bucket).all()
    assert (np.concatenate([p.entry for p in parts]) == full.entry).all()
    for p, lo, hi in zip(parts, bounds, bounds[1:]):
        assert (p.counts[lo:hi] == full.counts[lo:hi]).all() and p.counts.sum() == p.total
        assert p.offsets[lo] == 0 and p.offsets[hi] == p.total == p.offsets[nbt]


def test_span_model():
    # buckets of 3, 0, 4, 1 entries at offsets 0, 3, 3, 7
    counts, offsets = [3, 0, 4, 1], [0, 3, 3, 7, 8]
    assert m.span_model(counts, offsets, 3) == 1      # [3, 7): segments 1 .. 2; [0, 3) ends on the boundary: 0
    assert m.span_model(counts, offsets, 2) == 2      # [3, 7): segments 1 .. 3
    assert m.span_model(counts, offsets, 8) == 0
    assert m.span_model([0, 0], [0, 0, 0], 3) == 0
    assert m.span_model([6], [0, 6], 3) == 1 and m.span_model([7], [0, 7], 3) == 2


def test_one_liners():
    x = np.array([5, 0xFFFFFFFF, 7, 1, 9], dtype=np.uint32)
    assert m.scan_model(x).tolist() == [0, 5, 4, 11, 12]
    assert m.scan_model(x, 2).tolist() == [0, 5, 4, 1, 9]
    assert m.scan_model(x, 0).tolist() == [0, 0xFFFFFFFF, 7, 1, 9]
    assert m.scan_model(x, 9).tolist() == m.scan_model(x).tolist()
    words = np.array([0b1011, 1 << 63 | 1], dtype=np.uint64)
    assert m.density_model(words, 66, 10).tolist()[:5] == [10, 11, -1, 12, -1]
    assert m.density_model(words, 128, 10)[64] == 13 and m.density_model(words, 128, 10)[127] == 14
    assert (m.density_model(words, 128, 10)[65:127] == -1).all()
    assert [m.bit_reverse(i, 3) for i in range(8)] == [0, 4, 2, 6, 1, 5, 3, 7]
    vals = [3, m.R + 2, 2 * m.R + 1, (1 << 256) - 1]
    assert m.prepare_model(vals, 0) == [3, 2, 1, ((1 << 256) - 1) % m.R]
    assert m.prepare_model(vals, 0, 2) == [3, 1, 2, ((1 << 256) - 1) % m.R]
    for mode, bits in ((1, 256), (2, 261)):
        out = m.prepare_model([pow(2, bits, m.R) * 12345 % m.R, 0], mode)
        assert out == [12345, 0]
    assert m.from_words(m.to_words(vals)) == vals
