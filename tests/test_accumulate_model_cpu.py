"""The bookkeeping model of the accumulation kernels (tests/accumulate_model.py) over the integers
mod r: whatever the layout, a bucket's own partial and its continuation partials add up to the
bucket's plain sum, every slot is written at most where the kernels' consumers read it, and
nothing outside [b_lo, b_hi) is written.  test_gpu_accumulate.py holds the kernels to this model."""
import random

import pytest

from accumulate_model import NONE, expected

R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001


def _layout(rng, nbt, max_len, empty):
    offsets = [0]
    for _ in range(nbt):
        offsets.append(offsets[-1] + (0 if rng.random() < empty else rng.randrange(1, max_len + 1)))
    return offsets


def _check(values, offsets, S, b_lo, b_hi):
    add = lambda a, b: (a + b) % R
    sums, conts, cb = expected(values, offsets, S, b_lo, b_hi, add, 0)
    nbt = len(offsets) - 1
    segs = (len(values) + S - 1) // S
    assert set(conts) <= set(cb) and all(cb[s] != NONE for s in conts)
    assert all(0 <= s < segs for s in cb)
    for b in range(nbt):
        first, end = offsets[b], offsets[b + 1]
        inside = b_lo <= b < b_hi and end > first
        assert (b in sums) == inside, b
        parts = [conts[s] for s in sorted(conts) if cb[s] == b]
        if not inside:
            assert not parts
            continue
        assert (sums[b] + sum(parts)) % R == sum(values[first:end]) % R, b
        # one continuation partial per further segment the bucket reaches into
        assert len(parts) == (end - 1) // S - first // S, b
    # a segment that starts a bucket exactly at its own start continues nothing
    e_lo, e_hi = offsets[b_lo], offsets[b_hi]
    for s in range(segs):
        if e_lo <= s * S < e_hi:
            starts_bucket = any(offsets[b] == s * S and offsets[b + 1] > s * S for b in range(b_lo, b_hi))
            assert (cb[s] == NONE) == starts_bucket, s
        else:
            assert s not in cb, s


@pytest.mark.parametrize("S", [1, 3, 8])
def test_pieces_add_up_to_the_bucket_sums(S):
    rng = random.Random(100 + S)
    for trial in range(60):
        nbt = rng.randrange(1, 40)
        offsets = _layout(rng, nbt, rng.choice([1, 2, 5, 30]), rng.choice([0.0, 0.3, 0.8]))
        if offsets[-1] == 0:
            continue
        values = [rng.randrange(R) for _ in range(offsets[-1])]
        _check(values, offsets, S, 0, nbt)
        for _ in range(4):      # cut ranges: any [b_lo, b_hi) that holds an entry
            b_lo = rng.randrange(nbt)
            b_hi = rng.randrange(b_lo + 1, nbt + 1)
            if offsets[b_lo] < offsets[b_hi]:
                _check(values, offsets, S, b_lo, b_hi)


def test_a_bucket_over_three_segments_and_runs_of_empty_buckets():
    # entries 0..11, S = 4: bucket 0 = [0, 2), buckets 1-3 empty, bucket 4 = [2, 11), 5 empty, 6 = [11, 12)
    offsets = [0, 2, 2, 2, 2, 11, 11, 12]
    values = list(range(1, 13))
    add = lambda a, b: a + b
    sums, conts, cb = expected(values, offsets, 4, 0, 7, add, 0)
    assert sums == {0: 1 + 2, 4: 3 + 4, 6: 12}
    assert conts == {1: 5 + 6 + 7 + 8, 2: 9 + 10 + 11}
    assert cb == {0: NONE, 1: 4, 2: 4}
    # cut to bucket 4 alone: its first segment starts at entry 2, not at the segment's start
    sums, conts, cb = expected(values, offsets, 4, 4, 5, add, 0)
    assert sums == {4: 3 + 4} and conts == {1: 26, 2: 30} and cb == {1: 4, 2: 4}
