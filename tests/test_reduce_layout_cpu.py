"""The entry lists of tests/reduce_layout.py are what they claim: test_gpu_reduce.py can only
catch a wrong continuation fold if the list still holds the bucket that reaches it.  No library
call: the spans are counted from the offsets, the partials come from tests/accumulate_model.py over
the integers mod r (the base pool's own scalars)."""
import pytest

import reduce_layout as rl
from accumulate_model import NONE, bucket_totals, expected, range_sums
from test_gpu_accumulate import NBASES, NEG, _scalars

R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
SIZES = [(S, BT) for S in (3, 8) for BT in (256, 128)]
add = lambda a, b: (a + b) % R


def _values(plan):
    ks = _scalars()
    return [(R - ks[e & ~NEG]) % R if e & NEG else ks[e & ~NEG] % R for e in plan.entries]


def _present(plan, b0, nb):
    return {plan.ncont(b) for b in range(b0, b0 + nb) if plan.offsets[b + 1] > plan.offsets[b]}


@pytest.mark.parametrize("S,BT", SIZES)
def test_every_list_is_well_formed_and_every_range_is_in_its_regime(S, BT):
    for kind in rl.KINDS:
        p = rl.build(kind, S, BT)
        assert p.S == S and len(p.offsets) == p.Wb * p.NB + 1 and p.offsets[-1] == len(p.entries) <= 1 << 16
        assert all(e & ~NEG < NBASES for e in p.entries)
        assert len(p.entries) % S, (kind, "the last segment is partial")
        assert len(p.ranges) == len(p.regimes)
        for (b0, nbr), (lo, hi) in zip(p.ranges, p.regimes):
            assert b0 + nbr <= p.NB and (p.Wb == 1 or (b0, nbr) == (0, p.NB))
            assert nbr & (nbr - 1) == 0 or nbr % 1024 == 0
            assert lo < p.longest(b0, p.Wb * nbr) <= hi, (kind, b0, nbr)


@pytest.mark.parametrize("S,BT", SIZES)
def test_the_thresholds_and_the_tree_depths_are_present(S, BT):
    fold, seq, long_ = (rl.build(k, S, BT) for k in ("fold", "seq", "long"))
    want = set(rl.thresholds(BT))
    assert {k for k in want if k <= rl.FOLD_SPAN} <= _present(fold, 0, 64)
    assert {k for k in want if k <= rl.SEQ_MAX} <= _present(seq, 0, 64)
    assert {1} | set(range(2, 9)) & want <= _present(seq, 0, 64)      # ncont 1 and 2..8 beside longer ones
    for b0, nbr in long_.ranges:                                         # whole and cut
        assert want | set(rl.TREE_SPANS) <= _present(long_, b0, nbr), (b0, nbr)
    # the cut lists hold the same window of 64 behind their flank
    for kind, base in (("fold_cut", fold), ("seq_cut", seq)):
        p = rl.build(kind, S, BT)
        assert _present(p, 64, 64) >= _present(base, 0, 64) - {0} and p.longest(64, 64) == base.longest(0, 64)
    # a multiexp of three windows: a long bucket last in one window, another first in the next
    plain = rl.build("plain", S, BT)
    assert plain.marks["last_of_window"] == 15 and plain.marks["first_of_window"] == 16
    assert min(plain.ncont(15), plain.ncont(16)) > rl.SEQ_MAX


@pytest.mark.parametrize("S,BT", SIZES)
def test_edges_and_the_long_buckets_lists(S, BT):
    for kind in ("fold", "seq", "fold_cut", "seq_cut", "long"):
        p = rl.build(kind, S, BT)
        b = p.marks["ends_on_boundary"]
        assert p.offsets[b + 1] % S == 0 and p.ncont(b) >= 1
        b = p.marks["starts_on_boundary"]
        assert p.offsets[b] % S == 0 and p.ncont(b) >= 1
    for kind in rl.KINDS:
        p = rl.build(kind, S, BT)
        for b0, nbr in p.ranges:
            first, last = b0, b0 + p.Wb * nbr - 1
            assert p.offsets[last + 1] > p.offsets[last] and p.offsets[last + 1] % S, (kind, "last bucket")
            if b0:
                assert p.offsets[first + 1] > p.offsets[first] and p.offsets[first] % S, (kind, "first bucket")
    p = rl.build("long", S, BT)
    longs = [b for b in range(p.NB) if p.ncont(b) > rl.SEQ_MAX]
    for b0, nbr in p.ranges:
        inside = [b for b in longs if b0 <= b < b0 + nbr]
        # the same workgroup's list (buckets b0 + i BT ... of the range) holds two of them ...
        assert any((a - b0) // BT == (b - b0) // BT for a in inside for b in inside if a < b)
        # ... and empty buckets lie between long ones
        assert any(all(p.ncont(c) == 0 and p.offsets[c] == p.offsets[c + 1] for c in range(a + 1, a + 9))
                   for a in inside if a + 9 <= b0 + nbr)
    assert any(b - a > BT and (b // BT != a // BT) for a in longs for b in longs)
    p = rl.build("shard", S, BT)
    assert p.marks["far"] - p.marks["first_of_range"] > BT
    assert sum(p.offsets[b + 1] > p.offsets[b] for b in range(p.NB)) < 20


@pytest.mark.parametrize("S,BT", SIZES)
def test_a_cut_leaves_a_long_bucket_on_each_side(S, BT):
    for kind in ("fold_cut", "seq_cut", "long", "shard"):
        p = rl.build(kind, S, BT)
        (b0, nbr), = p.flanks
        assert (b0, nbr) in p.ranges
        below, above = p.flanks[(b0, nbr)]
        assert below == b0 - 1 and above == b0 + nbr
        assert p.ncont(below) > rl.SEQ_MAX and p.ncont(above) > rl.SEQ_MAX


@pytest.mark.parametrize("S,BT", SIZES)
def test_the_exceptional_buckets_give_the_partials_they_claim(S, BT):
    seen = set()
    for kind in rl.KINDS:
        p = rl.build(kind, S, BT)
        values = _values(p)
        for what, buckets in p.kinds.items():
            if what == "generic":
                continue
            for b in buckets:
                n = p.ncont(b)
                sums, conts, cb = expected(values, p.offsets, S, b, b + 1, add, 0)
                parts = [conts[s] for s in sorted(conts)]
                assert len(parts) == n and set(cb.values()) <= {b, NONE} and list(sums) == [b]
                seen.add((kind, what, n))
                if what == "periodic":
                    assert len(set(parts)) == 1 and parts[0] != 0
                elif what == "alternating":
                    x = parts[0]
                    assert x != 0 and {x, R - x} == set(parts) and sum(parts) % R == 0
                    assert parts[1] == R - x or parts[:4] == [x] * 4 and parts[4:8] == [R - x] * 4
                elif what == "identity":
                    assert sums[b] == 0 and set(parts) == {0}
                else:
                    assert what == "own_identity" and sums[b] == 0 and n >= 1 and sum(parts) % R
    # each fold meets each kind: k_cont_fold alone (fold), k_cont_seq (seq), k_cont_long (long)
    for what in ("periodic", "alternating", "identity", "own_identity"):
        assert any(k == "fold" and w == what for k, w, n in seen)
        assert any(k == "seq" and w == what and n > rl.FOLD_SPAN for k, w, n in seen) or what == "own_identity"
    assert ("long", "periodic", 128) in seen and ("long", "alternating", 66) in seen
    assert any(k == "seq" and w == "periodic" and n % 4 == 0 and n > rl.FOLD_SPAN for k, w, n in seen)


def test_the_model_of_the_reduction_over_the_integers():
    # buckets 2..5 of six, values 1..: sum (b - b0 + 1) B_b and sum B_b
    offsets = [0, 1, 1, 3, 3, 4, 6]
    values = [10, 1, 2, 3, 4, 5]
    plus = lambda a, b: a + b
    totals = bucket_totals(values, offsets, 2, 6, plus, 0)
    assert totals == {2: 3, 4: 3, 5: 9}
    assert range_sums(totals, 2, 4, plus, 0) == (1 * 3 + 3 * 3 + 4 * 9, 15)
