"""What the accumulation kernels (csrc/msm_impl.cuh: k_accumulate_pf, k_accumulate_g2d) must write,
over any group: the expected-value model of their segment bookkeeping.

Sorted entries lie bucket after bucket (offsets[b] .. offsets[b + 1]); thread s owns segment
[s S, s S + S), clipped to the entries of buckets [b_lo, b_hi).  Within its clipped segment:
  * a bucket whose first entry lies in the segment gets bucket_sums[b] = the sum of its entries up
    to the segment's end;
  * a segment that begins inside a bucket gets conts[s] = the sum from the segment's start to the
    bucket's (or the segment's) end, and cont_bucket[s] = b;
  * otherwise cont_bucket[s] = NONE, when the clipped segment starts at s S;
  * nothing else is written.
Used by test_accumulate_model_cpu.py (over the integers mod r) and test_gpu_accumulate.py (over G1
and G2 through the oracle).  bucket_totals and range_sums say what the back half (reduce_range)
must make of those pieces: test_gpu_reduce.py, test_reduce_layout_cpu.py."""

NONE = 0xFFFFFFFF


def bucket_totals(values, offsets, b_lo, b_hi, add, zero):
    """What the continuation folds (k_cont_seq, k_cont_long, k_cont_treeF, k_cont_fold) must leave
    in bucket_sums[b]: the plain sum of the bucket's entries, for every non-empty bucket of
    [b_lo, b_hi)."""
    out = {}
    for b in range(b_lo, b_hi):
        if offsets[b + 1] > offsets[b]:
            acc = zero
            for j in range(offsets[b], offsets[b + 1]):
                acc = add(acc, values[j])
            out[b] = acc
    return out


def range_sums(totals, b0, nbr, add, zero):
    """(sum_b (b - b0 + 1) B_b, sum_b B_b) over the buckets [b0, b0 + nbr) -- bucket b0 + i holds
    digit i + 1 of the range -- by the serial running sum of multiexp.rs."""
    run, acc = zero, zero
    for b in range(b0 + nbr - 1, b0 - 1, -1):
        if b in totals:
            run = add(run, totals[b])
        acc = add(acc, run)
    return acc, run


def expected(values, offsets, S, b_lo, b_hi, add, zero):
    """values[j]: the group element entry j contributes.  Returns three dicts holding only the
    written slots: bucket_sums[b], conts[s], cont_bucket[s]."""
    bucket_sums, conts, cont_bucket = {}, {}, {}
    e_lo, e_hi = offsets[b_lo], offsets[b_hi]

    def total(lo, hi):
        acc = zero
        for j in range(lo, hi):
            acc = add(acc, values[j])
        return acc

    for s in range((len(values) + S - 1) // S):
        lo, hi = max(s * S, e_lo), min(s * S + S, e_hi)
        if lo >= hi:
            continue
        continued = False
        for b in range(b_lo, b_hi):
            first, end = offsets[b], offsets[b + 1]
            if first == end or end <= lo or first >= hi:
                continue
            piece = total(max(first, lo), min(end, hi))
            if first >= s * S:
                bucket_sums[b] = piece
            else:
                conts[s], cont_bucket[s], continued = piece, b, True
        if not continued and lo == s * S:
            cont_bucket[s] = NONE
    return bucket_sums, conts, cont_bucket
