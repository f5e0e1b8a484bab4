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
and G2 through the oracle)."""

NONE = 0xFFFFFFFF


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
