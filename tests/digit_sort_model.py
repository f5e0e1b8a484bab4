"""Plain Python/numpy model of the layer between a caller's scalars and the accumulation kernels
(csrc/msm_common.hip): scalar preparation, the density index, the exclusive scans, the signed
c-bit digit recoding, the digit sort with its bucket shards, the derived (compacted) sorts and
the span words.  It takes nothing from the library; tests/test_digit_sort_model_cpu.py vouches
for it and tests/test_gpu_digit_sort.py compares the device with it, exactly.

Conventions (msm.h): a scalar is 8 little-endian 32-bit words; W = ceil(256 / c) digit windows;
NB = 2^(c-1) buckets per bucket window; Wb = W bucket windows, or 1 with a window table (pre);
nbt = Wb * NB.  Digit d != 0 of window w of the scalar with base index `base` goes to bucket
w * NB + |d| - 1 (|d| - 1 with pre) as the entry `base` (base * W + w with pre), bit 31 set when
d < 0.  Words the device does not write are modelled as UNSET, the 0xFF fill of the self-tests.
"""
import numpy as np

R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
NEG = 1 << 31
UNSET = 0xFFFFFFFF


# ------------------------------------------------------------------ encodings
def to_words(values):
    """ints in [0, 2^256) -> (n, 8) uint32, little endian"""
    buf = b"".join(int(v).to_bytes(32, "little") for v in values)
    return np.frombuffer(buf, dtype="<u4").reshape(-1, 8).astype(np.uint32)


def from_words(words):
    """(n, 8) uint32 -> ints"""
    raw = np.ascontiguousarray(words, dtype="<u4").tobytes()
    return [int.from_bytes(raw[i:i + 32], "little") for i in range(0, len(raw), 32)]


def geometry(c, pre):
    """W, NB, Wb, nbt of window size c"""
    W = (256 + c - 1) // c
    NB = 1 << (c - 1)
    Wb = 1 if pre else W
    return W, NB, Wb, Wb * NB


# ------------------------------------------------------------------ chosen scalars
def below_r(k):
    """k with its top set bits cleared, from the top down, until it is below r"""
    while k >= R:
        k &= ~(1 << (k.bit_length() - 1))
    return k


def patterns(c):
    """The scalars whose digits meet the conditions random ones almost never do, by name: every
    window raw 2^(c-1) (stays positive, no carry); every window 2^(c-1) + 1 (negative, carries);
    2^(c-1) + 1 and 2^(c-1) - 1 alternating (the carry makes the second exactly +2^(c-1)); all ones
    (digits of 0 that keep carrying); and 0, 1, r - 1, r - 2."""
    W, half = (256 + c - 1) // c, 1 << (c - 1)

    def every(f):
        return below_r(sum(f(w) << (c * w) for w in range(W)) & ((1 << 256) - 1))

    return {"half": every(lambda w: half), "half+1": every(lambda w: half + 1),
            "alternating": every(lambda w: half - 1 if w & 1 else half + 1), "ones": below_r((1 << 256) - 1),
            "0": 0, "1": 1, "r-1": R - 1, "r-2": R - 2}


def scalar_vector(c, n, rng):
    """n scalars: the patterns of c, then random ones below r"""
    out = list(patterns(c).values())[:n]
    return out + [rng.randrange(R) for _ in range(n - len(out))]


# ------------------------------------------------------------------ digits
def digits(k, c):
    """The signed-digit recoding of digit_at: d = raw + carry; d > 2^(c-1) -> d -= 2^c, carry 1.
    Returns (the W digits, the carry out of the top window)."""
    W = (256 + c - 1) // c
    half, carry, out = 1 << (c - 1), 0, []
    for w in range(W):
        d = ((k >> (c * w)) & ((1 << c) - 1)) + carry
        if d > half:
            d -= 1 << c
            carry = 1
        else:
            carry = 0
        out.append(d)
    return out, carry


def digits_array(words, c):
    """digits() of every row of an (n, 8) uint32 array, window by window as digit_at reads them
    (two 32-bit words, shifted): ((n, W) int64 digits, (n, W) carry into each window, (n,) carry out)"""
    s = np.ascontiguousarray(words, dtype=np.uint32).reshape(-1, 8).astype(np.uint64)
    n = s.shape[0]
    W = (256 + c - 1) // c
    half = 1 << (c - 1)
    zero = np.zeros(n, dtype=np.uint64)
    d = np.zeros((n, W), dtype=np.int64)
    cin = np.zeros((n, W), dtype=np.int64)
    carry = np.zeros(n, dtype=np.int64)
    for w in range(W):
        bit = w * c
        wi, sh = bit >> 5, bit & 31
        lo = s[:, wi] if wi < 8 else zero
        hi = s[:, wi + 1] if wi + 1 < 8 else zero
        raw = (((hi << np.uint64(32)) | lo) >> np.uint64(sh)) & np.uint64((1 << c) - 1)
        cin[:, w] = carry
        v = raw.astype(np.int64) + carry
        over = v > half
        d[:, w] = np.where(over, v - (1 << c), v)
        carry = over.astype(np.int64)
    return d, cin, carry


# ------------------------------------------------------------------ the digit sort
class Sorted:
    """bucket[j], entry[j] of every kept entry in (bucket, entry) order -- each bucket's multiset of
    entries -- with counts[nbt] and offsets[nbt + 1].  For a bucket shard the offsets count from
    bk_lo: the device writes counts[b] for bk_lo <= b < bk_hi and offsets[b] for bk_lo <= b <= bk_hi
    and b = nbt; `written_counts` / `written_offsets` mark those words."""

    def __init__(self, bucket, entry, nbt, lo, hi):
        order = np.lexsort((entry, bucket))
        self.bucket, self.entry, self.nbt = bucket[order], entry[order], nbt
        self.counts = np.bincount(self.bucket, minlength=nbt).astype(np.uint32)
        self.offsets = np.zeros(nbt + 1, dtype=np.uint32)
        np.cumsum(self.counts, out=self.offsets[1:], dtype=np.uint32)
        self.written_counts = np.zeros(nbt, dtype=bool)
        self.written_counts[lo:hi] = True
        self.written_offsets = np.zeros(nbt + 1, dtype=bool)
        self.written_offsets[lo:hi + 1] = True
        self.written_offsets[nbt] = True

    @property
    def total(self):
        return int(self.offsets[self.nbt])


def sort_model(scalars, idx, base_offset, c, pre, bk_lo=0, bk_hi=0):
    """scalars: ints or an (n, 8) uint32 array; idx: per-scalar base index (-1: absent) or None for
    base_offset + i; [bk_lo, bk_hi): a bucket shard (pre only), 0, 0: every bucket."""
    words = scalars if isinstance(scalars, np.ndarray) else to_words(scalars)
    words = words.reshape(-1, 8)
    n = words.shape[0]
    W, NB, Wb, nbt = geometry(c, pre)
    d, _, _ = digits_array(words, c)
    base = (np.arange(n, dtype=np.int64) + base_offset) if idx is None else np.asarray(idx, dtype=np.int64)
    w = np.broadcast_to(np.arange(W, dtype=np.int64), (n, W))
    keep = (d != 0) & (base >= 0)[:, None]
    mag = np.abs(d) - 1
    bucket = mag if pre else w * NB + mag
    entry = (base[:, None] * W + w) if pre else np.broadcast_to(base[:, None], (n, W))
    entry = entry | np.where(d < 0, NEG, 0)
    lo, hi = (bk_lo, bk_hi) if bk_hi > bk_lo else (0, nbt)
    keep &= (bucket >= lo) & (bucket < hi)
    return Sorted(bucket[keep].astype(np.int64), entry[keep].astype(np.int64), nbt, lo, hi)


def by_bucket(entries, offsets, lo, hi):
    """A device layout's entries of buckets [lo, hi) as (bucket, entry) arrays in (bucket, entry)
    order: comparable with Sorted.bucket / Sorted.entry"""
    offsets = np.asarray(offsets, dtype=np.int64)
    cnt = offsets[lo + 1:hi + 1] - offsets[lo:hi]
    bucket = np.repeat(np.arange(lo, hi, dtype=np.int64), cnt)
    entry = np.asarray(entries[int(offsets[lo]):int(offsets[hi])], dtype=np.int64)
    order = np.lexsort((entry, bucket))
    return bucket[order], entry[order]


# ------------------------------------------------------------------ derived sorts
def derive_model(src_entries, src_offsets, nbt, idx, pre, W, src_off, b0=0, b1=0):
    """The stable compaction of derive_sorted: every source entry whose base maps to -1 dropped,
    the others remapped, in the source's order.  Returns (dst_entries, dst_counts[nbt],
    dst_offsets[nbt + 1]); counts are set for b0 <= b < b1, offsets for b0 <= b <= b1 and b = nbt
    (the derived entry count), the rest UNSET.  b1 = 0: nbt."""
    if b1 == 0:
        b1 = nbt
    src_offsets = np.asarray(src_offsets, dtype=np.int64)
    E = int(src_offsets[nbt])
    e = np.asarray(src_entries[:E], dtype=np.int64)
    v = e & (NEG - 1)
    base = v // W if pre else v
    nb = np.asarray(idx, dtype=np.int64)[base - src_off]
    keep = nb >= 0
    new = (nb * W + (v - base * W)) if pre else nb
    new = new | (e & NEG)
    pos = np.zeros(E + 1, dtype=np.int64)
    np.cumsum(keep, out=pos[1:])
    counts = np.full(nbt, UNSET, dtype=np.uint32)
    offsets = np.full(nbt + 1, UNSET, dtype=np.uint32)
    o = pos[src_offsets[b0:b1 + 1]]
    offsets[b0:b1 + 1] = o
    counts[b0:b1] = o[1:] - o[:-1]
    offsets[nbt] = o[-1]
    return new[keep].astype(np.uint32), counts, offsets


# ------------------------------------------------------------------ spans
def span_model(counts, offsets, S):
    """max over the non-empty buckets of (last segment - first segment), segments of S entries"""
    counts = np.asarray(counts, dtype=np.int64)
    off = np.asarray(offsets, dtype=np.int64)[:len(counts)]
    nz = counts > 0
    if not nz.any():
        return 0
    return int(((off[nz] + counts[nz] - 1) // S - off[nz] // S).max())


# ------------------------------------------------------------------ one-liners
def scan_model(x, dn=None):
    """exclusive prefix sums mod 2^32 of the first n (dn given: min(n, dn + 1)) words; the rest unchanged"""
    x = np.asarray(x, dtype=np.uint32)
    m = len(x) if dn is None else min(len(x), dn + 1)
    out = x.copy()
    if m:
        out[0] = 0
        out[1:m] = np.cumsum(x[:m - 1].astype(np.uint64)).astype(np.uint32)   # (truncation = mod 2^32)
    return out


def density_model(words, n, base_offset):
    """idx[i] = base_offset + (set bits below i) where bit i of the Lsb0 words is set, else -1"""
    bits = np.unpackbits(np.ascontiguousarray(words, dtype="<u8").view(np.uint8), bitorder="little")[:n].astype(np.int64)
    return np.where(bits == 1, base_offset + np.cumsum(bits) - bits, -1).astype(np.int32)


def bit_reverse(i, bits):
    return int(format(i, "0%db" % bits)[::-1], 2) if bits else i


def prepare_model(values, mode, log_perm=0):
    """out[i] of scalars_prepare for the source ints `values`: mode 0 k mod r, 1 x * 2^-256 mod r,
    2 x * 2^-261 mod r; the source index bit-reversed over log_perm bits"""
    scale = {0: 1, 1: pow(2, -256, R), 2: pow(2, -261, R)}[mode]
    return [values[bit_reverse(i, log_perm)] * scale % R for i in range(len(values))]
