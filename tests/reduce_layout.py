"""Entry lists for the back half of a multiexp (msm_impl.cuh: reduce_range), built so that every
bucket spans a chosen number of accumulation segments.

ncont(b) = (last segment of bucket b) - (first segment) is the number of continuation partials the
accumulation leaves for b in conts[]; which kernel folds them depends on ncont and on the longest
ncont of the reduced range:
  longest <= 8 (REDUCE_FOLD_SPAN)   k_cont_fold adds them all
  2 <= ncont <= 64 (cont_seq_max)   k_cont_seq<C, 4>: four strided sums and an LDS tree
  ncont > 64                        k_cont_long: one workgroup of BT threads per bucket (BT = 256
                                    for G1, 128 for G2), more than one strided step above BT
  no span words                     k_cont_treeF, 4-ary levels: 1, 2, 3, 5 levels at 4, 5..16,
                                    17..64, 257..1024 partials
The lists (build(kind, S, BT)), each with the ranges [b0, b0 + nbr) it is reduced over:
  fold, seq      one shared window of 64 buckets, longest span 8 / 64
  fold_cut,      the same 64 buckets as buckets 64..127 of a window of 256, with a bucket of 65
  seq_cut        partials on each side: reduced whole (then k_cont_long runs) and over [64, 128)
  long           a window of 512 with every threshold up to 2 BT + 1, whole and over [128, 384)
  plain          three windows of 16, a long bucket last in one window and first in the next
  shard          a window of 4096, almost empty, whole and over [1024, 2048)
Used by test_reduce_layout_cpu.py, which holds every list to these claims, and by
test_gpu_reduce.py.  The base pool and the Layout class are test_gpu_accumulate.py's."""
import functools

from test_gpu_accumulate import PP, NEG, Layout

FOLD_SPAN, SEQ_MAX = 8, 64                       # REDUCE_FOLD_SPAN, cont_seq_max()
BLOCK = {"G1": 256, "G2": 128}                   # k_cont_long's workgroup
TREE_SPANS = [4, 5, 16, 17, 65, 257]             # 1, 2, 2, 3, 4 and 5 levels of the 4-ary tree


def thresholds(BT):
    return [0, 1, 2, 3, 4, 5, 7, 8, 9, 63, 64, 65, BT - 1, BT, BT + 1, 2 * BT + 1]


class ReduceLayout(Layout):
    def phase(self, r):
        """one generic bucket, so that the next bucket starts r entries into a segment"""
        n = (r - self.pos) % self.S
        if n:
            self.bucket(self.generic(n))

    def empties(self, n):
        for _ in range(n):
            self.bucket([])

    def pad_to(self, index):
        assert len(self.buckets) <= index, (len(self.buckets), index)
        self.empties(index - len(self.buckets))

    def span(self, k, kind="generic", mark=None, boundary=None, block=1):
        """a bucket with ncont = k at the current position.  boundary: True ends it on a segment
        boundary, False inside a segment, None either.  kind:
          generic      random bases and signs
          periodic     every continuation segment holds the same S entries: equal partials
          alternating  the same S entries, negated in every other run of `block` segments
          identity     the bucket's own partial and every continuation partial are the identity
          own_identity the own partial is the identity ([PP, -PP]), the continuation is not"""
        S, r = self.S, self.pos % self.S
        if kind == "generic":
            lo, hi = max(k * S - r + 1, 1), (k + 1) * S - r
            if boundary is False:
                hi -= 1
            n = hi if boundary else self.rng.randrange(lo, hi + 1)
            entries = self.generic(n)
        elif kind in ("periodic", "alternating"):
            pattern = self.generic(S)
            entries = self.generic(S - r)
            for i in range(k):
                flip = NEG if kind == "alternating" and (i // block) % 2 else 0
                entries += [e ^ flip for e in pattern]
        elif kind == "identity":
            assert r == 0
            entries = [e for _ in range(k + 1) for e in self.identity_run(S)]
        else:
            assert kind == "own_identity" and r == S - 2 and k >= 1
            entries = [PP, PP | NEG] + self.generic(self.rng.randrange((k - 1) * S + 1, k * S + 1))
        self.bucket(entries, mark)
        b = len(self.buckets) - 1
        self.kinds.setdefault(kind, []).append(b)
        return b


def ncont(offsets, S, b):
    """continuation partials of bucket b (0 for an empty one)"""
    first, end = offsets[b], offsets[b + 1]
    return (end - 1) // S - first // S if end > first else 0


def _window_of_64(L, spans, periodic, alternating, identity):
    """64 buckets: one of each span, the exceptional buckets, every edge; the last one ends
    inside a segment"""
    start = len(L.buckets)
    L.span(spans[0])
    for i, k in enumerate(spans[1:]):
        if i % 3 == 0:
            L.empties(1 + i % 2)
        L.span(k)
    L.span(3, boundary=True, mark="ends_on_boundary")
    L.span(2, mark="starts_on_boundary")
    for k in periodic:
        L.span(k, "periodic")
    for k, block in alternating:
        L.span(k, "alternating", block=block)
    L.phase(0)
    L.span(identity, "identity")
    L.phase(L.S - 2)
    L.span(2, "own_identity")
    L.empties(3)
    L.span(1)
    L.pad_to(start + 63)
    L.span(2, boundary=False)


def _flank(L, index):
    """a bucket of 65 partials at `index`, ending inside a segment"""
    L.span(0)
    L.empties(2)
    L.span(1)
    L.pad_to(index)
    return L.span(SEQ_MAX + 1, boundary=False)


FOLD = dict(spans=[0, 1, 2, 3, 4, 5, 7, 8], periodic=[4, 8], alternating=[(8, 1), (8, 4)], identity=3)
SEQ = dict(spans=[0, 1, 2, 3, 4, 5, 7, 8, 9, 16, 17, 63, 64], periodic=[16, 64], alternating=[(16, 1), (16, 4)],
           identity=12)


class Plan:
    """entries, offsets, the shape (Wb windows of NB buckets), the ranges (b0, nbr) to reduce and
    the intended interval (lo, hi] of each range's longest span; kinds[kind]: the buckets of
    each exceptional kind; flanks: per range, the two buckets just outside it"""

    def __init__(self, L, Wb, NB, ranges, regimes, flanks=None):
        self.entries, self.offsets = L.arrays()
        self.S, self.Wb, self.NB, self.ranges, self.regimes = L.S, Wb, NB, ranges, regimes
        self.kinds, self.marks, self.flanks = L.kinds, L.marks, flanks or {}
        assert len(self.offsets) - 1 == Wb * NB, (len(self.offsets) - 1, Wb, NB)

    def ncont(self, b):
        return ncont(self.offsets, self.S, b)

    def longest(self, b0, nb):
        return max(self.ncont(b) for b in range(b0, b0 + nb))


KINDS = ["fold", "seq", "fold_cut", "seq_cut", "long", "plain", "shard"]
INF = 1 << 30


@functools.lru_cache(maxsize=None)
def build(kind, S, BT):
    L = ReduceLayout(S, 1000 * BT + 10 * S + KINDS.index(kind))
    L.kinds = {}
    if kind in ("fold", "seq"):
        _window_of_64(L, **(FOLD if kind == "fold" else SEQ))
        lim = (0, FOLD_SPAN) if kind == "fold" else (FOLD_SPAN, SEQ_MAX)
        return Plan(L, 1, 64, [(0, 64)], [lim])
    if kind in ("fold_cut", "seq_cut"):
        below = _flank(L, 63)
        _window_of_64(L, **(FOLD if kind == "fold_cut" else SEQ))
        above = L.span(SEQ_MAX + 1)
        L.empties(5)
        L.span(2)
        L.pad_to(255)
        L.span(1, boundary=False)
        lim = (0, FOLD_SPAN) if kind == "fold_cut" else (FOLD_SPAN, SEQ_MAX)
        return Plan(L, 1, 256, [(0, 256), (64, 64)], [(SEQ_MAX, INF), lim], {(64, 64): (below, above)})
    if kind == "long":
        # [128, 384) holds every threshold; 127 and 384 are the flanks; two buckets above 64
        # partials side by side (128, 129: one workgroup's list) and two more than BT apart
        below = _flank(L, 127)
        L.span(BT - 1, mark="first_of_range")
        L.span(BT, mark="beside")
        for i, k in enumerate([0, 1, 2, 3, 4, 5, 7, 8, 9, 16, 17, 63, 64, 65]):
            if i % 4 == 1:
                L.empties(2)
            L.span(k)
        L.span(3, boundary=True, mark="ends_on_boundary")
        L.span(2, mark="starts_on_boundary")
        L.span(128, "periodic")
        L.span(16, "periodic")
        L.span(66, "alternating", block=1)
        L.span(72, "alternating", block=4)
        L.phase(0)
        L.span(5, "identity")
        L.phase(S - 2)
        L.span(3, "own_identity")
        L.pad_to(300)                                    # a run of empty buckets between long ones
        L.span(BT + 1)
        L.empties(40)
        L.span(2 * BT + 1, mark="far")
        L.span(1)
        L.pad_to(383)
        L.span(SEQ_MAX + 2, boundary=False, mark="last_of_range")
        above = L.span(SEQ_MAX + 1)
        L.pad_to(511)
        L.span(1, boundary=False)
        return Plan(L, 1, 512, [(0, 512), (128, 256)], [(SEQ_MAX, INF), (SEQ_MAX, INF)], {(128, 256): (below, above)})
    if kind == "plain":
        L.span(1)
        L.span(0)
        L.empties(2)
        L.span(9)
        L.span(4, "periodic")
        L.pad_to(15)
        L.span(SEQ_MAX + 1, mark="last_of_window")
        L.span(SEQ_MAX + 2, mark="first_of_window")
        L.span(2)
        L.empties(3)
        L.span(8, "alternating")
        L.span(17)
        L.pad_to(33)
        L.span(3)
        L.phase(0)
        L.span(2, "identity")
        L.span(5)
        L.pad_to(47)
        L.span(2, boundary=False)
        return Plan(L, 3, 16, [(0, 16)], [(SEQ_MAX, INF)])
    assert kind == "shard"
    L.pad_to(5)
    L.span(2)
    below = _flank(L, 1023)
    L.span(SEQ_MAX + 2, mark="first_of_range")
    L.empties(5)
    L.span(3)
    L.span(0)
    L.pad_to(1500)
    L.span(9)
    L.span(16, "periodic")
    L.pad_to(1800)
    L.span(SEQ_MAX + 1, mark="far")
    L.pad_to(2047)
    L.span(2, boundary=False, mark="last_of_range")
    above = L.span(SEQ_MAX + 1)
    L.pad_to(4095)
    L.span(1, boundary=False)
    return Plan(L, 1, 4096, [(0, 4096), (1024, 1024)], [(SEQ_MAX, INF), (SEQ_MAX, INF)],
                {(1024, 1024): (below, above)})
