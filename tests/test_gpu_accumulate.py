"""The accumulation kernels on an entry list whose order the test chooses.

In a multiexp the order of the entries inside a bucket is decided by the sort's LDS atomics, so a
test through bh_multiexp cannot choose the sequence of additions an accumulator sees.
bh_selftest_accumulate (csrc/selftest.hip, msm_selftest_accumulate in csrc/msm_impl.cuh) launches
k_accumulate_pf<G1>, k_accumulate_pf<G2> or k_accumulate_g2d directly on caller-supplied bases,
entries (bit 31: negate), offsets, S and [b_lo, b_hi), and returns bucket_sums, conts and
cont_bucket, pre-filled with 0xFF bytes.  Every slot is compared with tests/accumulate_model.py
evaluated over the oracle's group: written slots bit-exactly as group elements (identity = the
all-zero point, coordinates inside the bounds of curve.cuh), unwritten slots still 0xFF.

The layout puts, in one entry list: [A, B, A + B] (a doubling of an accumulator with ZZ != 1),
[A, B, -(A + B), D] (the identity reached at ZZ != 1, then a restart), [P, P], [P, -P], buckets
whose sum is the identity, a bucket over four segments with a doubling inside one continuation
partial, another continuation partial that is the identity and its end exactly on a segment
boundary, runs of empty buckets in the middle and at a segment start, a first bucket at entry 0,
and random buckets up to two workgroups of segments with a partial last one.  Each run is repeated
with [b_lo, b_hi) cutting a segment at both ends.
"""
import ctypes
import functools
import random

import numpy as np
import pytest

from accumulate_model import NONE, expected
from oracle import bls12_381 as bls
from xyzz_device import G1, G2, check_point, limbs

pytestmark = pytest.mark.gpu

GROUPS = {"G1": G1, "G2": G2}
NEG = 1 << 31
INVALID = 10                                    # BH_ERR_INVALID_ARGUMENT
PACKED = {"G1": 24, "G2": 48}                   # u32 words per record: 2 x PACKED_WORDS
TABLE = {"G1": 32, "G2": 64}                    # raw-limb records (G1_TABLE_REC, G2_TABLE_REC)
A, B, C, D, E, F, PP, Q, NC, POOL0 = 0, 1, 2, 3, 4, 5, 6, 7, 8, 9   # C = A + B, F = D + E, NC = -C
NBASES = 32


def _fn():
    import bellman_hip as bh
    f = bh.lib().bh_selftest_accumulate
    f.restype = ctypes.c_int
    f.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint32,
                  ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint32,
                  ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    return f


def _scalars():
    """the bases' scalars: chosen, with C = A + B, F = D + E, NC = -C"""
    rng = random.Random(5)
    ks = [rng.randrange(1, 1 << 64) for _ in range(NBASES)]
    ks[C] = ks[A] + ks[B]
    ks[F] = ks[D] + ks[E]
    ks[NC] = bls.R - ks[C]
    return tuple(ks)


@functools.lru_cache(maxsize=None)
def _bases(name):
    """affine base points; the scalars are chosen, the sums follow"""
    c = GROUPS[name].curve
    return tuple(c.to_affine(c.mul(c.generator(), k)) for k in _scalars())


def _records(grp, rec):
    """the bases as packed (canonical Montgomery values in 32-bit words) or raw-limb records"""
    rows = []
    for a in _bases(grp.name):
        comps = [v for o in a for v in grp.mont(o)]
        if rec == PACKED[grp.name]:
            row = [(v >> (32 * i)) & 0xFFFFFFFF for v in comps for i in range(12)]
        else:
            row = [w for v in comps for w in limbs(v)]
        rows.append(row + [0] * (rec - len(row)))
    return np.array(rows, dtype=np.uint32)


class Layout:
    def __init__(self, S, seed):
        self.S, self.rng, self.buckets, self.pos, self.marks = S, random.Random(seed), [], 0, {}

    def bucket(self, entries, mark=None):
        if mark:
            self.marks[mark] = len(self.buckets)
        self.buckets.append(list(entries))
        self.pos += len(entries)

    def generic(self, n):
        return [self.rng.randrange(POOL0, NBASES) | (NEG if self.rng.random() < 0.5 else 0) for _ in range(n)]

    def identity_run(self, n):
        """n >= 2 entries that sum to the identity, through accumulators with ZZ != 1"""
        out = []
        while n:
            if n == 2 or n == 4:
                out += [PP, PP | NEG]
                n -= 2
            else:
                out += self.rng.choice([[A, B, C | NEG], [D, E, F | NEG], [A, B, NC]])
                n -= 3
        return out

    def fill_to(self, target, empty=0.0):
        while self.pos < target:
            if self.rng.random() < empty:
                self.bucket([])
            else:
                self.bucket(self.generic(min(self.rng.randrange(1, 7), target - self.pos)))

    def align(self, r):
        self.fill_to(self.pos + (r - self.pos) % self.S)

    def arrays(self):
        offsets = [0]
        for b in self.buckets:
            offsets.append(offsets[-1] + len(b))
        return [e for b in self.buckets for e in b], offsets


def _layout(S):
    L = Layout(S, 40 + S)
    L.bucket([A, B, C], "dbl")                           # starts at entry 0; a doubling at ZZ != 1
    L.bucket([A, B, C | NEG, D], "restart")              # the identity at ZZ != 1, then a restart
    L.bucket([PP, PP])
    L.bucket([PP, PP | NEG], "ident")
    L.bucket([A, B, NC])                                 # the identity through a base that is -C itself
    L.bucket([Q | NEG])
    for _ in range(3):
        L.bucket([])                                     # empty buckets in the middle
    L.bucket(L.generic(2))
    L.align(0)
    L.bucket([])                                         # empty buckets at a segment start
    L.bucket([])
    L.bucket([Q, D | NEG])
    L.align(1)
    # four segments: S - 1 entries of its own, [A, B, C, ...] (a doubling inside a continuation
    # partial), a continuation partial that is the identity, and a last full segment, so that the
    # bucket ends exactly on a segment boundary
    L.bucket(L.generic(S - 1) + [A, B, C] + L.generic(S - 3) + L.identity_run(S) + L.generic(S), "span")
    assert L.pos % S == 0
    L.bucket([D, E, F], "after_span")                    # starts at a segment start
    L.align(S - 2)
    L.bucket([PP, PP | NEG] + L.generic(S + 1), "ident_then_cont")   # own partial = identity, then a continuation
    # random buckets up to a second workgroup of segments (256 per workgroup) and a partial last segment
    L.fill_to(256 * S + 5 * S + 1, empty=0.2)
    return L


@functools.lru_cache(maxsize=None)
def _plan(name, S):
    """entries, offsets, the two bucket ranges and what the model expects for each"""
    grp = GROUPS[name]
    c = grp.curve
    L = _layout(S)
    entries, offsets = L.arrays()
    nbt = len(offsets) - 1
    assert (len(entries) + S - 1) // S > 256 and len(entries) % S
    jac = [c.from_affine(a) for a in _bases(name)]
    values = [c.neg(jac[e & ~NEG]) if e & NEG else jac[e & ~NEG] for e in entries]
    # the cut range: from the spanning bucket (which starts one entry into a segment) to a bucket
    # of the second workgroup's segments that ends inside a segment
    b_lo = L.marks["span"]
    b_hi = max(b for b in range(nbt) if offsets[b] % S and offsets[b] > 256 * S + S)
    assert offsets[b_lo] % S and offsets[b_hi] % S
    ranges = [(0, nbt), (b_lo, b_hi)]
    return entries, offsets, [(lo, hi, expected(values, offsets, S, lo, hi, c.add, c.identity)) for lo, hi in ranges]


def _launch(grp, kernel, rec, entries, offsets, S, b_lo, b_hi):
    nbt, n = len(offsets) - 1, len(entries)
    segs = (n + S - 1) // S if S else n         # (S = 0 is refused: test_invalid_arguments...)
    bases = _records(grp, rec)
    ent = np.array(entries, dtype=np.uint32)
    off = np.array(offsets, dtype=np.uint32)
    sums = np.zeros((nbt, grp.pw), dtype=np.uint32)
    conts = np.zeros((segs, grp.pw), dtype=np.uint32)
    cb = np.zeros(segs, dtype=np.uint32)
    st = _fn()(0, 0 if grp is G1 else 1, kernel, bases.ctypes.data, len(bases), rec, ent.ctypes.data, n,
               off.ctypes.data, nbt, S, b_lo, b_hi, sums.ctypes.data, conts.ctypes.data, cb.ctypes.data)
    return st, sums, conts, cb


CONFIGS = [("G1", 0), ("G2", 0), ("G2", 1)]         # kernel 0: k_accumulate_pf, 1: k_accumulate_g2d


@pytest.mark.parametrize("S", [3, 8])
@pytest.mark.parametrize("table_records", [False, True], ids=["packed", "limbs"])
@pytest.mark.parametrize("name,kernel", CONFIGS, ids=["g1", "g2", "g2_direct"])
def test_accumulation_on_an_ordered_entry_list(name, kernel, table_records, S):
    grp = GROUPS[name]
    rec = (TABLE if table_records else PACKED)[name]
    entries, offsets, runs = _plan(name, S)
    c = grp.curve
    for b_lo, b_hi, (want_sums, want_conts, want_cb) in runs:
        st, sums, conts, cb = _launch(grp, kernel, rec, entries, offsets, S, b_lo, b_hi)
        assert st == 0
        for what, got, want in (("bucket_sums", sums, want_sums), ("conts", conts, want_conts)):
            for i, words in enumerate(got):
                if i in want:
                    check_point(grp, words, want[i], zero_form=c.is_identity(want[i]), tag=(what, i, b_lo, b_hi))
                else:
                    assert (words == 0xFFFFFFFF).all(), (what, i, "written", b_lo, b_hi)
        assert [int(v) for v in cb] == [want_cb.get(s, NONE) for s in range(len(cb))]
        # the scenarios are what they claim to be
        if (b_lo, b_hi) == (0, len(offsets) - 1):
            assert any(c.is_identity(v) for v in want_conts.values())
            assert sum(c.is_identity(v) for v in want_sums.values()) >= 3
            span = runs[1][0]       # the cut range begins at the spanning bucket
            assert len({s for s, b in want_cb.items() if b == span}) >= 3


def test_invalid_arguments_are_refused_before_any_launch():
    grp = G1
    entries, offsets = [0, 1, 2, 3 | NEG, 4, 5], [0, 2, 2, 6]
    ok = dict(kernel=0, rec=PACKED["G1"], entries=entries, offsets=offsets, S=3, b_lo=0, b_hi=3)
    bad = [
        dict(offsets=[0, 4, 2, 6]),             # decreasing
        dict(offsets=[0, 2, 2, 5]),             # does not end at the entry count
        dict(offsets=[1, 2, 2, 6]),             # does not start at 0
        dict(entries=[0, 1, 2, NBASES, 4, 5]),  # a base index past the bases
        dict(entries=[0, 1, 2, NBASES | NEG, 4, 5]),
        dict(S=0),
        dict(b_lo=2, b_hi=2),
        dict(b_lo=2, b_hi=1),
        dict(b_hi=4),                           # past nbt
        dict(b_lo=1, b_hi=2),                   # no entry in the range
        dict(rec=28),
        dict(rec=TABLE["G2"]),
        dict(kernel=1),                         # k_accumulate_g2d is G2's
        dict(kernel=2),
    ]
    for change in bad:
        st, _, _, _ = _launch(grp, **{**ok, **change})
        assert st == INVALID, change
    too_many = [0] * ((1 << 16) + 1)
    st, _, _, _ = _launch(grp, 0, PACKED["G1"], too_many, [0, len(too_many)], 8, 0, 1)
    assert st == INVALID
    assert _fn()(0, 0, 0, None, 1, 24, None, 1, None, 1, 1, 0, 1, None, None, None) == INVALID
