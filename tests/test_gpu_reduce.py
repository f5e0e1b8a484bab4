"""The back half of a multiexp -- continuation folds and bucket reduction -- on entry lists whose
spans the test chooses, against the oracle's group.

bh_selftest_reduce (csrc/selftest.hip, msm_selftest_reduce in csrc/msm_impl.cuh) puts a
caller-ordered entry list into a workspace as a sort would have left it and runs what a multiexp
runs: msm_accumulate (k_accumulate_pf), max_span over the reduced range and msm_back, i.e.
reduce_range: k_cont_seq, k_cont_long or k_cont_treeF, then k_cont_fold, k_rowcol_sum and
k_rowcol_final.  Which kernel folds a bucket depends on how many accumulation segments it spans
and on the longest span of the range; tests/reduce_layout.py builds lists with a bucket on each
side of every threshold (tests/test_reduce_layout_cpu.py holds the lists to that).  mode 0 hands
max_span's device words to the kernels (the prover's and the job queue's tails), mode 1 passes no
span words (msm_window_sums: every level of k_cont_treeF).

Per list, range and mode, exactly, as group elements:
  (a) bucket_sums[b] = the sum of the bucket's entries, for every non-empty bucket of the range
      (the identity as the all-zero point, coordinates inside the bounds of curve.cuh);
  (b) every other bucket, and every bucket of the range that lies in one segment, is byte for
      byte what bh_selftest_accumulate leaves on the same input;
  (c) out[0] + 2^lc out[1] (one shared window) or each of the Wb totals = sum (b + 1) B_b;
  (d) a proper range of a window (the bucket-shard path): out[2] = sum B_b.
"""
import ctypes
import functools

import numpy as np
import pytest

import reduce_layout as rl
import test_gpu_accumulate as acc
from accumulate_model import bucket_totals, range_sums
from xyzz_device import G1, G2, check_point, point_values

pytestmark = pytest.mark.gpu

GROUPS = {"G1": G1, "G2": G2}
NEG, INVALID = acc.NEG, acc.INVALID


def _fn():
    import bellman_hip as bh
    f = bh.lib().bh_selftest_reduce
    P, Z, U, I = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint32, ctypes.c_int
    f.restype = I
    f.argtypes = [I, I, I, P, Z, U, P, Z, P, Z, U, U, U, U, U, P, P, P]
    return f


def _reduce(grp, mode, rec, entries, offsets, S, Wb, NB, b0, nbr, nbt=None):
    """bh_selftest_reduce -> (status, bucket_sums[nbt], out points, lc)"""
    nbt = len(offsets) - 1 if nbt is None else nbt
    bases = acc._records(grp, rec)
    ent = np.array(entries, dtype=np.uint32)
    off = np.array(offsets, dtype=np.uint32)
    sums = np.zeros((max(nbt, 1), grp.pw), dtype=np.uint32)
    out = np.full((max(Wb, 3), grp.pw), 0xFFFFFFFF, dtype=np.uint32)
    lc = ctypes.c_int(-1)
    st = _fn()(0, 0 if grp is G1 else 1, mode, bases.ctypes.data, len(bases), rec, ent.ctypes.data, len(ent),
               off.ctypes.data, nbt, S, Wb, NB, b0, nbr, sums.ctypes.data, out.ctypes.data, ctypes.byref(lc))
    return st, sums, out, lc.value


def _point(grp, words, tag):
    """a device XYZZ point -> the oracle's Jacobian point (check_point's conditions on the way)"""
    F, c = grp.F, grp.curve
    X, Y, ZZ, ZZZ = (grp.demont(e) for e in point_values(grp, [int(w) for w in words]))
    if F.is_zero(ZZ):
        check_point(grp, words, c.identity, tag=tag)
        return c.identity
    p = c.from_affine((F.mul(X, F.inv(ZZ)), F.mul(Y, F.inv(ZZZ))))
    check_point(grp, words, p, tag=tag)
    assert c.on_curve_affine(c.to_affine(p)), ("not on the curve", tag)
    return p


@functools.lru_cache(maxsize=None)
def _model(name, kind, S):
    """the list, every bucket's sum, and per range the window totals (sum (b + 1) B_b, sum B_b)"""
    c = GROUPS[name].curve
    plan = rl.build(kind, S, rl.BLOCK[name])
    jac = [c.from_affine(a) for a in acc._bases(name)]
    values = [c.neg(jac[e & ~NEG]) if e & NEG else jac[e & ~NEG] for e in plan.entries]
    totals = bucket_totals(values, plan.offsets, 0, plan.Wb * plan.NB, c.add, c.identity)
    windows = {(b0, nbr): [range_sums(totals, b0 + w * nbr, nbr, c.add, c.identity) for w in range(plan.Wb)]
               for b0, nbr in plan.ranges}
    return plan, totals, windows


def _check(name, kind, S, modes=(0, 1)):
    grp = GROUPS[name]
    c = grp.curve
    plan, totals, windows = _model(name, kind, S)
    rec = (acc.PACKED if S == 3 else acc.TABLE)[name]       # both record forms, one per S
    nbt = plan.Wb * plan.NB
    for b0, nbr in plan.ranges:
        lo, hi = b0, b0 + plan.Wb * nbr
        st, before, _, _ = acc._launch(grp, 0, rec, plan.entries, plan.offsets, S, lo, hi)
        assert st == 0
        for mode in modes:
            tag = (kind, S, b0, nbr, mode)
            st, sums, out, lc = _reduce(grp, mode, rec, plan.entries, plan.offsets, S, plan.Wb, plan.NB, b0, nbr)
            assert st == 0, tag
            for b in range(nbt):
                if lo <= b < hi and plan.ncont(b):
                    check_point(grp, sums[b], totals[b], zero_form=c.is_identity(totals[b]),
                                tag=tag + ("bucket", b, "ncont", plan.ncont(b)))                        # (a)
                else:
                    assert (sums[b] == before[b]).all(), tag + ("bucket", b, "changed")                  # (b)
                    if lo <= b < hi and b in totals:
                        check_point(grp, sums[b], totals[b], zero_form=c.is_identity(totals[b]), tag=tag + (b,))
                    else:
                        assert (sums[b] == 0xFFFFFFFF).all()
            want = windows[(b0, nbr)]
            if plan.Wb > 1:
                for w in range(plan.Wb):
                    assert c.eq(_point(grp, out[w], tag + ("out", w)), want[w][0]), tag + ("window", w)  # (c)
                continue
            o = [_point(grp, out[i], tag + ("out", i)) for i in range(2)]
            assert lc == min(10, ((nbr - 1).bit_length() + 1) // 2), tag     # rowcol_geom (msm_rowcol.h)
            assert c.eq(c.add(o[0], c.mul(o[1], 1 << lc)), want[0][0]), tag + ("weighted sum",)         # (c)
            if (b0, nbr) != (0, plan.NB):
                assert c.eq(_point(grp, out[2], tag + ("out", 2)), want[0][1]), tag + ("plain sum",)     # (d)


@pytest.mark.parametrize("S", [3, 8])
@pytest.mark.parametrize("kind", ["fold", "seq", "long"])
def test_each_longest_span_regime_g1(kind, S):
    _check("G1", kind, S)


@pytest.mark.parametrize("S", [3, 8])
@pytest.mark.parametrize("kind", ["fold_cut", "seq_cut"])
def test_a_cut_range_leaves_the_long_buckets_beside_it_alone_g1(kind, S):
    _check("G1", kind, S)


@pytest.mark.parametrize("S", [3, 8])
def test_three_windows_of_a_plain_multiexp_g1(S):
    _check("G1", "plain", S)


@pytest.mark.parametrize("S", [3, 8])
def test_a_bucket_shard_range_of_a_sparse_window_g1(S):
    _check("G1", "shard", S)


@pytest.mark.parametrize("S", [3, 8])
@pytest.mark.parametrize("mode", [0, 1], ids=["span_words", "tree"])
def test_thresholds_and_exceptional_partials_g2(mode, S):
    _check("G2", "long", S, modes=(mode,))


@pytest.mark.parametrize("S", [3, 8])
@pytest.mark.parametrize("kind", ["fold", "seq"])
def test_the_shorter_regimes_g2(kind, S):
    _check("G2", kind, S)


def test_invalid_arguments_are_refused_before_any_launch():
    grp = G1
    entries, offsets = [0, 1, 2, 3 | NEG, 4, 5], [0, 2, 2, 6, 6]
    ok = dict(mode=0, rec=acc.PACKED["G1"], entries=entries, offsets=offsets, S=3, Wb=1, NB=4, b0=0, nbr=4)
    assert _reduce(grp, **ok)[0] == 0
    big = [0] + [6] * 2048                              # 2048 buckets, six entries in the first
    assert _reduce(grp, **{**ok, **dict(offsets=big, NB=2048, b0=0, nbr=1024)})[0] == 0
    bad = [
        dict(offsets=[0, 4, 2, 6, 6]),                  # decreasing
        dict(offsets=[0, 2, 2, 5, 5]),                  # does not end at the entry count
        dict(offsets=[1, 2, 2, 6, 6]),                  # does not start at 0
        dict(entries=[0, 1, 2, acc.NBASES, 4, 5]),      # a base index past the bases
        dict(entries=[0, 1, 2, acc.NBASES | NEG, 4, 5]),
        dict(S=0),
        dict(rec=28),
        dict(rec=acc.TABLE["G2"]),
        dict(mode=2),                                   # the host-decided modes are not exposed
        dict(mode=-1),
        dict(NB=3, nbr=3, offsets=[0, 2, 2, 6]),        # a whole window that is no power of two
        dict(b0=0, nbr=3),                              # a range that is neither
        dict(offsets=big, NB=2048, b0=0, nbr=1536),     # a shard range: no multiple of 1024
        dict(Wb=2, NB=2, nbr=1),                        # several windows: whole windows only
        dict(Wb=2, NB=2, b0=1, nbr=1),
        dict(Wb=2, NB=4, nbr=4),                        # Wb * NB != nbt
        dict(Wb=1, NB=2, nbr=2),
        dict(b0=2, nbr=4),                              # past the window
        dict(b0=4, nbr=1),
        dict(nbr=0),
        dict(b0=1, nbr=1),                              # no entry in the range
        dict(b0=3, nbr=1),
        dict(Wb=0, NB=4),
        dict(Wb=256, NB=1, nbr=1, offsets=[0] + [6] * 256),          # more windows than the outputs hold
    ]
    for change in bad:
        assert _reduce(grp, **{**ok, **change})[0] == INVALID, change
    too_many = [0] * ((1 << 16) + 1)
    assert _reduce(grp, **{**ok, **dict(entries=too_many, offsets=[0, len(too_many)], NB=1, nbr=1)})[0] == INVALID
    assert _reduce(grp, **{**ok, **dict(offsets=[0] + [6] * (1 << 17), NB=1 << 17, nbr=1 << 17)})[0] == INVALID
    lc = ctypes.c_int(0)
    assert _fn()(0, 0, 0, None, 1, 24, None, 1, None, 1, 1, 1, 1, 0, 1, None, None, ctypes.byref(lc)) == INVALID
    assert _fn()(0, 2, 0, None, 1, 24, None, 1, None, 1, 1, 1, 1, 0, 1, None, None, None) == INVALID
