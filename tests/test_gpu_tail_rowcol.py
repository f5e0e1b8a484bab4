"""The row/column bucket reduction (msm_rowcol.h; k_cont_fold, k_rowcol_sum, k_rowcol_final) on the
device: plain multiexps at forced windows against the oracle's golden results (bucket counts
below one full level, square and non-square splits, the largest window), level sums that meet a
doubling and the identity, sparse buckets at the smallest window-table size (2^17 constraints),
and bucket shards (the out[2] row-sum path).  Bit-exact, as every group result."""
import ctypes
import random

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
# 2^17 constraints, 2^17 - 1 aux scalars: the smallest power-of-two chain whose aux multiexps use
# window tables and bucket shards (a multiexp needs 2^16 scalars for a table, TABLE_MIN_USED; a
# 2^16-constraint chain has 2^16 - 1 and stays on plain windows)
ROUNDS_TABLES = (1 << 16) - 1


def _bh():
    import bellman_hip as bh
    return bh


def _columns(nb):
    """Cn of the library's geometry for nb buckets."""
    f = _bh().lib().bh_selftest_rowcol_geometry
    f.restype = ctypes.c_int
    f.argtypes = [ctypes.c_uint32, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_uint64), ctypes.c_size_t]
    buf = (ctypes.c_uint64 * 256)()
    assert f(nb, 3, 0, buf, 256) > 0
    return int(buf[1]), int(buf[2])


@pytest.mark.parametrize("group,c", [("g1", 4), ("g1", 5), ("g1", 11), ("g1", 12), ("g1", 16), ("g2", 4), ("g2", 12)])
def test_plain_multiexp_at_forced_windows(ctx, golden, group, c):
    """2^(c-1) buckets per window: 8 and 16 (fewer than one level's 8 summands per axis), 1024
    (square), 2048 (non-square) and 32768 (the largest plain window), every window a grid row."""
    bh = _bh()
    data = golden["msm_" + group]
    case = [k for k in data["cases"] if "(all bases)" in k["note"]][0]
    bases = bh.Bases(ctx, bh.BH_G1 if group == "g1" else bh.BH_G2, b"".join(bytes.fromhex(h) for h in data["bases"]))
    exps = [int(x, 16) for x in case["exps"]]
    ctx.set_window(c)
    try:
        assert bh.multiexp(ctx, bases, 0, None, exps).hex() == case["point"]
    finally:
        ctx.set_window(0)


@pytest.mark.parametrize("g2", [False, True])
@pytest.mark.parametrize("c", [11, 12])
def test_equal_and_opposite_row_and_column_partials(ctx, g2, c):
    """P, -P and P in different buckets of one column and of one row (small scalars: window 0's
    digit is the scalar, bucket = scalar - 1), so the level sums add P + (-P) (the identity, then
    + P), P + P (a doubling) inside one thread's group and between two groups' partial sums.
    Compared with the oracle's multiexp."""
    bh = _bh()
    from oracle import bellman as bm
    from oracle import bls12_381 as bls
    E = bm.BLS12_381
    G = E.G2 if g2 else E.G1
    gen = bls.G2.generator() if g2 else bls.G1.generator()
    enc = bls.g2_to_uncompressed if g2 else bls.g1_to_uncompressed
    aff = lambda k: G.to_affine(G.mul(gen, k % R))
    P, N, Q = aff(11), aff(R - 11), aff(29)
    cn, rows = _columns(1 << (c - 1))
    assert cn >= 16 and rows >= 8
    b = lambda k, j: k * cn + j + 1  # the scalar whose window-0 digit lands in row k, column j
    pts, exps = [], []
    for bucket, p in [
            (b(0, 5), P), (b(1, 5), N), (b(2, 5), P),      # column 5: P - P + P
            (b(0, 6), P), (b(1, 6), P),                    # column 6: P + P inside one group
            (b(0, 7), P), (b(rows - 1, 7), P),             # column 7: P + P between two groups' partials
            (b(3, 0), P), (b(3, 1), N), (b(3, 2), P),      # row 3: P - P + P
            (b(4, 0), P), (b(4, 1), P),                    # row 4: P + P inside one group
            (b(5, 0), P), (b(5, cn - 1), P),               # row 5: P + P between two groups' partials
            (b(6, 3), Q), (b(7, 3), Q), (b(6, 4), N)]:     # equal column sums and a mixed row
        pts.append(p)
        exps.append(bucket)
    rng = random.Random(31 + c)
    for _ in range(6):  # full-size scalars: every other window populated too
        pts.append(aff(rng.randrange(1, R)))
        exps.append(rng.randrange(R))
    assert max(exps[:17]) < 1 << (c - 1)
    bases = bh.Bases(ctx, bh.BH_G2 if g2 else bh.BH_G1, b"".join(enc(p) for p in pts))
    want = enc(G.to_affine(bm.multiexp(E, G, pts, 0, None, exps)))
    ctx.set_window(c)
    try:
        assert bh.multiexp(ctx, bases, 0, None, exps) == want
    finally:
        ctx.set_window(0)
    assert bh.multiexp(ctx, bases, 0, None, exps) == want


def _upload(ctx, asg):
    bh = _bh()
    h = bh.ctypes.c_void_p()
    bh._check(bh._lib.bh_witness_upload(ctx.h, bh._ptr(asg["a"]), bh._ptr(asg["b"]), bh._ptr(asg["c"]),
                                        asg["a"].shape[0], bh._ptr(asg["inputs"]), asg["inputs"].shape[0],
                                        bh._ptr(asg["aux"]), asg["aux"].shape[0], bh._ptr(asg["a_aux_density"]),
                                        bh._ptr(asg["b_input_density"]), bh._ptr(asg["b_aux_density"]),
                                        bh.ctypes.byref(h)), "bh_witness_upload")
    return bh.Witness(ctx, h, asg["a"].shape[0])


def _tables_used(ctx):
    """Multiexps of the context's last proof that ran on a window table (one shared bucket window)."""
    return int(ctx.last_stats()[10])


def test_sparse_buckets_at_the_smallest_table_size(ctx, monkeypatch):
    """Every aux scalar one of 3 fixed values at 2^17 constraints: all but a few dozen buckets of
    the shared window are empty (they read as the identity) and the populated ones span many
    accumulation segments (the continuation folds).  Not a satisfying assignment, so the proof
    is not valid, but tables, plain windows, two scalar shards and 2 and 8 bucket shards compute
    the same multiexps byte for byte (the path of test_degenerate_scalars_tables_plain_and_shards_agree)."""
    bh = _bh()
    params = bh.Parameters.chain(ctx, ROUNDS_TABLES)
    asg = bh.chain_assignment(ROUNDS_TABLES)
    rng = np.random.default_rng(16)
    values = bh.fr_to_mont([3, 0x1234567 ** 9 % R, R - 2])
    asg["aux"][:] = values[rng.integers(0, 3, size=asg["aux"].shape[0])]
    w = _upload(ctx, asg)
    ctx.set_tables(False)
    try:
        plain = bh.prove_witness(ctx, params, w, 27134, 17146)
    finally:
        ctx.set_tables(True)
    assert _tables_used(ctx) == 0
    params.prepare(w)
    assert bh.prove_witness(ctx, params, w, 27134, 17146) == plain
    assert _tables_used(ctx) >= 2  # h and l at least: the shared-window reduction ran
    scalar_parts = b"".join(bh.prove_witness_partial(ctx, params, w, k, 2) for k in range(2))
    assert bh.proof_from_partials(params.vk_bytes(), scalar_parts, 2, 27134, 17146) == plain
    monkeypatch.setenv("BH_SHARD_BUCKETS", "1")
    for n in (2, 8):
        parts = b"".join(bh.prove_witness_partial(ctx, params, w, k, n) for k in range(n))
        assert _tables_used(ctx) >= 1
        assert bh.proof_from_partials(params.vk_bytes(), parts, n, 27134, 17146) == plain
        if n == 2:  # split by bucket range, not by scalar range: other partial sums, the same total
            assert parts != scalar_parts


@pytest.mark.parametrize("nshards", [2, 8])
def test_bucket_shards_of_the_smallest_table_proof(ctx, monkeypatch, nshards):
    """The honest 2^17-constraint proof split into 2 and 8 bucket ranges (each rank's reduction
    returns out[0..2]; the host adds bk_lo times the range's plain row sum out[2]) equals the
    single-device proof, and its partial sums differ from the scalar shards' (the ranges were
    taken)."""
    bh = _bh()
    params = bh.Parameters.chain(ctx, ROUNDS_TABLES)
    w = bh.Witness.chain(ctx, ROUNDS_TABLES)
    params.prepare(w)
    single = bh.prove_witness(ctx, params, w, 27134, 17146)
    assert _tables_used(ctx) >= 2
    scalar_parts = b"".join(bh.prove_witness_partial(ctx, params, w, k, nshards) for k in range(nshards))
    assert bh.proof_from_partials(params.vk_bytes(), scalar_parts, nshards, 27134, 17146) == single
    monkeypatch.setenv("BH_SHARD_BUCKETS", "1")
    params.prepare(w, nshards)
    parts = b"".join(bh.prove_witness_partial(ctx, params, w, k, nshards) for k in range(nshards))
    assert _tables_used(ctx) >= 1
    assert parts != scalar_parts
    assert bh.proof_from_partials(params.vk_bytes(), parts, nshards, 27134, 17146) == single
