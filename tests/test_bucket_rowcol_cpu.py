"""The row/column bucket reduction's identity on the host (msm_rowcol.h):

    sum_b (b+1) B_b = sum_j (j+1) Col_j + Cn * sum_k k Row_k,   b = k*Cn + j,

with Col and Row computed level by level exactly as the driver launches k_rowcol_sum -- every
level "out[g][j] = sum of Q rows of in" over the rows_in x inner matrices the geometry function
returns -- and the final weighted sums as k_rowcol_final's BT threads x Lb sums take them.  The
geometry comes from the library's own rowcol_geom (bh_selftest_rowcol_geometry), the same function
the driver, the workspace sizing and the host combine's shift read; the group is the integers
mod r, since every operation is linear.  No GPU."""
import ctypes
import os
import random

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R_MOD = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001


@pytest.fixture(scope="module")
def lib():
    lib = ctypes.CDLL(os.path.join(ROOT, "bellman-mpc_amd", "bellman_hip", "libbellman_hip.so"))
    f = lib.bh_selftest_rowcol_geometry
    f.restype = ctypes.c_int
    f.argtypes = [ctypes.c_uint32, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_uint64), ctypes.c_size_t]
    return lib


def geometry(lib, nbr, qlg=3, g2=False):
    buf = (ctypes.c_uint64 * 256)()
    n = lib.bh_selftest_rowcol_geometry(nbr, qlg, int(g2), buf, 256)
    assert n >= 9 + 5 * 2
    w = list(buf[:n])
    g = dict(zip(["lc", "Cn", "R", "ncol", "nrow", "BT", "Lb", "col_points", "row_points"], w[:9]))
    lv = [dict(zip(["rows_in", "rows_out", "inner", "Q", "out_off"], w[9 + 5 * i:14 + 5 * i]))
          for i in range(g["ncol"] + g["nrow"])]
    g["col"], g["row"] = lv[:g["ncol"]], lv[g["ncol"]:]
    assert n == 9 + 5 * len(lv)
    return g


def run_levels(levels, first_in, points):
    """The driver's launches of one job: level i reads level i-1's output (the buckets first)
    and writes rows_out x inner sums at out_off of the job's partial array."""
    part = [None] * points
    src, src_off = first_in, 0
    for l in levels:
        assert l["rows_out"] == -(-l["rows_in"] // l["Q"])
        assert l["out_off"] + l["rows_out"] * l["inner"] <= points
        for g in range(l["rows_out"]):
            for j in range(l["inner"]):
                acc = 0
                for r in range(g * l["Q"], min(g * l["Q"] + l["Q"], l["rows_in"])):
                    acc += src[src_off + r * l["inner"] + j]
                part[l["out_off"] + g * l["inner"] + j] = acc % R_MOD
        src, src_off = part, l["out_off"]
        rows_last = l["rows_out"] * l["inner"]
    return part[src_off:src_off + rows_last]


def final_sums(z, BT, Lb, one_based):
    """k_rowcol_final: thread i owns sums [i*Lb, i*Lb + Lb) (identities past the end), weights
    local index (+1 for the columns), then x_i = acc_i + Lb * (sum of the later threads' runs)."""
    assert BT * Lb >= len(z) and BT & (BT - 1) == 0 and Lb & (Lb - 1) == 0
    at = lambda m: z[m] if m < len(z) else 0
    run = [sum(at(i * Lb + k) for k in range(Lb)) for i in range(BT)]
    acc = [sum((k + one_based) * at(i * Lb + k) for k in range(Lb)) for i in range(BT)]
    x = [acc[i] + Lb * sum(run[i + 1:]) for i in range(BT)]
    return sum(x) % R_MOD, sum(run) % R_MOD


def reduce_range(lib, buckets, qlg=3, g2=False):
    """out[0..2] and the shift for one bucket range, through the library's geometry."""
    g = geometry(lib, len(buckets), qlg, g2)
    assert g["Cn"] == 1 << g["lc"] and g["Cn"] * g["R"] == len(buckets)
    assert g["col"][0]["rows_in"] == g["R"] and g["col"][0]["inner"] == g["Cn"]
    assert g["row"][0]["rows_in"] == len(buckets) and g["row"][0]["inner"] == 1
    col = run_levels(g["col"], buckets, g["col_points"])
    row = run_levels(g["row"], buckets, g["row_points"])
    assert len(col) == g["Cn"] and len(row) == g["R"]
    out0, _ = final_sums(col, g["BT"], g["Lb"], 1)
    out1, out2 = final_sums(row, g["BT"], g["Lb"], 0)
    assert g["BT"] <= (128 if g2 else 256)
    return (out0, out1, out2), g


@pytest.mark.parametrize("qlg", [3, 4])
@pytest.mark.parametrize("nb", [1, 2, 8, 1 << 10, 1 << 11, 1 << 15])
def test_decomposition_equals_the_weighted_bucket_sum(lib, nb, qlg):
    rng = random.Random(nb * 7 + qlg)
    # about a third of the buckets empty: they read as the identity (0)
    buckets = [rng.randrange(R_MOD) if rng.random() > 0.35 else 0 for _ in range(nb)]
    want = sum((b + 1) * v for b, v in enumerate(buckets)) % R_MOD
    for g2 in (False, True):
        (o0, o1, o2), g = reduce_range(lib, buckets, qlg, g2)
        assert (o0 + (o1 << g["lc"])) % R_MOD == want
        assert o2 == sum(buckets) % R_MOD
        # every level takes at most 2^qlg summands per thread
        assert all(l["Q"] <= 1 << qlg for l in g["col"] + g["row"])


def test_splits_cover_square_and_non_square_shapes(lib):
    shapes = {nb: (geometry(lib, nb)["Cn"], geometry(lib, nb)["R"]) for nb in (1, 2, 8, 1 << 10, 1 << 11, 1 << 15, 1 << 19)}
    assert shapes[1] == (1, 1) and shapes[2] == (2, 1) and shapes[8] == (4, 2)
    assert shapes[1 << 10] == (32, 32) and shapes[1 << 11] == (64, 32)
    assert shapes[1 << 19] == (1024, 512)  # the 2^22 proof's c = 20: Cn = the shard granule
    for nb, (cn, r) in shapes.items():
        assert cn * r == nb and cn <= 1024


@pytest.mark.parametrize("nbr,padded", [(2 * 1024, False), (3 * 1024, True), (5 * 1024, True), (171 * 1024, True),
                                        (683 * 1024, True)])
def test_shard_ranges_with_any_number_of_rows(lib, nbr, padded):
    """A bucket shard's range is a multiple of 1024 buckets, not a power of two: the column levels'
    last group is short (padded) wherever Q does not divide the rows."""
    g = geometry(lib, nbr)
    assert g["Cn"] * g["R"] == nbr
    assert any(l["rows_in"] % l["Q"] for l in g["col"]) == padded
    if nbr <= 5 * 1024:
        rng = random.Random(nbr)
        buckets = [rng.randrange(R_MOD) for _ in range(nbr)]
        (o0, o1, _), g = reduce_range(lib, buckets)
        assert (o0 + (o1 << g["lc"])) % R_MOD == sum((b + 1) * v for b, v in enumerate(buckets)) % R_MOD


def test_bucket_shard_of_2p12_combines_with_its_offset(lib):
    """Buckets [1024, 3072) of 2^12: the shard's out[0] + 2^shift out[1] + bk_lo out[2] is its part
    of the window total, and with the two other ranges' parts gives the whole window."""
    rng = random.Random(12)
    nb = 1 << 12
    buckets = [rng.randrange(R_MOD) if rng.random() > 0.5 else 0 for _ in range(nb)]
    want = sum((b + 1) * v for b, v in enumerate(buckets)) % R_MOD
    total = 0
    for lo, hi in ((0, 1024), (1024, 3072), (3072, 4096)):
        (o0, o1, o2), g = reduce_range(lib, buckets[lo:hi])
        part = (o0 + (o1 << g["lc"]) + lo * o2) % R_MOD
        assert part == sum((b + 1) * buckets[b] for b in range(lo, hi)) % R_MOD
        total += part
    assert total % R_MOD == want


def test_all_buckets_empty(lib):
    (o0, o1, o2), _ = reduce_range(lib, [0] * 2048)
    assert (o0, o1, o2) == (0, 0, 0)
