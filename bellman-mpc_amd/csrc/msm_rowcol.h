// Geometry of the row/column bucket reduction of one bucket window, or of a bucket shard's range
// of it (msm_impl.cuh, reduce_range).  Plain host C++: the driver, the workspace sizing, the host
// combine's shift and the host test (bh_selftest_rowcol_geometry,
// tests/test_bucket_rowcol_cpu.py) all read this one function.
//
// Buckets b = 0 .. nbr-1 of a range (bucket b holds digit b+1, plus the range's offset) are laid
// out as R rows of Cn = 2^lc columns, b = k*Cn + j, and
//   sum_b (b+1) B_b = sum_j (j+1) Col_j + Cn * sum_k k Row_k,
//   Col_j = sum_k B_{k,j},  Row_k = sum_j B_{k,j}:
// plain sums, computed by levels of one kernel, "out[g][j] = the sum of Q rows of in[.][j]":
//   column levels: a rows x Cn matrix -> ceil(rows / Q) x Cn (the last group may be short) until
//                  one row is left;
//   row levels:    the same kernel on the flat array as a (count x 1) matrix, count -> count / Q
//                  (Q divides Cn, so no group straddles two rows) until R values are left.
// The final stage (k_rowcol_final) takes the weighted sums of the Cn column and R row sums.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace bh {

constexpr int ROWCOL_MAX_LEVELS = 16;  // 32 bits at qlg >= 2
// log2 of the most summands one thread takes in one level: 8 (16 measured no different in the
// 2^22 proof, profiles/tail_ab_rowcol.txt; 8 has the shorter chains)
constexpr int ROWCOL_QLG = 3;
constexpr int ROWCOL_MAX_LC = 10;  // Cn <= 1024 = BUCKET_SHARD_GRANULE: a shard is whole rows

struct RowColLevel {
  uint32_t rows_in, rows_out, inner, Q;  // in: rows_in x inner, out: rows_out x inner
  size_t out_off;                        // first point of this level's output in its partial array
};

struct RowColGeom {
  int lc;            // log2 Cn: the host adds 2^lc * out[1]
  uint32_t Cn, R;    // columns, rows (R * Cn >= nbr; buckets past nbr read as the identity)
  int ncol, nrow;    // levels (>= 1 each: the first level also maps empty buckets to the identity)
  RowColLevel col[ROWCOL_MAX_LEVELS], row[ROWCOL_MAX_LEVELS];
  size_t col_points, row_points;  // partial-array sizes; the last level's output: Col[Cn], Row[R]
  uint32_t final_threads, final_per_thread;  // k_rowcol_final: BT threads x Lb sums >= max(Cn, R)
};

inline int rowcol_lg2_ceil(uint32_t x) {
  int r = 0;
  while (((uint64_t)1 << r) < x) r++;
  return r;
}

// levels reducing `count` groups-of-rows to one: bits of log2(count) spread evenly over
// ceil(bits / qlg) levels (at most 2^qlg summands per thread and level), larger levels first
inline int rowcol_levels(uint32_t rows, uint32_t inner, int qlg, RowColLevel* lv, size_t* points) {
  const int bits = rowcol_lg2_ceil(rows);
  int n = (bits + qlg - 1) / qlg;
  if (n < 1) n = 1;
  size_t off = 0;
  for (int i = 0; i < n; i++) {
    const int b = bits / n + (i < bits % n ? 1 : 0);
    lv[i].rows_in = rows;
    lv[i].Q = 1u << b;
    lv[i].rows_out = (rows + lv[i].Q - 1) / lv[i].Q;
    lv[i].inner = inner;
    lv[i].out_off = off;
    off += (size_t)lv[i].rows_out * inner;
    rows = lv[i].rows_out;
  }
  *points = off;
  return n;
}

// nbr buckets (a whole window: a power of two; a bucket shard: a multiple of 1024);
// qlg: log2 of the most summands one thread takes in one level (3: 8; at least 2)
inline RowColGeom rowcol_geom(uint32_t nbr, int qlg, bool g2) {
  RowColGeom g;
  if (qlg < 2) qlg = 2;
  int lc = (rowcol_lg2_ceil(nbr) + 1) / 2;
  if (lc > ROWCOL_MAX_LC) lc = ROWCOL_MAX_LC;
  g.lc = lc;
  g.Cn = 1u << lc;
  g.R = (nbr + g.Cn - 1) / g.Cn;
  g.ncol = rowcol_levels(g.R, g.Cn, qlg, g.col, &g.col_points);
  // rows: R * Cn values, Cn -> 1 per row; as a flat (count x 1) matrix
  size_t off = 0;
  const int bits = lc;
  int n = (bits + qlg - 1) / qlg;
  if (n < 1) n = 1;
  uint32_t per_row = g.Cn;
  for (int i = 0; i < n; i++) {
    const int b = bits / n + (i < bits % n ? 1 : 0);
    g.row[i].rows_in = g.R * per_row;
    g.row[i].Q = 1u << b;
    per_row >>= b;
    g.row[i].rows_out = g.R * per_row;
    g.row[i].inner = 1;
    g.row[i].out_off = off;
    off += g.row[i].rows_out;
  }
  g.nrow = n;
  g.row_points = off;
  // final stage: one workgroup per weighted sum, at most 256 (G1) / 128 (G2) threads
  const uint32_t m = g.Cn > g.R ? g.Cn : g.R, bmax = g2 ? 128u : 256u;
  uint32_t lb = 1, t = 1;
  while ((uint64_t)bmax * lb < m) lb <<= 1;
  while ((uint64_t)t * lb < m) t <<= 1;
  g.final_threads = t;
  g.final_per_thread = lb;
  return g;
}

}  // namespace bh
