// Groth16 parameter generation for any R1CS on the device: a KeypairAssembly
// (generator.rs:44-156) resident in HBM as three column-compressed matrices, and the classic
// generate_parameters (generator.rs:241-634 without the fork's MPC asserts, as
// oracle/bellman.py:generate_parameters restates it) running on it.
//
//   k_r1cs_powers    tau^i, i < m                                  (generator.rs:349-360)
//   k_r1cs_segments  pass 1 of the QAP evaluation: one lane per segment of at most R1CS_S terms,
//                    partial = sum coeff * x[row]                  (eval_at_tau, generator.rs:485-499)
//   k_r1cs_columns   pass 2: one lane per column adds its (at most R1CS_S) partials
//   k_r1cs_long      pass 2 for a column of more than R1CS_S partials: one wave per column
//   k_r1cs_ext       e = (beta u + alpha v + w) / gamma|delta, the flags u != 0, v != 0 and the
//                    count of aux e == 0                           (generator.rs:500-510, 582-590)
//   k_r1cs_compact   the identity filter (generator.rs:614-632): non-zero u / v in order, canonical
// The h scalars are one launch_fr_convert of the powers (times (tau^m - 1)/delta, to canonical),
// the Lagrange coefficients the resident ifft of the powers, the flags' prefix msm_common.hip's
// tiled scan, and the points crs.hip's fixed_base_batch.  Field addition is exact, so the order of
// the partial sums does not matter and nothing here is atomic but the one u32 counter.
//
// The prover's side, bh_r1cs_witness: ProvingAssignment's a = A z, b = B z, c = C z (prover.rs:19-53,
// 99-139) as the same two passes over the ROW view of the matrices, which the first call builds from
// the column arrays on the device.
//   k_r1cs_row_keys      per term: its column (a search of the segment starts), hence its matrix and
//                        variable, its row key = matrix * m + row, and the rows' histogram
//   k_r1cs_row_scatter   per term: a slot of its row from the row's cursor
//   k_r1cs_row_segcount / k_r1cs_row_fill   the rows cut into segments as the columns are
//   k_r1cs_row_segments  pass 1 by rows: partial = sum coeff[term] * z[var]   (eval, prover.rs:19-53)
//   k_r1cs_unsatisfied   a_i * b_i != c_i -> the least such i (TestConstraintSystem::which_is_unsatisfied)
// The histogram and the cursors are u32 atomics, so the order of a row's terms differs from build
// to build.  That changes no result: a row's value is a sum in Fr, and field addition is exact.
#include <string.h>

#include <algorithm>
#include <memory>

#include "crs.h"
#include "ntt_common.cuh"
#include "r1cs.h"

using namespace bh;

namespace bh {

// acc + x for acc, x < 2r, kept < 2r
__device__ __forceinline__ DFr fr_acc(const DFr& acc, const DFr& x) {
  return fe_csub<FrCfg, 2>(fe_add<FrCfg>(acc, x));
}
__device__ __forceinline__ DFr ld_const(const FrConst& c) {
  DFr r;
#pragma unroll
  for (int l = 0; l < 9; l++) r.v[l] = c.v[l];
  return r;
}
// device Montgomery (< 2r) -> canonical packed words (x * 2^-261 <= r, as k_scalars_prepare)
__device__ __forceinline__ void st_canonical(uint32_t* out, size_t i, const DFr& x) {
  st_packed(out, i, fe_csub<FrCfg, 1>(fe_from_mont<FrCfg>(x)));
}

__global__ void __launch_bounds__(256) k_r1cs_powers(uint32_t* out, uint32_t n, const uint32_t* lo, const uint32_t* hi,
                                                     int lo_bits) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  st_packed(out, i, pow_factor(lo, hi, lo_bits, i));
}

__global__ void __launch_bounds__(256) k_r1cs_segments(const uint32_t* coeff, const uint32_t* row, const uint32_t* seg,
                                                       uint32_t nseg, const uint32_t* x, uint32_t* part) {
  const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= nseg) return;
  const uint32_t t0 = seg[k], t1 = seg[k + 1];
  DFr acc = fe_zero<FrCfg>();
  for (uint32_t t = t0; t < t1; t++) acc = fr_acc(acc, fe_mul<FrCfg>(ld_packed(coeff, t), ld_packed(x, row[t])));
  st_packed(part, k, acc);
}

__global__ void __launch_bounds__(256) k_r1cs_columns(const uint32_t* colseg, uint32_t ncol, const uint32_t* part,
                                                      uint32_t* y) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= ncol) return;
  const uint32_t p0 = colseg[j], p1 = colseg[j + 1];
  if (p1 - p0 > R1CS_S) return;  // k_r1cs_long's
  DFr acc = fe_zero<FrCfg>();
  for (uint32_t p = p0; p < p1; p++) acc = fr_acc(acc, ld_packed(part, p));
  st_packed(y, j, acc);
}

__global__ void __launch_bounds__(64) k_r1cs_long(const uint32_t* longcols, const uint32_t* colseg,
                                                  const uint32_t* part, uint32_t* y) {
  __shared__ uint32_t s[64 * 9];
  const uint32_t j = longcols[blockIdx.x];
  const uint32_t p0 = colseg[j], p1 = colseg[j + 1];
  const uint32_t lane = threadIdx.x;
  DFr acc = fe_zero<FrCfg>();
  for (uint32_t p = p0 + lane; p < p1; p += 64) acc = fr_acc(acc, ld_packed(part, p));
  for (uint32_t off = 32; off; off >>= 1) {
    if (lane >= off && lane < 2 * off) {
#pragma unroll
      for (int l = 0; l < 9; l++) s[lane * 9 + l] = acc.v[l];
    }
    __syncthreads();
    if (lane < off) {
      DFr o;
#pragma unroll
      for (int l = 0; l < 9; l++) o.v[l] = s[(lane + off) * 9 + l];
      acc = fr_acc(acc, o);
    }
    __syncthreads();
  }
  if (lane == 0) st_packed(y, j, acc);
}

struct ExtConsts {
  FrConst alpha, beta, gamma_inv, delta_inv;  // device Montgomery limbs
};

// y: u | v | w, n each (packed device Montgomery, < 2r)
__global__ void __launch_bounds__(256) k_r1cs_ext(const uint32_t* y, uint32_t n, uint32_t ni, ExtConsts c,
                                                  uint32_t* ext, uint32_t* fu, uint32_t* fv, uint32_t* unconstrained) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  const DFr u = ld_packed(y, j), v = ld_packed(y, (size_t)n + j), w = ld_packed(y, 2 * (size_t)n + j);
  // beta u + alpha v + w < 6r, times an inverse < r: within fe_mul's bound (A * B < 2^6)
  const DFr t = fe_add<FrCfg>(fe_add<FrCfg>(fe_mul<FrCfg>(u, ld_const(c.beta)), fe_mul<FrCfg>(v, ld_const(c.alpha))), w);
  const DFr e = fe_mul<FrCfg>(t, ld_const(j < ni ? c.gamma_inv : c.delta_inv));
  st_canonical(ext, j, e);
  // u, v < 2r as they were stored (fr_acc).  e < 2r by fe_mul's contract (field.cuh): a < A r and
  // b < B r give (a b + m r) / 2^261 with m < 2^261, which is < (A B r / 2^261 + 1) r < 2r when
  // A B r < 2^261; here A = 6, B = 1 and 2^261 / r > 70.  The test is exact: -1, held as
  // r - (2^261 mod r) or that plus r, is not zero (generator.rs:500-510, 582-590, 614-632)
  fu[j] = fr_is_zero_below_2r(u) ? 0u : 1u;
  fv[j] = fr_is_zero_below_2r(v) ? 0u : 1u;
  if (j >= ni && fr_is_zero_below_2r(e)) atomicAdd(unconstrained, 1u);
}

__global__ void __launch_bounds__(256) k_r1cs_compact(const uint32_t* y, const uint32_t* flag, const uint32_t* pos,
                                                      uint32_t n, uint32_t* out) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n || !flag[j]) return;
  st_canonical(out, pos[j], ld_packed(y, j));
}

// ---- the row view (r1cs.h: bh_r1cs::RowView)
// the column of term t: the one j with seg[colseg[j]] <= t < seg[colseg[j + 1]].  Empty columns
// share their successor's start and are never the answer; seg[colseg[0]] = 0 and
// seg[colseg[ncol]] = terms bracket every t
__device__ __forceinline__ uint32_t term_column(const uint32_t* seg, const uint32_t* colseg, uint32_t ncol,
                                                uint32_t t) {
  uint32_t lo = 0, hi = ncol;
  while (hi - lo > 1) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (seg[colseg[mid]] <= t) lo = mid;
    else hi = mid;
  }
  return lo;
}

// n: variables, m: domain size (rows per matrix in the view).  row[t] < m was checked at creation
__global__ void __launch_bounds__(256) k_r1cs_row_keys(const uint32_t* seg, const uint32_t* colseg, uint32_t ncol,
                                                       const uint32_t* row, uint32_t terms, uint32_t n, uint32_t m,
                                                       uint32_t* key, uint32_t* var, uint32_t* hist) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= terms) return;
  const uint32_t col = term_column(seg, colseg, ncol, t);
  const uint32_t k = col / n;
  const uint32_t key_t = k * m + row[t];
  key[t] = key_t;
  var[t] = col - k * n;
  atomicAdd(&hist[key_t], 1u);
}

// cursor: a copy of the rows' first slots; every row hands out exactly its histogram count
__global__ void __launch_bounds__(256) k_r1cs_row_scatter(const uint32_t* key, const uint32_t* var, uint32_t terms,
                                                          uint32_t* cursor, uint32_t* out_term, uint32_t* out_var) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= terms) return;
  const uint32_t p = atomicAdd(&cursor[key[t]], 1u);
  out_term[p] = t;
  out_var[p] = var[t];
}

// cnt[i] = segments of row i, cnt[nrows] = 0 (so that the exclusive scan ends in the total)
__global__ void __launch_bounds__(256) k_r1cs_row_segcount(const uint32_t* rowptr, uint32_t nrows, uint32_t* cnt) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i > nrows) return;
  cnt[i] = i < nrows ? (rowptr[i + 1] - rowptr[i] + R1CS_S - 1) / R1CS_S : 0u;
}

// seg: rowseg[nrows] + 1 entries.  A row of more than R1CS_S segments has more than R1CS_S^2 terms,
// so there are fewer than long_cap = terms / R1CS_S^2 + 1 of them
__global__ void __launch_bounds__(256) k_r1cs_row_fill(const uint32_t* rowptr, const uint32_t* rowseg, uint32_t nrows,
                                                       uint32_t* seg, uint32_t* longrows, uint32_t long_cap,
                                                       uint32_t* nlong) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i > nrows) return;
  const uint32_t s0 = rowseg[i];
  if (i == nrows) {
    seg[s0] = rowptr[nrows];
    return;
  }
  const uint32_t cnt = rowseg[i + 1] - s0, t0 = rowptr[i];
  for (uint32_t s = 0; s < cnt; s++) seg[s0 + s] = t0 + s * R1CS_S;
  if (cnt > R1CS_S) {
    const uint32_t q = atomicAdd(nlong, 1u);
    if (q < long_cap) longrows[q] = i;
  }
}

// pass 1 by rows, the indirect counterpart of k_r1cs_segments: entry p of the view is term[p] of
// the column arrays times variable var[p] of z (packed device Montgomery, < 2r)
__global__ void __launch_bounds__(256) k_r1cs_row_segments(const uint32_t* coeff, const uint32_t* term,
                                                           const uint32_t* var, const uint32_t* seg, uint32_t nseg,
                                                           const uint32_t* z, uint32_t* part) {
  const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= nseg) return;
  const uint32_t p0 = seg[k], p1 = seg[k + 1];
  DFr acc = fe_zero<FrCfg>();
  for (uint32_t p = p0; p < p1; p++)
    acc = fr_acc(acc, fe_mul<FrCfg>(ld_packed(coeff, term[p]), ld_packed(z, var[p])));
  st_packed(part, k, acc);
}

// abc: a | b | c, m each, < 2r.  a b < 2r and c < 2r: the difference (+ 2r) is < 4r; it is brought
// below 2r and tested exactly (ntt_common.cuh: fr_is_zero_below_2r).  A test that took the
// Montgomery form of -1, r - (2^261 mod r), for zero -- as fe_is_zero did for Fr before it bounded
// its k by the multiples of r that fit nine limbs -- would pass precisely a constraint whose c is
// too large by one.
__global__ void __launch_bounds__(256) k_r1cs_unsatisfied(const uint32_t* abc, uint32_t m, uint32_t nc,
                                                          uint32_t* first) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nc) return;
  const DFr ab = fe_mul<FrCfg>(ld_packed(abc, i), ld_packed(abc, (size_t)m + i));
  const DFr d = fe_sub<FrCfg, 2>(ab, ld_packed(abc, 2 * (size_t)m + i));
  if (!fr_is_zero_below_2r(fe_csub<FrCfg, 2>(d))) atomicMin(first, i);
}

void r1cs_kernels(std::vector<KernInfo>& v) {
  v.push_back({"k_r1cs_row_keys", (const void*)k_r1cs_row_keys, 256, 0});
  v.push_back({"k_r1cs_row_scatter", (const void*)k_r1cs_row_scatter, 256, 0});
  v.push_back({"k_r1cs_row_segcount", (const void*)k_r1cs_row_segcount, 256, 0});
  v.push_back({"k_r1cs_row_fill", (const void*)k_r1cs_row_fill, 256, 0});
  v.push_back({"k_r1cs_row_segments", (const void*)k_r1cs_row_segments, 256, 0});
  v.push_back({"k_r1cs_unsatisfied", (const void*)k_r1cs_unsatisfied, 256, 0});
  v.push_back({"k_r1cs_powers", (const void*)k_r1cs_powers, 256, 0});
  v.push_back({"k_r1cs_segments", (const void*)k_r1cs_segments, 256, 0});
  v.push_back({"k_r1cs_columns", (const void*)k_r1cs_columns, 256, 0});
  v.push_back({"k_r1cs_long", (const void*)k_r1cs_long, 64, 0});
  v.push_back({"k_r1cs_ext", (const void*)k_r1cs_ext, 256, 0});
  v.push_back({"k_r1cs_compact", (const void*)k_r1cs_compact, 256, 0});
}

// n canonical scalars on the device (all non-zero) -> packed affine points, in chunks as
// chain.hip's fixed_base_to_srs; everything stream-ordered, the scratch shared by the chunks
template <class C>
bh_status fixed_base_device(bh_ctx* ctx, const bh_srs& tab, const uint32_t* d_sc, size_t n, bh_srs* out) {
  out->ctx = ctx;
  out->group = HostOf<C>::ID;
  out->n = n;
  out->identity_idx.clear();
  constexpr int words = HostOf<C>::WORDS;
  BH_TRY_HIP(out->pts.alloc(std::max<size_t>(n, 1) * words * 4));
  if (!n) return BH_OK;
  const size_t chunk = std::min<size_t>(n, (size_t)1 << 21);
  DevBuf d_xyzz, d_scr;
  BH_TRY_HIP(d_xyzz.alloc(chunk * sizeof(typename C::P)));
  BH_TRY_HIP(d_scr.alloc(chunk * sizeof(typename C::P) / 4 + 64));
  for (size_t base = 0; base < n; base += chunk) {
    const size_t k = std::min(chunk, n - base);
    BH_TRY_HIP(fixed_base_batch<C>(tab.pts.as<uint32_t>(), d_sc + base * 8, k, d_xyzz.p, d_scr.p,
                                   out->pts.as<uint32_t>() + base * words, ctx->stream));
  }
  BH_TRY_HIP(hipStreamSynchronize(ctx->stream));  // the scratch is freed on return
  return BH_OK;
}

template bh_status fixed_base_device<G1Ops>(bh_ctx*, const bh_srs&, const uint32_t*, size_t, bh_srs*);
template bh_status fixed_base_device<G2Ops>(bh_ctx*, const bh_srs&, const uint32_t*, size_t, bh_srs*);

}  // namespace bh

namespace {

inline unsigned nb(size_t n, unsigned bs) { return (unsigned)((n + bs - 1) / bs); }

// raw 29-bit limbs of the integer x < 2^256
FrConst limbs29(const uint64_t raw[4]) {
  FrConst c;
  for (int i = 0; i < 9; i++) {
    const int bit = 29 * i, w = bit >> 6, sh = bit & 63;
    uint64_t lo = raw[w] >> sh;
    if (sh > 35 && w + 1 < 4) lo |= raw[w + 1] << (64 - sh);
    c.v[i] = (uint32_t)(lo & 0x1fffffffu);
  }
  return c;
}
// launch_fr_convert's constant that multiplies a device value by k and leaves it canonical:
// (a 2^261) * k * 2^-261 = a k, so the limbs of the integer k itself
FrConst canonical_times(const Fr& k) {
  uint64_t raw[4];
  fr_to_canonical(k, raw);
  return limbs29(raw);
}
FrConst dev_limbs(const Fr& k) {
  FrConst c;
  fr_to_dev_limbs(k, c.v);
  return c;
}
FrConst from_dev_const() {
  FrConst c;
  memcpy(c.v, FrConv::FROM_DEV, sizeof c.v);
  return c;
}

bool below_r(const uint64_t w[4]) { return !geq_p<4>(w); }

// pass 2: y[j] = the sum of the partials colseg[j] .. colseg[j + 1], for columns or for rows alike
hipError_t sum_partials(const uint32_t* colseg, size_t ncol, const uint32_t* longcols, size_t nlong,
                        const uint32_t* d_part, uint32_t* d_y, hipStream_t st) {
  hipLaunchKernelGGL(k_r1cs_columns, dim3(nb(ncol, 256)), dim3(256), 0, st, colseg, (uint32_t)ncol, d_part, d_y);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  if (nlong) hipLaunchKernelGGL(k_r1cs_long, dim3((unsigned)nlong), dim3(64), 0, st, longcols, colseg, d_part, d_y);
  return hipGetLastError();
}

// the QAP evaluation of every column against d_x (m packed device-Montgomery Fr): d_y receives
// ncol values, d_part is nseg values of scratch.  Enqueued on st.
hipError_t qap_eval(const bh_r1cs* r, const uint32_t* d_x, uint32_t* d_part, uint32_t* d_y, hipStream_t st) {
  if (r->nseg)
    hipLaunchKernelGGL(k_r1cs_segments, dim3(nb(r->nseg, 256)), dim3(256), 0, st, r->coeff.as<uint32_t>(),
                       r->row.as<uint32_t>(), r->seg.as<uint32_t>(), (uint32_t)r->nseg, d_x, d_part);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  return sum_partials(r->colseg.as<uint32_t>(), r->ncol, r->longcols.as<uint32_t>(), r->nlong, d_part, d_y, st);
}

struct Matrix {
  const uint64_t* ptr;
  const uint32_t* row;
  const uint64_t* coeff;
};

}  // namespace

extern "C" {

bh_status bh_r1cs_create(bh_ctx* ctx, size_t num_inputs, size_t num_aux, size_t num_constraints,
                         const uint64_t* a_ptr, const uint32_t* a_row, const uint64_t* a_coeff,
                         const uint64_t* b_ptr, const uint32_t* b_row, const uint64_t* b_coeff,
                         const uint64_t* c_ptr, const uint32_t* c_row, const uint64_t* c_coeff, bh_r1cs** out) {
  if (!ctx || !out || !a_ptr || !b_ptr || !c_ptr || num_inputs == 0) return BH_ERR_INVALID_ARGUMENT;
  if (num_aux > SIZE_MAX - num_inputs || num_constraints > SIZE_MAX - num_inputs) return BH_ERR_INVALID_ARGUMENT;
  const size_t n = num_inputs + num_aux;
  size_t m;
  uint32_t L;
  bh_status s = bh_domain_size(num_constraints + num_inputs, &m, &L);
  if (s) return s;
  const Matrix M[3] = {{a_ptr, a_row, a_coeff}, {b_ptr, b_row, b_coeff}, {c_ptr, c_row, c_coeff}};
  // every index and offset is validated here, before anything is indexed with it
  size_t terms = num_inputs;  // the appended rows' terms
  for (const Matrix& x : M) {
    if (x.ptr[0] != 0) return BH_ERR_INVALID_ARGUMENT;
    for (size_t j = 0; j < n; j++)
      if (x.ptr[j + 1] < x.ptr[j]) return BH_ERR_INVALID_ARGUMENT;
    const uint64_t nnz = x.ptr[n];
    if (nnz && (!x.row || !x.coeff)) return BH_ERR_INVALID_ARGUMENT;
    if (nnz > 0xffffffffull || terms + nnz > 0xffffffffull) return BH_ERR_INVALID_ARGUMENT;  // u32 term offsets
    terms += nnz;
    for (uint64_t t = 0; t < nnz; t++)
      if (x.row[t] >= num_constraints || !below_r(x.coeff + 4 * t)) return BH_ERR_INVALID_ARGUMENT;
  }
  if (3 * (uint64_t)n > 0xffffffffull) return BH_ERR_INVALID_ARGUMENT;  // u32 column indices
  std::unique_ptr<bh_r1cs> r(new bh_r1cs());
  r->device = ctx->device;
  r->ni = num_inputs;
  r->na = num_aux;
  r->nc = num_constraints + num_inputs;
  r->m = m;
  r->L = L;
  r->nnz[0] = a_ptr[n] + num_inputs;
  r->nnz[1] = b_ptr[n];
  r->nnz[2] = c_ptr[n];
  r->terms = terms;
  r->ncol = 3 * n;
  // eval (prover.rs:19-53) calls inc for every term before it looks at the coefficient: a variable is
  // dense in a matrix exactly when the circuit's own column is not empty
  auto dense = [](const uint64_t* ptr, size_t first, size_t count) {
    std::vector<uint64_t> w((count + 63) / 64, 0);
    for (size_t i = 0; i < count; i++)
      if (ptr[first + i + 1] > ptr[first + i]) w[i >> 6] |= 1ull << (i & 63);
    return w;
  };
  r->a_aux_density = dense(a_ptr, num_inputs, num_aux);
  r->b_input_density = dense(b_ptr, 0, num_inputs);
  r->b_aux_density = dense(b_ptr, num_inputs, num_aux);
  // the concatenated term arrays and the segment scheme
  std::vector<uint64_t> hc(terms * 4);
  std::vector<uint32_t> hr(terms), hseg, hcol(r->ncol + 1), hlong;
  hseg.reserve(r->ncol + terms / R1CS_S + 1);
  const Fr one = Fr::one();
  size_t t = 0;
  for (int k = 0; k < 3; k++) {
    for (size_t j = 0; j < n; j++) {
      const size_t col = (size_t)k * n + j;
      const size_t t0 = t;
      const uint64_t lo = M[k].ptr[j], len = M[k].ptr[j + 1] - lo;
      if (len) {
        memcpy(&hc[t * 4], M[k].coeff + 4 * lo, len * 32);
        memcpy(&hr[t], M[k].row + lo, len * 4);
        t += len;
      }
      if (k == 0 && j < num_inputs) {  // input_j * 0 = 0 (generator.rs:276-282)
        memcpy(&hc[t * 4], one.v, 32);
        hr[t] = (uint32_t)(num_constraints + j);
        t++;
      }
      hcol[col] = (uint32_t)hseg.size();
      for (size_t b = t0; b < t; b += R1CS_S) hseg.push_back((uint32_t)b);
      if (hseg.size() - hcol[col] > R1CS_S) hlong.push_back((uint32_t)col);
    }
  }
  hcol[r->ncol] = (uint32_t)hseg.size();
  r->nseg = hseg.size();
  hseg.push_back((uint32_t)terms);
  r->nlong = hlong.size();
  std::lock_guard<std::mutex> lk(ctx->mu);
  BH_TRY_HIP(hipSetDevice(ctx->device));
  BH_TRY_HIP(r->coeff.alloc(terms * 32));
  BH_TRY_HIP(r->row.alloc(terms * 4));
  BH_TRY_HIP(r->seg.alloc(hseg.size() * 4));
  BH_TRY_HIP(r->colseg.alloc(hcol.size() * 4));
  BH_TRY_HIP(r->longcols.alloc(std::max<size_t>(hlong.size(), 1) * 4));
  BH_TRY_HIP(hipMemcpyAsync(r->coeff.p, hc.data(), terms * 32, hipMemcpyHostToDevice, ctx->stream));
  launch_fr_convert(r->coeff.as<uint32_t>(), r->coeff.as<uint32_t>(), terms, fr_to_dev_const(), 0, ctx->stream);
  BH_TRY_HIP(hipGetLastError());
  BH_TRY_HIP(hipMemcpyAsync(r->row.p, hr.data(), terms * 4, hipMemcpyHostToDevice, ctx->stream));
  BH_TRY_HIP(hipMemcpyAsync(r->seg.p, hseg.data(), hseg.size() * 4, hipMemcpyHostToDevice, ctx->stream));
  BH_TRY_HIP(hipMemcpyAsync(r->colseg.p, hcol.data(), hcol.size() * 4, hipMemcpyHostToDevice, ctx->stream));
  if (!hlong.empty())
    BH_TRY_HIP(hipMemcpyAsync(r->longcols.p, hlong.data(), hlong.size() * 4, hipMemcpyHostToDevice, ctx->stream));
  BH_TRY_HIP(hipStreamSynchronize(ctx->stream));  // the host vectors go out of scope
  *out = r.release();
  return BH_OK;
}

bh_status bh_r1cs_free(bh_r1cs* r) {
  if (!r) return BH_OK;
  (void)hipSetDevice(r->device);
  delete r;
  return BH_OK;
}

bh_status bh_r1cs_sizes(const bh_r1cs* r, size_t out[7]) {
  if (!r || !out) return BH_ERR_INVALID_ARGUMENT;
  out[0] = r->ni;
  out[1] = r->na;
  out[2] = r->nc;
  out[3] = r->nnz[0];
  out[4] = r->nnz[1];
  out[5] = r->nnz[2];
  out[6] = R1CS_S;
  return BH_OK;
}

bh_status bh_r1cs_eval(bh_ctx* ctx, const bh_r1cs* r, const uint64_t* x, uint64_t* u_out, uint64_t* v_out,
                       uint64_t* w_out) {
  if (!ctx || !r || !x || !u_out || !v_out || !w_out || r->device != ctx->device) return BH_ERR_INVALID_ARGUMENT;
  std::lock_guard<std::mutex> lk(ctx->mu);
  BH_TRY_HIP(hipSetDevice(ctx->device));
  bh_status s = scratch_check(ctx);
  if (s) return s;
  const size_t n = r->ni + r->na;
  DevBuf d_x, d_part, d_y;
  BH_TRY_HIP(d_x.alloc(r->m * 32));
  BH_TRY_HIP(d_part.alloc(std::max<size_t>(r->nseg, 1) * 32));
  BH_TRY_HIP(d_y.alloc(r->ncol * 32));
  if ((s = upload_fr(ctx, x, r->m, r->m, d_x.as<uint32_t>()))) return s;
  BH_TRY_HIP(hipGetLastError());
  BH_TRY_HIP(qap_eval(r, d_x.as<uint32_t>(), d_part.as<uint32_t>(), d_y.as<uint32_t>(), ctx->stream));
  launch_fr_convert(d_y.as<uint32_t>(), d_y.as<uint32_t>(), r->ncol, from_dev_const(), 1, ctx->stream);
  BH_TRY_HIP(hipGetLastError());
  uint64_t* outs[3] = {u_out, v_out, w_out};
  for (int k = 0; k < 3; k++)
    BH_TRY_HIP(hipMemcpyAsync(outs[k], d_y.as<uint32_t>() + (size_t)k * n * 8, n * 32, hipMemcpyDeviceToHost,
                              ctx->stream));
  BH_TRY_HIP(hipStreamSynchronize(ctx->stream));
  return BH_OK;
}

bh_status bh_generate_parameters(bh_ctx* ctx, const bh_r1cs* r, const uint64_t alpha_w[4], const uint64_t beta_w[4],
                                 const uint64_t gamma_w[4], const uint64_t delta_w[4], const uint64_t tau_w[4],
                                 bh_params** out) {
  if (!ctx || !r || !alpha_w || !beta_w || !gamma_w || !delta_w || !tau_w || !out || r->device != ctx->device)
    return BH_ERR_INVALID_ARGUMENT;
  for (const uint64_t* w : {alpha_w, beta_w, gamma_w, delta_w, tau_w})
    if (!below_r(w)) return BH_ERR_INVALID_ARGUMENT;
  const Fr alpha = fr_from_canonical(alpha_w), beta = fr_from_canonical(beta_w), gamma = fr_from_canonical(gamma_w),
           delta = fr_from_canonical(delta_w), tau = fr_from_canonical(tau_w);
  if (gamma.is_zero() || delta.is_zero()) return BH_ERR_UNEXPECTED_IDENTITY;  // generator.rs:330-345
  const size_t m = r->m, n = r->ni + r->na, ni = r->ni, na = r->na;
  const int L = (int)r->L;
  // z(tau) = tau^m - 1 (generator.rs:362-372).  The deviation from the reference: tau = 0 or
  // tau^m = 1 would make h scalars zero, which the reference writes as identity points and
  // k_fixed_base is not defined for
  Fr tm = tau;
  for (int i = 0; i < L; i++) tm = sqr(tm);
  const Fr zt = sub(tm, Fr::one());
  if (tau.is_zero() || zt.is_zero()) return BH_ERR_INVALID_ARGUMENT;
  const Fr gamma_inv = inv(gamma), delta_inv = inv(delta);
  const Fr hcoeff = mul(zt, delta_inv);
  std::unique_ptr<bh_params> p(new bh_params());
  p->ctx = ctx;
  const Jac<Fp> g1 = crs_g1_gen();
  const Jac<Fp2> g2 = crs_g2_gen();
  const auto t1 = crs_table_g1();
  const auto t2 = crs_table_g2();
  std::vector<uint64_t> ic_sc(ni * 4);
  {
    std::lock_guard<std::mutex> lk(ctx->mu);
    BH_TRY_HIP(hipSetDevice(ctx->device));
    bh_status s = scratch_check(ctx);
    if (s) return s;
    Domain* D;
    if ((s = ctx_domain(ctx, L, &D))) return s;
    hipStream_t st = ctx->stream;
    // powers of tau and the h scalars tau^i (tau^m - 1)/delta, i < m - 1 (generator.rs:349-397)
    DevBuf lo, hi, d_pow, d_tmp, d_h;
    const int lo_bits = (L + 1) / 2;
    if ((s = upload_split_table(ctx, lo, hi, tau, Fr::one(), L, lo_bits))) return s;
    BH_TRY_HIP(d_pow.alloc(m * 32));
    BH_TRY_HIP(d_tmp.alloc(m * 32));
    BH_TRY_HIP(d_h.alloc(std::max<size_t>(m - 1, 1) * 32));
    hipLaunchKernelGGL(k_r1cs_powers, dim3(nb(m, 256)), dim3(256), 0, st, d_pow.as<uint32_t>(), (uint32_t)m,
                       lo.as<uint32_t>(), hi.as<uint32_t>(), lo_bits);
    BH_TRY_HIP(hipGetLastError());
    launch_fr_convert(d_pow.as<uint32_t>(), d_h.as<uint32_t>(), m - 1, canonical_times(hcoeff), 1, st);
    BH_TRY_HIP(hipGetLastError());
    // Lagrange coefficients (generator.rs:400-401), resident
    if ((s = device_ifft(ctx, D, d_pow.as<uint32_t>(), d_tmp.as<uint32_t>()))) return s;
    // u, v, w of every variable (generator.rs:411-510)
    DevBuf d_part, d_y, d_ext, d_flags, d_pos, d_scan, d_a, d_b, d_cnt;
    BH_TRY_HIP(d_part.alloc(std::max<size_t>(r->nseg, 1) * 32));
    BH_TRY_HIP(d_y.alloc(r->ncol * 32));
    BH_TRY_HIP(d_ext.alloc(n * 32));
    BH_TRY_HIP(d_flags.alloc(2 * n * 4));
    BH_TRY_HIP(d_pos.alloc(2 * n * 4));
    BH_TRY_HIP(d_scan.alloc(scan_scratch_words(n) * 4));
    BH_TRY_HIP(d_a.alloc(n * 32));
    BH_TRY_HIP(d_b.alloc(n * 32));
    BH_TRY_HIP(d_cnt.alloc(4));
    BH_TRY_HIP(qap_eval(r, d_pow.as<uint32_t>(), d_part.as<uint32_t>(), d_y.as<uint32_t>(), st));
    BH_TRY_HIP(hipMemsetAsync(d_cnt.p, 0, 4, st));
    uint32_t* fu = d_flags.as<uint32_t>();
    uint32_t* fv = fu + n;
    uint32_t* pu = d_pos.as<uint32_t>();
    uint32_t* pv = pu + n;
    const ExtConsts ec{dev_limbs(alpha), dev_limbs(beta), dev_limbs(gamma_inv), dev_limbs(delta_inv)};
    hipLaunchKernelGGL(k_r1cs_ext, dim3(nb(n, 256)), dim3(256), 0, st, d_y.as<uint32_t>(), (uint32_t)n, (uint32_t)ni,
                       ec, d_ext.as<uint32_t>(), fu, fv, d_cnt.as<uint32_t>());
    BH_TRY_HIP(hipGetLastError());
    // the identity filter (generator.rs:614-632): order kept, inputs first
    exclusive_scan(fu, pu, n, d_scan.as<uint32_t>(), st);
    BH_TRY_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_r1cs_compact, dim3(nb(n, 256)), dim3(256), 0, st, d_y.as<uint32_t>(), fu, pu, (uint32_t)n,
                       d_a.as<uint32_t>());
    BH_TRY_HIP(hipGetLastError());
    exclusive_scan(fv, pv, n, d_scan.as<uint32_t>(), st);
    BH_TRY_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_r1cs_compact, dim3(nb(n, 256)), dim3(256), 0, st, d_y.as<uint32_t>() + n * 8, fv, pv,
                       (uint32_t)n, d_b.as<uint32_t>());
    BH_TRY_HIP(hipGetLastError());
    // lengths, the unconstrained count and the ic scalars: all that crosses back
    uint32_t hw[5] = {0, 0, 0, 0, 0};
    BH_TRY_HIP(hipMemcpyAsync(&hw[0], pu + n - 1, 4, hipMemcpyDeviceToHost, st));
    BH_TRY_HIP(hipMemcpyAsync(&hw[1], fu + n - 1, 4, hipMemcpyDeviceToHost, st));
    BH_TRY_HIP(hipMemcpyAsync(&hw[2], pv + n - 1, 4, hipMemcpyDeviceToHost, st));
    BH_TRY_HIP(hipMemcpyAsync(&hw[3], fv + n - 1, 4, hipMemcpyDeviceToHost, st));
    BH_TRY_HIP(hipMemcpyAsync(&hw[4], d_cnt.p, 4, hipMemcpyDeviceToHost, st));
    BH_TRY_HIP(hipMemcpyAsync(ic_sc.data(), d_ext.p, ni * 32, hipMemcpyDeviceToHost, st));
    BH_TRY_HIP(hipStreamSynchronize(st));
    if (hw[4]) return BH_ERR_UNCONSTRAINED_VARIABLE;  // generator.rs:586-590
    const size_t a_n = (size_t)hw[0] + hw[1], b_n = (size_t)hw[2] + hw[3];
    d_part.release();
    d_y.release();
    d_tmp.release();
    d_pow.release();
    // fixed-base multiplications (generator.rs:374-397, 520-572)
    bh_srs tab1, tab2;
    if ((s = srs_upload_affine(ctx, t1.data(), t1.size(), &tab1))) return s;
    if ((s = srs_upload_affine(ctx, t2.data(), t2.size(), &tab2))) return s;
    if ((s = fixed_base_device<G1Ops>(ctx, tab1, d_h.as<uint32_t>(), m - 1, &p->h))) return s;
    if ((s = fixed_base_device<G1Ops>(ctx, tab1, d_ext.as<uint32_t>() + ni * 8, na, &p->l))) return s;
    if ((s = fixed_base_device<G1Ops>(ctx, tab1, d_a.as<uint32_t>(), a_n, &p->a))) return s;
    if ((s = fixed_base_device<G1Ops>(ctx, tab1, d_b.as<uint32_t>(), b_n, &p->b_g1))) return s;
    if ((s = fixed_base_device<G2Ops>(ctx, tab2, d_b.as<uint32_t>(), b_n, &p->b_g2))) return s;
  }
  // ic and the verifying key on the host (ni points); a zero ic scalar is the identity
  auto g1mul = [&](const uint64_t* c) { return jac_to_affine(jac_mul(g1, c, 4)); };
  auto g2mul = [&](const uint64_t* c) { return jac_to_affine(jac_mul(g2, c, 4)); };
  for (size_t i = 0; i < ni; i++) p->ic.push_back(g1mul(&ic_sc[4 * i]));
  p->alpha_g1 = g1mul(alpha_w);
  p->beta_g1 = g1mul(beta_w);
  p->beta_g2 = g2mul(beta_w);
  p->gamma_g2 = g2mul(gamma_w);
  p->delta_g1 = g1mul(delta_w);
  p->delta_g2 = g2mul(delta_w);
  *out = p.release();
  return BH_OK;
}

}  // extern "C"

namespace {

// The row view of r (r1cs.h), built once per handle on st.  Caller holds ctx->mu and r->rv.mu.
// Scratch while it builds: 8 bytes per term (keys, variables) and three words per row; kept: 8
// bytes per term, one word per row and per row segment.
bh_status row_view(const bh_r1cs* r, hipStream_t st) {
  bh_r1cs::RowView& rv = r->rv;
  if (rv.ready) return BH_OK;
  const size_t terms = r->terms, nrows = 3 * r->m, n = r->ni + r->na;
  if (nrows + 1 > 0xffffffffull) return BH_ERR_INVALID_ARGUMENT;  // u32 row keys
  const size_t long_cap = terms / ((size_t)R1CS_S * R1CS_S) + 1;
  DevBuf d_key, d_var, d_hist, d_rowptr, d_cursor, d_scan;
  BH_TRY_HIP(d_key.alloc(terms * 4));
  BH_TRY_HIP(d_var.alloc(terms * 4));
  BH_TRY_HIP(d_hist.alloc((nrows + 1) * 4));
  BH_TRY_HIP(d_rowptr.alloc((nrows + 1) * 4));
  BH_TRY_HIP(d_cursor.alloc((nrows + 1) * 4));
  BH_TRY_HIP(d_scan.alloc(scan_scratch_words(nrows + 1) * 4 + 64));
  BH_TRY_HIP(rv.term.alloc(terms * 4));
  BH_TRY_HIP(rv.var.alloc(terms * 4));
  BH_TRY_HIP(rv.rowseg.alloc((nrows + 1) * 4));
  BH_TRY_HIP(rv.longrows.alloc(long_cap * 4));
  BH_TRY_HIP(rv.words.alloc(2 * 4));
  uint32_t* hist = d_hist.as<uint32_t>();
  uint32_t* rowptr = d_rowptr.as<uint32_t>();
  // rows' histogram -> first slots -> scatter through per-row cursors
  BH_TRY_HIP(hipMemsetAsync(hist, 0, (nrows + 1) * 4, st));
  BH_TRY_HIP(hipMemsetAsync(rv.words.p, 0, 2 * 4, st));
  hipLaunchKernelGGL(k_r1cs_row_keys, dim3(nb(terms, 256)), dim3(256), 0, st, r->seg.as<uint32_t>(),
                     r->colseg.as<uint32_t>(), (uint32_t)r->ncol, r->row.as<uint32_t>(), (uint32_t)terms, (uint32_t)n,
                     (uint32_t)r->m, d_key.as<uint32_t>(), d_var.as<uint32_t>(), hist);
  BH_TRY_HIP(hipGetLastError());
  exclusive_scan(hist, rowptr, nrows + 1, d_scan.as<uint32_t>(), st);
  BH_TRY_HIP(hipGetLastError());
  BH_TRY_HIP(hipMemcpyAsync(d_cursor.p, rowptr, (nrows + 1) * 4, hipMemcpyDeviceToDevice, st));
  hipLaunchKernelGGL(k_r1cs_row_scatter, dim3(nb(terms, 256)), dim3(256), 0, st, d_key.as<uint32_t>(),
                     d_var.as<uint32_t>(), (uint32_t)terms, d_cursor.as<uint32_t>(), rv.term.as<uint32_t>(),
                     rv.var.as<uint32_t>());
  BH_TRY_HIP(hipGetLastError());
  // segments per row (the histogram's buffer is free again), their scan, then the fill
  hipLaunchKernelGGL(k_r1cs_row_segcount, dim3(nb(nrows + 1, 256)), dim3(256), 0, st, rowptr, (uint32_t)nrows, hist);
  BH_TRY_HIP(hipGetLastError());
  exclusive_scan(hist, rv.rowseg.as<uint32_t>(), nrows + 1, d_scan.as<uint32_t>(), st);
  BH_TRY_HIP(hipGetLastError());
  uint32_t nseg = 0, nlong = 0;
  BH_TRY_HIP(hipMemcpyAsync(&nseg, rv.rowseg.as<uint32_t>() + nrows, 4, hipMemcpyDeviceToHost, st));
  BH_TRY_HIP(hipStreamSynchronize(st));  // the segment array is sized by the count
  BH_TRY_HIP(rv.seg.alloc(((size_t)nseg + 1) * 4));
  hipLaunchKernelGGL(k_r1cs_row_fill, dim3(nb(nrows + 1, 256)), dim3(256), 0, st, rowptr, rv.rowseg.as<uint32_t>(),
                     (uint32_t)nrows, rv.seg.as<uint32_t>(), rv.longrows.as<uint32_t>(), (uint32_t)long_cap,
                     rv.words.as<uint32_t>());
  BH_TRY_HIP(hipGetLastError());
  BH_TRY_HIP(hipMemcpyAsync(&nlong, rv.words.p, 4, hipMemcpyDeviceToHost, st));
  BH_TRY_HIP(hipStreamSynchronize(st));  // the scratch is freed on return
  if (nlong > long_cap) return BH_ERR_HIP;  // (cannot happen: see k_r1cs_row_fill)
  rv.nrows = nrows;
  rv.nseg = nseg;
  rv.nlong = nlong;
  rv.ready = true;
  return BH_OK;
}

// a | b | c = the rows' sums of the ready row view against z (n packed device-Montgomery Fr), d_part
// rv.nseg values of scratch: every one of the 3 m rows is written, the empty ones (nc .. m of each
// matrix) with zero.  Enqueued on st; the caller holds r->rv.mu
hipError_t rows_product(const bh_r1cs* r, const uint32_t* d_z, uint32_t* d_part, uint32_t* d_abc, hipStream_t st) {
  const bh_r1cs::RowView& rv = r->rv;
  if (rv.nseg)
    hipLaunchKernelGGL(k_r1cs_row_segments, dim3(nb(rv.nseg, 256)), dim3(256), 0, st, r->coeff.as<uint32_t>(),
                       rv.term.as<uint32_t>(), rv.var.as<uint32_t>(), rv.seg.as<uint32_t>(), (uint32_t)rv.nseg, d_z,
                       d_part);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  return sum_partials(rv.rowseg.as<uint32_t>(), rv.nrows, rv.longrows.as<uint32_t>(), rv.nlong, d_part, d_abc, st);
}

}  // namespace

namespace bh {

bh_status r1cs_powers_device(bh_ctx* ctx, const Fr& x, size_t n, uint32_t* d_out) {
  if (!n) return BH_OK;
  int L = 0;
  while (((size_t)1 << L) < n) L++;
  const int lo_bits = (L + 1) / 2;
  DevBuf lo, hi;
  if (bh_status s = upload_split_table(ctx, lo, hi, x, Fr::one(), L, lo_bits)) return s;
  hipLaunchKernelGGL(k_r1cs_powers, dim3(nb(n, 256)), dim3(256), 0, ctx->stream, d_out, (uint32_t)n,
                     lo.as<uint32_t>(), hi.as<uint32_t>(), lo_bits);
  BH_TRY_HIP(hipGetLastError());
  BH_TRY_HIP(hipStreamSynchronize(ctx->stream));  // the tables are freed on return
  return BH_OK;
}

hipError_t r1cs_eval_device(const bh_r1cs* r, const uint32_t* d_x, uint32_t* d_part, uint32_t* d_y, hipStream_t st) {
  return qap_eval(r, d_x, d_part, d_y, st);
}

bh_status r1cs_rows_device(const bh_r1cs* r, const uint32_t* d_z, DevBuf* part, uint32_t* d_abc, hipStream_t st) {
  std::lock_guard<std::mutex> rlk(r->rv.mu);
  if (bh_status s = row_view(r, st)) return s;
  BH_TRY_HIP(part->alloc(std::max<size_t>(r->rv.nseg, 1) * 32));
  BH_TRY_HIP(rows_product(r, d_z, part->as<uint32_t>(), d_abc, st));
  return BH_OK;
}

}  // namespace bh

extern "C" {

bh_status bh_r1cs_witness(bh_ctx* ctx, const bh_r1cs* r, const uint64_t* input_assignment,
                          const uint64_t* aux_assignment, size_t* first_unsatisfied, bh_witness** out) {
  if (!ctx || !r || !out || !input_assignment || (r->na && !aux_assignment) || r->device != ctx->device)
    return BH_ERR_INVALID_ARGUMENT;
  const size_t ni = r->ni, na = r->na, n = ni + na, nc = r->nc, m = r->m;
  for (size_t i = 0; i < ni; i++)
    if (!below_r(input_assignment + 4 * i)) return BH_ERR_INVALID_ARGUMENT;
  for (size_t i = 0; i < na; i++)
    if (!below_r(aux_assignment + 4 * i)) return BH_ERR_INVALID_ARGUMENT;
  std::lock_guard<std::mutex> lk(ctx->mu);
  BH_TRY_HIP(hipSetDevice(ctx->device));
  bh_status s = scratch_check(ctx);
  if (s) return s;
  // one stream for all of it, as bh_witness_upload: the copy stream, synchronised before returning
  hipStream_t st = ctx->h2d;
  std::lock_guard<std::mutex> rlk(r->rv.mu);
  if ((s = row_view(r, st))) return s;
  const bh_r1cs::RowView& rv = r->rv;
  std::unique_ptr<bh_witness> w(new bh_witness());
  if ((s = witness_host(ctx, w.get(), nc, input_assignment, ni, aux_assignment, na, r->a_aux_density.data(),
                        r->b_input_density.data(), r->b_aux_density.data())))
    return s;
  if (w->m != m) return BH_ERR_INVALID_ARGUMENT;
  w->raw = false;
  if ((s = witness_density_upload(w.get(), st))) return s;
  // z = [inputs, aux] in device Montgomery for the product; the witness's own copies canonical, as
  // the multiexps read them (scalars_prepare, like bh_witness_upload).  The context's staging
  // buffers are free under ctx->mu: the partial sums and z need nothing of their own
  BH_TRY_HIP(ctx->staging.alloc(std::max<size_t>(rv.nseg, 1) * 32));
  BH_TRY_HIP(ctx->staging2.alloc(n * 32));
  uint32_t* d_part = ctx->staging.as<uint32_t>();
  uint32_t* d_z = ctx->staging2.as<uint32_t>();
  HostPool& pool = ctx_pool(ctx);
  BH_TRY_HIP(ctx->ring.copy(pool, w->inputs.p, input_assignment, ni * 32, st));
  launch_fr_convert(w->inputs.as<uint32_t>(), d_z, ni, fr_to_dev_const(), 0, st);
  BH_TRY_HIP(hipGetLastError());
  BH_TRY_HIP(scalars_prepare(w->inputs.as<uint32_t>(), w->inputs.as<uint32_t>(), ni, 1, 0, st));
  if (na) {
    BH_TRY_HIP(ctx->ring.copy(pool, w->aux.p, aux_assignment, na * 32, st));
    launch_fr_convert(w->aux.as<uint32_t>(), d_z + ni * 8, na, fr_to_dev_const(), 0, st);
    BH_TRY_HIP(hipGetLastError());
    BH_TRY_HIP(scalars_prepare(w->aux.as<uint32_t>(), w->aux.as<uint32_t>(), na, 1, 0, st));
  }
  // a | b | c = the rows' sums, straight into the witness
  uint32_t* abc = w->abc.as<uint32_t>();
  BH_TRY_HIP(rows_product(r, d_z, d_part, abc, st));
  uint32_t first = 0xffffffffu;
  if (first_unsatisfied) {
    uint32_t* d_first = rv.words.as<uint32_t>() + 1;
    BH_TRY_HIP(hipMemsetAsync(d_first, 0xff, 4, st));
    hipLaunchKernelGGL(k_r1cs_unsatisfied, dim3(nb(nc, 256)), dim3(256), 0, st, abc, (uint32_t)m, (uint32_t)nc,
                       d_first);
    BH_TRY_HIP(hipGetLastError());
    BH_TRY_HIP(hipMemcpyAsync(&first, d_first, 4, hipMemcpyDeviceToHost, st));
  }
  if ((s = witness_index_maps(ctx, w.get(), st))) return s;
  BH_TRY_HIP(hipStreamSynchronize(st));
  if (first_unsatisfied) *first_unsatisfied = first == 0xffffffffu ? SIZE_MAX : (size_t)first;
  *out = w.release();
  return BH_OK;
}

bh_status bh_witness_sizes(const bh_witness* w, size_t sizes[4]) {
  if (!w || !sizes) return BH_ERR_INVALID_ARGUMENT;
  sizes[0] = w->num_constraints;
  sizes[1] = w->m;
  sizes[2] = w->num_inputs;
  sizes[3] = w->num_aux;
  return BH_OK;
}

bh_status bh_witness_read(const bh_witness* w, uint64_t* a, uint64_t* b, uint64_t* c, uint64_t* inputs,
                          uint64_t* aux, uint64_t* a_aux_density, uint64_t* b_input_density,
                          uint64_t* b_aux_density) {
  if (!w || !w->ctx || w->raw) return BH_ERR_INVALID_ARGUMENT;  // (raw: bh_prove's own, never handed out)
  bh_ctx* ctx = w->ctx;
  std::lock_guard<std::mutex> lk(ctx->mu);
  BH_TRY_HIP(hipSetDevice(ctx->device));
  const size_t m = w->m, ni = w->num_inputs, na = w->num_aux;
  hipStream_t st = ctx->stream;
  // the witness is left as it is: each vector is converted into the context's staging buffer
  BH_TRY_HIP(ctx->staging.alloc(std::max({m, ni, na, (size_t)1}) * 32));
  uint32_t* d_tmp = ctx->staging.as<uint32_t>();
  uint64_t* vecs[3] = {a, b, c};
  for (int v = 0; v < 3; v++) {
    if (!vecs[v]) continue;
    launch_fr_convert(w->abc.as<uint32_t>() + (size_t)v * m * 8, d_tmp, m, from_dev_const(), 1, st);
    BH_TRY_HIP(hipGetLastError());
    BH_TRY_HIP(hipMemcpyAsync(vecs[v], d_tmp, m * 32, hipMemcpyDeviceToHost, st));
    BH_TRY_HIP(hipStreamSynchronize(st));
  }
  // canonical x -> bls12_381 Montgomery x 2^256: launch_fr_convert's x * k * 2^-261 with k = 2^517
  Fr one = Fr::one();
  const FrConst to_mont = dev_limbs(fr_from_canonical(one.v));
  const struct { uint64_t* host; const DevBuf& dev; size_t n; } sc[2] = {{inputs, w->inputs, ni}, {aux, w->aux, na}};
  for (const auto& x : sc) {
    if (!x.host || !x.n) continue;
    launch_fr_convert(x.dev.as<uint32_t>(), d_tmp, x.n, to_mont, 1, st);
    BH_TRY_HIP(hipGetLastError());
    BH_TRY_HIP(hipMemcpyAsync(x.host, d_tmp, x.n * 32, hipMemcpyDeviceToHost, st));
    BH_TRY_HIP(hipStreamSynchronize(st));
  }
  if (a_aux_density) memcpy(a_aux_density, w->a_aux_density.data(), w->a_aux_words * 8);
  if (b_input_density) memcpy(b_input_density, w->b_input_density.data(), w->b_in_words * 8);
  if (b_aux_density) memcpy(b_aux_density, w->b_aux_density.data(), w->b_aux_words * 8);
  return BH_OK;
}

}  // extern "C"
