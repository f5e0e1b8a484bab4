// Device self-tests of field arithmetic whose correctness rests on hand-derived bounds
// (tests/test_gpu_selftest.py; not part of the public ABI, declared in api_internal.h), of the
// field predicates and conversions (bh_selftest_field_misc), and the validated entry to the
// accumulation kernels on an ordered entry list (bh_selftest_accumulate), and the validated entries
// to the layer that produces such lists (bh_selftest_digit_sort and the four after it, at the end).
// The group law's self-test has units of its own (selftest_group.cuh).
//
// fe2_mul_sub_kara (field.cuh; Fp2Ops::mul_sub_lazy, the G2 mixed addition's Y3 = R (Q - X3) - Y1
// PPP under one Montgomery reduction per half) keeps signed Karatsuba column sums in a biased
// unsigned 64-bit accumulator: the bias and the +p fix-up of a negative top limb are argued from
// operand values < 2^386 with normalised 29-bit limbs.  This kernel evaluates it, and the same
// a*b - c*d as two full Fp2 products and a subtraction (the path it replaced), on caller-chosen
// operands -- the test drives both at the stated maxima and where the result is negative before
// the fix-up, against host big integers.
#include <algorithm>

#include "api_internal.h"

namespace {
__global__ void __launch_bounds__(64) k_selftest_fp2_mul_sub(const uint32_t* in, uint32_t* out, uint32_t n) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  constexpr int N = FpCfg::N;
  auto ld = [&](int k) {
    DFp x;
#pragma unroll
    for (int l = 0; l < N; l++) x.v[l] = in[((size_t)t * 8 + k) * N + l];
    return x;
  };
  const DFp2 a{ld(0), ld(1)}, b{ld(2), ld(3)}, c{ld(4), ld(5)}, d{ld(6), ld(7)};
  const DFp2 lazy = Fp2Ops::mul_sub_lazy(a, b, c, d);
  const DFp2 two = Fp2Ops::sub<2>(Fp2Ops::mul(a, b), Fp2Ops::mul(c, d));
  const DFp* r[4] = {&lazy.c0, &lazy.c1, &two.c0, &two.c1};
#pragma unroll
  for (int k = 0; k < 4; k++)
#pragma unroll
    for (int l = 0; l < N; l++) out[((size_t)t * 4 + k) * N + l] = r[k]->v[l];
}
// Every product form of field.cuh in both column forms (CH = false: split chains and a merge per
// column; CH = true: one carry-seeded chain per column), on the same operands.
template <bool CH>
__device__ void selftest_products(const DFp& a, const DFp& b, const DFp& c, const DFp& d, const DFp& e, const DFp& f,
                                  const DFp& g, const DFp& h, const DFr& x, const DFr& y, uint32_t* out) {
  constexpr int N = FpCfg::N;
  DFp r[8];
  r[0] = fe_mul<FpCfg, CH>(a, b);
  r[1] = fe_sqr<FpCfg, CH>(a);
  r[2] = fe_mul2<FpCfg, CH>(a, b, c, d);
  r[3] = fe_from_mont<FpCfg, CH>(a);
  fe2_mul_kara<FpCfg, CH>(a, b, c, d, r[4], r[5]);
  fe2_mul_sub_kara<FpCfg, CH>(e, f, g, h, h, e, f, g, r[6], r[7]);
  const DFr s = fe_mul<FrCfg, CH>(x, y);
#pragma unroll
  for (int k = 0; k < 8; k++)
#pragma unroll
    for (int l = 0; l < N; l++) out[k * N + l] = r[k].v[l];
#pragma unroll
  for (int l = 0; l < FrCfg::N; l++) out[8 * N + l] = s.v[l];
}

constexpr int SELFTEST_PRODUCTS_IN = 8 * FpCfg::N + 2 * FrCfg::N;   // a .. h (Fp); x, y (Fr)
constexpr int SELFTEST_PRODUCTS_OUT = 8 * FpCfg::N + FrCfg::N;      // per column form

__global__ void __launch_bounds__(64) k_selftest_field_products(const uint32_t* in, uint32_t* out, uint32_t n) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  const uint32_t* src = in + (size_t)t * SELFTEST_PRODUCTS_IN;
  DFp f[8];
  DFr g[2];
#pragma unroll
  for (int k = 0; k < 8; k++)
#pragma unroll
    for (int l = 0; l < FpCfg::N; l++) f[k].v[l] = src[k * FpCfg::N + l];
#pragma unroll
  for (int k = 0; k < 2; k++)
#pragma unroll
    for (int l = 0; l < FrCfg::N; l++) g[k].v[l] = src[8 * FpCfg::N + k * FrCfg::N + l];
  uint32_t* dst = out + (size_t)t * 2 * SELFTEST_PRODUCTS_OUT;
  selftest_products<false>(f[0], f[1], f[2], f[3], f[4], f[5], f[6], f[7], g[0], g[1], dst);
  selftest_products<true>(f[0], f[1], f[2], f[3], f[4], f[5], f[6], f[7], g[0], g[1], dst + SELFTEST_PRODUCTS_OUT);
}

// The predicates, subtractions and conversions of field.cuh that the group law and the transforms
// rest on.  Per case a, b (Fp) and x, y (Fr), raw limbs -> (Fp) is_zero(a), reduce_full(a),
// csub<1>(a), neg_canonical(a), sub<K>(a, b) for the K of curve.cuh (1, 2, 4, 8, 16, 128), a + b,
// pack(a) and unpack(pack(a)); (Fr, the forms the library instantiates) is_zero(x), csub<1>(x),
// csub<2>(x), sub<2>(x, y), x + y, pack(x), unpack(pack(x)).  Every form is evaluated on every
// case; the test reads the ones whose preconditions the case meets.
constexpr int FIELD_MISC_IN = 2 * FpCfg::N + 2 * FrCfg::N;
constexpr int FIELD_MISC_FP = 1 + 10 * FpCfg::N + Packed<FpCfg>::W + FpCfg::N;
constexpr int FIELD_MISC_FR = 1 + 4 * FrCfg::N + Packed<FrCfg>::W + FrCfg::N;
constexpr int FIELD_MISC_OUT = FIELD_MISC_FP + FIELD_MISC_FR;

template <class C>
__device__ uint32_t* put_limbs(uint32_t* dst, const Fe<C>& x) {
#pragma unroll
  for (int l = 0; l < C::N; l++) dst[l] = x.v[l];
  return dst + C::N;
}

__global__ void __launch_bounds__(64) k_selftest_field_misc(const uint32_t* in, uint32_t* out, uint32_t n) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  const uint32_t* src = in + (size_t)t * FIELD_MISC_IN;
  DFp a, b;
  DFr x, y;
#pragma unroll
  for (int l = 0; l < FpCfg::N; l++) {
    a.v[l] = src[l];
    b.v[l] = src[FpCfg::N + l];
  }
#pragma unroll
  for (int l = 0; l < FrCfg::N; l++) {
    x.v[l] = src[2 * FpCfg::N + l];
    y.v[l] = src[2 * FpCfg::N + FrCfg::N + l];
  }
  uint32_t* d = out + (size_t)t * FIELD_MISC_OUT;
  *d++ = fe_is_zero<FpCfg>(a) ? 1u : 0u;
  d = put_limbs(d, fe_reduce_full<FpCfg>(a));
  d = put_limbs(d, fe_csub<FpCfg, 1>(a));
  d = put_limbs(d, FpOps::neg_canonical(a));
  d = put_limbs(d, fe_sub<FpCfg, 1>(a, b));
  d = put_limbs(d, fe_sub<FpCfg, 2>(a, b));
  d = put_limbs(d, fe_sub<FpCfg, 4>(a, b));
  d = put_limbs(d, fe_sub<FpCfg, 8>(a, b));
  d = put_limbs(d, fe_sub<FpCfg, 16>(a, b));
  d = put_limbs(d, fe_sub<FpCfg, 128>(a, b));
  d = put_limbs(d, fe_add<FpCfg>(a, b));
  uint32_t wp[Packed<FpCfg>::W];
  fe_pack<FpCfg>(a, wp);
#pragma unroll
  for (int l = 0; l < Packed<FpCfg>::W; l++) *d++ = wp[l];
  d = put_limbs(d, fe_unpack<FpCfg>(wp));
  *d++ = fe_is_zero<FrCfg>(x) ? 1u : 0u;
  d = put_limbs(d, fe_csub<FrCfg, 1>(x));
  d = put_limbs(d, fe_csub<FrCfg, 2>(x));
  d = put_limbs(d, fe_sub<FrCfg, 2>(x, y));
  d = put_limbs(d, fe_add<FrCfg>(x, y));
  uint32_t wr[Packed<FrCfg>::W];
  fe_pack<FrCfg>(x, wr);
#pragma unroll
  for (int l = 0; l < Packed<FrCfg>::W; l++) *d++ = wr[l];
  d = put_limbs(d, fe_unpack<FrCfg>(wr));
}
}  // namespace

// n cases of a, b (Fp, 14 raw limbs each) and x, y (Fr, 9 raw limbs each) -> FIELD_MISC_OUT words
// per case in the order listed at k_selftest_field_misc
extern "C" bh_status bh_selftest_field_misc(int device, const uint32_t* in, size_t n, uint32_t* out) {
  if ((n && (!in || !out)) || n > (1u << 20)) return BH_ERR_INVALID_ARGUMENT;
  if (!n) return BH_OK;
  BH_TRY_HIP(hipSetDevice(device));
  const size_t in_b = n * FIELD_MISC_IN * 4, out_b = n * FIELD_MISC_OUT * 4;
  bh::DevBuf din, dout;
  BH_TRY_HIP(din.alloc(in_b));
  BH_TRY_HIP(dout.alloc(out_b));
  BH_TRY_HIP(hipMemcpy(din.p, in, in_b, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(k_selftest_field_misc, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, nullptr, din.as<uint32_t>(),
                     dout.as<uint32_t>(), (uint32_t)n);
  BH_TRY_HIP(hipGetLastError());
  BH_TRY_HIP(hipMemcpy(out, dout.p, out_b, hipMemcpyDeviceToHost));
  return BH_OK;
}

// The accumulation kernels (msm_impl.cuh) on an entry list in the caller's order.  The kernels
// index memory from these arrays, so everything is checked here and nothing is launched on a
// violation: sizes capped at 2^16, rec one of the two record forms of the group, offsets
// non-decreasing from 0 to the entry count, every base index (bit 31: negate) below nbases,
// 1 <= S, b_lo < b_hi <= nbt, and at least one entry in [offsets[b_lo], offsets[b_hi]).
// Returns bucket_sums[nbt] and conts[segs] as raw XYZZ limbs and cont_bucket[segs],
// segs = ceil(n_entries / S); slots the kernel did not write hold 0xFF bytes.
extern "C" bh_status bh_selftest_accumulate(int device, int group, int kernel, const uint32_t* bases, size_t nbases,
                                            uint32_t rec, const uint32_t* entries, size_t n_entries,
                                            const uint32_t* offsets, size_t nbt, uint32_t S, uint32_t b_lo,
                                            uint32_t b_hi, uint32_t* bucket_sums, uint32_t* conts,
                                            uint32_t* cont_bucket) {
  constexpr size_t CAP = (size_t)1 << 16;
  if (!bases || !entries || !offsets || !bucket_sums || !conts || !cont_bucket) return BH_ERR_INVALID_ARGUMENT;
  if (group != 0 && group != 1) return BH_ERR_INVALID_ARGUMENT;
  if (kernel != 0 && !(kernel == 1 && group == 1)) return BH_ERR_INVALID_ARGUMENT;
  const uint32_t packed = group ? 2u * Fp2Ops::PACKED_WORDS : 2u * G1F::PACKED_WORDS;
  const uint32_t table = group ? bh::G2_TABLE_REC : bh::G1_TABLE_REC;
  if (rec != packed && rec != table) return BH_ERR_INVALID_ARGUMENT;
  if (!nbases || nbases > CAP || !n_entries || n_entries > CAP || !nbt || nbt > CAP) return BH_ERR_INVALID_ARGUMENT;
  if (S < 1 || S > CAP || !(b_lo < b_hi && b_hi <= nbt)) return BH_ERR_INVALID_ARGUMENT;
  if (offsets[0] != 0 || offsets[nbt] != n_entries) return BH_ERR_INVALID_ARGUMENT;
  for (size_t b = 0; b < nbt; b++)
    if (offsets[b] > offsets[b + 1]) return BH_ERR_INVALID_ARGUMENT;
  if (offsets[b_lo] == offsets[b_hi]) return BH_ERR_INVALID_ARGUMENT;
  for (size_t j = 0; j < n_entries; j++)
    if ((entries[j] & 0x7fffffffu) >= nbases) return BH_ERR_INVALID_ARGUMENT;
  BH_TRY_HIP(hipSetDevice(device));
  if (group)
    BH_TRY_HIP(bh::msm_selftest_accumulate<G2Ops>(kernel, bases, nbases, rec, entries, n_entries, offsets, nbt, S, b_lo,
                                                  b_hi, bucket_sums, conts, cont_bucket));
  else
    BH_TRY_HIP(bh::msm_selftest_accumulate<G1Ops>(kernel, bases, nbases, rec, entries, n_entries, offsets, nbt, S, b_lo,
                                                  b_hi, bucket_sums, conts, cont_bucket));
  return BH_OK;
}

// The back half of a multiexp (msm_impl.cuh: msm_accumulate, max_span, msm_back -> reduce_range)
// on an entry list in the caller's order: Wb windows of NB buckets (nbt = Wb * NB), reduced over
// [b0, b0 + nbr) of one shared window (Wb == 1) or over every window (b0 = 0, nbr = NB).  mode 0:
// max_span's words over the reduced range are handed to the kernels, as the prover and the job
// queue run a tail; mode 1: no span words, every level of the continuation tree, as
// msm_window_sums runs it.  Checked here, nothing launched on a violation: the rules of
// bh_selftest_accumulate for sizes, rec, offsets, base indices and S; Wb <= 128, Wb * NB == nbt;
// nbr a power of two, or with Wb == 1 a multiple of 1024; b0 + nbr <= NB, and for Wb > 1 the
// whole windows; at least one entry in the range.
// Returns bucket_sums[nbt] as k_cont_fold left them (raw XYZZ limbs; buckets outside the range or
// without entries: 0xFF bytes), k_rowcol_final's points in out -- Wb totals for Wb > 1, out[0..1]
// for the whole of one shared window, out[0..2] for a proper range of it (the bucket-shard path) --
// and the geometry's lc: a shared window's total is out[0] + 2^lc * out[1].
extern "C" bh_status bh_selftest_reduce(int device, int group, int mode, const uint32_t* bases, size_t nbases,
                                        uint32_t rec, const uint32_t* entries, size_t n_entries,
                                        const uint32_t* offsets, size_t nbt, uint32_t S, uint32_t Wb, uint32_t NB,
                                        uint32_t b0, uint32_t nbr, uint32_t* bucket_sums, uint32_t* out, int* lc) {
  constexpr size_t CAP = (size_t)1 << 16;
  if (!bases || !entries || !offsets || !bucket_sums || !out || !lc) return BH_ERR_INVALID_ARGUMENT;
  if ((group != 0 && group != 1) || (mode != 0 && mode != 1)) return BH_ERR_INVALID_ARGUMENT;
  const uint32_t packed = group ? 2u * Fp2Ops::PACKED_WORDS : 2u * G1F::PACKED_WORDS;
  const uint32_t table = group ? bh::G2_TABLE_REC : bh::G1_TABLE_REC;
  if (rec != packed && rec != table) return BH_ERR_INVALID_ARGUMENT;
  if (!nbases || nbases > CAP || !n_entries || n_entries > CAP || !nbt || nbt > CAP) return BH_ERR_INVALID_ARGUMENT;
  if (S < 1 || S > CAP) return BH_ERR_INVALID_ARGUMENT;
  if (Wb < 1 || Wb > 128 || NB < 1 || NB > CAP || (size_t)Wb * NB != nbt) return BH_ERR_INVALID_ARGUMENT;
  if (nbr < 1 || nbr > NB || b0 > NB - nbr) return BH_ERR_INVALID_ARGUMENT;
  const bool pow2 = (nbr & (nbr - 1)) == 0;
  if (Wb > 1 ? !(pow2 && b0 == 0 && nbr == NB) : !(pow2 || nbr % bh::BUCKET_SHARD_GRANULE == 0))
    return BH_ERR_INVALID_ARGUMENT;
  if (offsets[0] != 0 || offsets[nbt] != n_entries) return BH_ERR_INVALID_ARGUMENT;
  for (size_t b = 0; b < nbt; b++)
    if (offsets[b] > offsets[b + 1]) return BH_ERR_INVALID_ARGUMENT;
  if (offsets[b0] == offsets[b0 + (size_t)Wb * nbr]) return BH_ERR_INVALID_ARGUMENT;
  for (size_t j = 0; j < n_entries; j++)
    if ((entries[j] & 0x7fffffffu) >= nbases) return BH_ERR_INVALID_ARGUMENT;
  BH_TRY_HIP(hipSetDevice(device));
  if (group)
    BH_TRY_HIP(bh::msm_selftest_reduce<G2Ops>(mode, bases, nbases, rec, entries, n_entries, offsets, S, Wb, NB, b0, nbr,
                                              bucket_sums, out));
  else
    BH_TRY_HIP(bh::msm_selftest_reduce<G1Ops>(mode, bases, nbases, rec, entries, n_entries, offsets, S, Wb, NB, b0, nbr,
                                              bucket_sums, out));
  *lc = bh::rowcol_geom(nbr, bh::ROWCOL_QLG, group != 0).lc;
  return BH_OK;
}

// n cases of 8 Fp operands a .. h (14 raw limbs each; e .. h < 2^386, fe2_mul_sub_kara's bound) and
// 2 Fr operands x, y (9 raw limbs each) -> per case, once per column form (split, then
// carry-seeded): a*b, a^2, a*b + c*d, a/R (Fp); (a + b u)(c + d u) by fe2_mul_kara (c0, c1);
// (e + f u)(g + h u) - (h + e u)(f + g u) by fe2_mul_sub_kara (c0, c1); x*y (Fr): 8 x 14 + 9 raw limbs
extern "C" bh_status bh_selftest_field_products(int device, const uint32_t* in, size_t n, uint32_t* out) {
  if ((n && (!in || !out)) || n > (1u << 20)) return BH_ERR_INVALID_ARGUMENT;
  if (!n) return BH_OK;
  BH_TRY_HIP(hipSetDevice(device));
  const size_t in_b = n * SELFTEST_PRODUCTS_IN * 4, out_b = n * 2 * SELFTEST_PRODUCTS_OUT * 4;
  bh::DevBuf din, dout;
  BH_TRY_HIP(din.alloc(in_b));
  BH_TRY_HIP(dout.alloc(out_b));
  BH_TRY_HIP(hipMemcpy(din.p, in, in_b, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(k_selftest_field_products, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, nullptr,
                     din.as<uint32_t>(), dout.as<uint32_t>(), (uint32_t)n);
  BH_TRY_HIP(hipGetLastError());
  BH_TRY_HIP(hipMemcpy(out, dout.p, out_b, hipMemcpyDeviceToHost));
  return BH_OK;
}

// n cases of 8 Fp operands (a0, a1, b0, b1, c0, c1, d0, d1; 14 raw 29-bit limbs each) ->
// 4 Fp results per case (lazy c0, c1; two-product c0, c1), raw limbs
extern "C" bh_status bh_selftest_fp2_mul_sub(int device, const uint32_t* in, size_t n, uint32_t* out) {
  if ((n && (!in || !out)) || n > (1u << 20)) return BH_ERR_INVALID_ARGUMENT;
  if (!n) return BH_OK;
  BH_TRY_HIP(hipSetDevice(device));
  const size_t in_b = n * 8 * FpCfg::N * 4, out_b = n * 4 * FpCfg::N * 4;
  bh::DevBuf din, dout;
  BH_TRY_HIP(din.alloc(in_b));
  BH_TRY_HIP(dout.alloc(out_b));
  BH_TRY_HIP(hipMemcpy(din.p, in, in_b, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(k_selftest_fp2_mul_sub, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, nullptr,
                     din.as<uint32_t>(), dout.as<uint32_t>(), (uint32_t)n);
  BH_TRY_HIP(hipGetLastError());
  BH_TRY_HIP(hipMemcpy(out, dout.p, out_b, hipMemcpyDeviceToHost));
  return BH_OK;
}

// ------------------------------------------------------------------ scalars -> sorted entries
// The layer between a caller's scalars and the accumulation kernels (msm_common.hip), driven
// through the host functions of msm.h unchanged on host arrays (tests/test_gpu_digit_sort.py
// against tests/digit_sort_model.py).  The kernels index memory from these arrays, so each entry
// validates them and launches nothing on a violation; device buffers are sized by the library's
// own functions and every output starts as 0xFF bytes.
namespace {
constexpr size_t SORT_CAP_N = (size_t)1 << 16;   // scalars / index-map words
constexpr size_t SORT_CAP_E = (size_t)1 << 23;   // entries (2^16 scalars x 128 windows at c = 2)
constexpr size_t SCAN_CAP_N = (size_t)1 << 21;

hipError_t alloc_ff(bh::DevBuf& b, size_t words) {
  hipError_t e = b.alloc(words * 4);
  if (e == hipSuccess && words) e = hipMemset(b.p, 0xFF, words * 4);
  return e;
}
hipError_t alloc_copy(bh::DevBuf& b, const void* src, size_t bytes) {
  hipError_t e = b.alloc(bytes);
  if (e == hipSuccess && bytes) e = hipMemcpy(b.p, src, bytes, hipMemcpyHostToDevice);
  return e;
}
// a base index b is usable when b * W + w < 2^31 (bit 31 of an entry is the sign)
bool idx_in_range(const int32_t* idx, size_t n, uint32_t W) {
  const int64_t lim = ((int64_t)1 << 31) / (int64_t)W;
  for (size_t i = 0; i < n; i++)
    if (idx[i] < -1 || (int64_t)idx[i] >= lim) return false;
  return true;
}
}  // namespace

// sort_entries, then max_span over [red_lo, red_lo + Wb * red_nb) as the prover's sort_job calls
// them, for the shape msm_shape(n, c) (pre = 0) or msm_shape_table(n, c) (pre = 1) with segment
// length S and, when bk_lo | bk_hi, the bucket shard [bk_lo, bk_hi).  scalars: n x 8 LE words;
// idx: n base indices (-1 = absent) or null for base_offset + i.  Returns entries[n * W],
// counts[nbt], offsets[nbt + 1] (nbt = Wb * NB), the span words and their number.
extern "C" bh_status bh_selftest_digit_sort(int device, const uint32_t* scalars, size_t n, const int32_t* idx,
                                            uint32_t base_offset, int c, int pre, uint32_t bk_lo, uint32_t bk_hi,
                                            uint32_t S, uint32_t* entries, uint32_t* counts, uint32_t* offsets,
                                            uint32_t* span_words, uint32_t* n_span_words) {
  if (c < 2 || c > 24 || (pre != 0 && pre != 1)) return BH_ERR_INVALID_ARGUMENT;
  if (n > SORT_CAP_N || (n && (!scalars || !entries))) return BH_ERR_INVALID_ARGUMENT;
  if (!counts || !offsets || !span_words || !n_span_words) return BH_ERR_INVALID_ARGUMENT;
  if (S < 1 || S > (1u << 16)) return BH_ERR_INVALID_ARGUMENT;
  bh::MsmShape sh = pre ? bh::msm_shape_table(n, c) : bh::msm_shape(n, c);
  sh.S = (int)S;
  const size_t E = n * (size_t)sh.W, nbt = (size_t)sh.Wb * sh.NB;
  if (E >= ((size_t)1 << 31)) return BH_ERR_INVALID_ARGUMENT;
  if (idx ? !idx_in_range(idx, n, (uint32_t)sh.W)
          : (uint64_t)base_offset + n > (((uint64_t)1 << 31) / (uint64_t)sh.W))
    return BH_ERR_INVALID_ARGUMENT;
  if (bk_lo || bk_hi) {
    const uint32_t G = std::max<uint32_t>(bh::BUCKET_SHARD_GRANULE, (uint32_t)sh.NB >> 12);
    if (!pre || bk_lo >= bk_hi || bk_hi > (uint32_t)sh.NB || bk_lo % G || bk_hi % G) return BH_ERR_INVALID_ARGUMENT;
    sh.bk_lo = bk_lo;
    sh.bk_hi = bk_hi;
  }
  BH_TRY_HIP(hipSetDevice(device));
  const size_t tc = bh::sort_tilecount_words(sh, n);
  const size_t span_nbt = (size_t)sh.Wb * sh.red_nb();
  const uint32_t g = bh::max_span_blocks(span_nbt);
  bh::DevBuf dsc, didx, dtc, dts, drecs, dent, dcnt, doff, dspan;
  BH_TRY_HIP(alloc_copy(dsc, scalars, n * 32));
  if (idx) BH_TRY_HIP(alloc_copy(didx, idx, n * 4));
  BH_TRY_HIP(alloc_ff(dtc, tc));
  BH_TRY_HIP(alloc_ff(dts, bh::scan_scratch_words(tc) + 16));
  BH_TRY_HIP(alloc_ff(drecs, 2 * E));
  BH_TRY_HIP(alloc_ff(dent, E));
  BH_TRY_HIP(alloc_ff(dcnt, nbt + 1));
  BH_TRY_HIP(alloc_ff(doff, nbt + 1));
  BH_TRY_HIP(alloc_ff(dspan, bh::MAX_SPAN_BLOCKS));
  BH_TRY_HIP(bh::sort_entries(dsc.as<uint32_t>(), n, idx ? didx.as<int32_t>() : nullptr, base_offset, sh,
                              dtc.as<uint32_t>(), dts.as<uint32_t>(), drecs.as<uint2>(), dent.as<uint32_t>(),
                              dcnt.as<uint32_t>(), doff.as<uint32_t>(), nullptr));
  BH_TRY_HIP(bh::max_span(dcnt.as<uint32_t>() + sh.red_lo(), doff.as<uint32_t>() + sh.red_lo(), span_nbt, S,
                          dspan.as<uint32_t>(), nullptr, nullptr));
  BH_TRY_HIP(hipDeviceSynchronize());
  if (E) BH_TRY_HIP(hipMemcpy(entries, dent.p, E * 4, hipMemcpyDeviceToHost));
  BH_TRY_HIP(hipMemcpy(counts, dcnt.p, nbt * 4, hipMemcpyDeviceToHost));
  BH_TRY_HIP(hipMemcpy(offsets, doff.p, (nbt + 1) * 4, hipMemcpyDeviceToHost));
  BH_TRY_HIP(hipMemcpy(span_words, dspan.p, (size_t)g * 4, hipMemcpyDeviceToHost));
  *n_span_words = g;
  return BH_OK;
}

// derive_sorted on a source layout given as host arrays: src_entries[Emax], src_offsets[nbt + 1]
// (read at [b0, b1] and at nbt, the source's entry count: non-decreasing there and <= Emax),
// every source entry's base inside [src_off, src_off + n_idx), the target map idx[n_idx] (-1 =
// absent).  b1 = 0 stands for nbt, as in derive_sorted.  Returns dst_entries[Emax],
// dst_counts[nbt], dst_offsets[nbt + 1].
extern "C" bh_status bh_selftest_derive_sorted(int device, const uint32_t* src_entries, size_t Emax,
                                               const uint32_t* src_offsets, size_t nbt, int pre, uint32_t W,
                                               uint32_t src_off, const int32_t* idx, size_t n_idx, size_t b0,
                                               size_t b1, uint32_t* dst_entries, uint32_t* dst_counts,
                                               uint32_t* dst_offsets) {
  if (!src_entries || !src_offsets || !idx || !dst_entries || !dst_counts || !dst_offsets)
    return BH_ERR_INVALID_ARGUMENT;
  if (!Emax || Emax > SORT_CAP_E || !nbt || nbt > SORT_CAP_E || !n_idx || n_idx > SORT_CAP_N)
    return BH_ERR_INVALID_ARGUMENT;
  if ((pre != 0 && pre != 1) || W < 1 || W > 128) return BH_ERR_INVALID_ARGUMENT;
  if (b1 == 0) b1 = nbt;
  if (b0 > b1 || b1 > nbt) return BH_ERR_INVALID_ARGUMENT;
  const size_t E = src_offsets[nbt];
  if (E > Emax || src_offsets[b1] > E) return BH_ERR_INVALID_ARGUMENT;
  for (size_t b = b0; b < b1; b++)
    if (src_offsets[b] > src_offsets[b + 1]) return BH_ERR_INVALID_ARGUMENT;
  if (!idx_in_range(idx, n_idx, W)) return BH_ERR_INVALID_ARGUMENT;
  for (size_t j = 0; j < E; j++) {
    const uint32_t v = src_entries[j] & 0x7fffffffu;
    const uint32_t base = pre ? v / W : v;
    if (base < src_off || (size_t)(base - src_off) >= n_idx) return BH_ERR_INVALID_ARGUMENT;
  }
  BH_TRY_HIP(hipSetDevice(device));
  bh::DevBuf dse, dso, didx, dpos, dscr, dent, dcnt, doff;
  BH_TRY_HIP(alloc_copy(dse, src_entries, Emax * 4));
  BH_TRY_HIP(alloc_copy(dso, src_offsets, (nbt + 1) * 4));
  BH_TRY_HIP(alloc_copy(didx, idx, n_idx * 4));
  BH_TRY_HIP(alloc_ff(dpos, Emax + 1));
  BH_TRY_HIP(alloc_ff(dscr, bh::derive_scratch_words(Emax)));
  BH_TRY_HIP(alloc_ff(dent, Emax));
  BH_TRY_HIP(alloc_ff(dcnt, nbt + 1));
  BH_TRY_HIP(alloc_ff(doff, nbt + 1));
  BH_TRY_HIP(bh::derive_sorted(dse.as<uint32_t>(), dso.as<uint32_t>(), nbt, Emax, pre, W, src_off, didx.as<int32_t>(),
                               dpos.as<uint32_t>(), dscr.as<uint32_t>(), dent.as<uint32_t>(), dcnt.as<uint32_t>(),
                               doff.as<uint32_t>(), nullptr, b0, b1));
  BH_TRY_HIP(hipDeviceSynchronize());
  BH_TRY_HIP(hipMemcpy(dst_entries, dent.p, Emax * 4, hipMemcpyDeviceToHost));
  BH_TRY_HIP(hipMemcpy(dst_counts, dcnt.p, nbt * 4, hipMemcpyDeviceToHost));
  BH_TRY_HIP(hipMemcpy(dst_offsets, doff.p, (nbt + 1) * 4, hipMemcpyDeviceToHost));
  return BH_OK;
}

// exclusive_scan of in[n] in place (dn < 0), or the scan bounded by a device word holding dn
// (elements 0 .. dn), in place as derive_sorted runs it; out[n] is the buffer afterwards
extern "C" bh_status bh_selftest_scan(int device, const uint32_t* in, size_t n, int64_t dn, uint32_t* out) {
  if ((n && (!in || !out)) || n > SCAN_CAP_N || dn < -1 || dn > (int64_t)0xffffffff) return BH_ERR_INVALID_ARGUMENT;
  if (!n) return BH_OK;
  BH_TRY_HIP(hipSetDevice(device));
  bh::DevBuf dbuf, dscr, ddn;
  const uint32_t dn_word = (uint32_t)dn;
  BH_TRY_HIP(alloc_copy(dbuf, in, n * 4));
  BH_TRY_HIP(alloc_ff(dscr, bh::scan_scratch_words(n) + 16));
  BH_TRY_HIP(alloc_copy(ddn, &dn_word, 4));
  if (dn < 0)
    bh::exclusive_scan(dbuf.as<uint32_t>(), dbuf.as<uint32_t>(), n, dscr.as<uint32_t>(), nullptr);
  else
    bh::exclusive_scan_bounded(dbuf.as<uint32_t>(), dbuf.as<uint32_t>(), n, dscr.as<uint32_t>(), nullptr,
                               ddn.as<uint32_t>());
  BH_TRY_HIP(hipGetLastError());
  BH_TRY_HIP(hipDeviceSynchronize());
  BH_TRY_HIP(hipMemcpy(out, dbuf.p, n * 4, hipMemcpyDeviceToHost));
  return BH_OK;
}

// scalars_prepare: in (8 LE words per scalar; 2^log_perm of them when log_perm > 0, then
// n = 2^log_perm) -> out[n x 8]; mode 0 canonical words, 1 bls12_381 Montgomery, 2 device Montgomery
extern "C" bh_status bh_selftest_scalars_prepare(int device, const uint32_t* in, size_t n, int mode, int log_perm,
                                                 uint32_t* out) {
  if ((n && (!in || !out)) || n > SORT_CAP_N || mode < 0 || mode > 2 || log_perm < 0 || log_perm > 16)
    return BH_ERR_INVALID_ARGUMENT;
  if (log_perm > 0 && n != ((size_t)1 << log_perm)) return BH_ERR_INVALID_ARGUMENT;
  if (!n) return BH_OK;
  BH_TRY_HIP(hipSetDevice(device));
  bh::DevBuf din, dout;
  BH_TRY_HIP(alloc_copy(din, in, n * 32));
  BH_TRY_HIP(alloc_ff(dout, n * 8));
  BH_TRY_HIP(bh::scalars_prepare(din.as<uint32_t>(), dout.as<uint32_t>(), n, mode, log_perm, nullptr));
  BH_TRY_HIP(hipDeviceSynchronize());
  BH_TRY_HIP(hipMemcpy(out, dout.p, n * 32, hipMemcpyDeviceToHost));
  return BH_OK;
}

// density_index: words[ceil(n / 64)] -> idx[n]
extern "C" bh_status bh_selftest_density_index(int device, const uint64_t* words, size_t n, uint32_t base_offset,
                                               int32_t* idx) {
  if ((n && (!words || !idx)) || n > 2 * SORT_CAP_N || (uint64_t)base_offset + n >= ((uint64_t)1 << 31))
    return BH_ERR_INVALID_ARGUMENT;
  if (!n) return BH_OK;
  BH_TRY_HIP(hipSetDevice(device));
  const size_t nwords = (n + 63) / 64;
  bh::DevBuf dw, didx, dtmp, dscr;
  BH_TRY_HIP(alloc_copy(dw, words, nwords * 8));
  BH_TRY_HIP(alloc_ff(didx, n));
  BH_TRY_HIP(alloc_ff(dtmp, nwords));
  BH_TRY_HIP(alloc_ff(dscr, bh::scan_scratch_words(nwords) + 16));
  BH_TRY_HIP(bh::density_index(dw.as<uint64_t>(), n, base_offset, didx.as<int32_t>(), dtmp.as<uint32_t>(),
                               dscr.as<uint32_t>(), nullptr));
  BH_TRY_HIP(hipDeviceSynchronize());
  BH_TRY_HIP(hipMemcpy(idx, didx.p, n * 4, hipMemcpyDeviceToHost));
  return BH_OK;
}
