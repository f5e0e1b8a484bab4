// Device self-tests of field arithmetic whose correctness rests on hand-derived bounds
// (tests/test_gpu_selftest.py; not part of the public ABI, declared in api_internal.h), of the
// field predicates and conversions (bh_selftest_field_misc), and the validated entry to the
// accumulation kernels on an ordered entry list (bh_selftest_accumulate).  The group law's
// self-test has units of its own (selftest_group.cuh).
//
// fe2_mul_sub_kara (field.cuh; Fp2Ops::mul_sub_lazy, the G2 mixed addition's Y3 = R (Q - X3) - Y1
// PPP under one Montgomery reduction per half) keeps signed Karatsuba column sums in a biased
// unsigned 64-bit accumulator: the bias and the +p fix-up of a negative top limb are argued from
// operand values < 2^386 with normalised 29-bit limbs.  This kernel evaluates it, and the same
// a*b - c*d as two full Fp2 products and a subtraction (the path it replaced), on caller-chosen
// operands -- the test drives both at the stated maxima and where the result is negative before
// the fix-up, against host big integers.
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
