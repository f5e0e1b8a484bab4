// Device self-tests of field arithmetic whose correctness rests on hand-derived bounds
// (tests/test_gpu_selftest.py; not part of the public ABI, declared in api_internal.h).
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
}  // namespace

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
