// Device self-test of the group law (curve.cuh) on caller-chosen raw limbs
// (bh_selftest_group_law, tests/test_gpu_group_law.py; not part of the public ABI).
//
// The formulas of CurveOps hold under operand bounds (X < 10p, Y < 4p, ZZ, ZZZ < 2p) that a
// multiexp only ever meets at typical representatives; here the test chooses the representative
// of every coordinate and reads the unreduced result.  Included by one translation unit per field
// form (selftest_group.hip: G1, and G2 as the reduction units compile it; selftest_group_kara.hip:
// G2 as msm_g2_acc.hip compiles it).  Everything is in an anonymous namespace: two units
// instantiating a kernel template under one external name would link to a single copy, and both
// forms would run the same code.  One kernel per operation keeps compile time and scratch bounded.
#pragma once
#include "api_internal.h"

namespace {
enum : int { GL_MADD = 0, GL_MADD_NEG = 1, GL_ADD = 2, GL_DBL = 3, GL_DBL_AFFINE = 4, GL_REDUCE = 5, GL_OPS = 6 };

// field elements per case: a point is X, Y, ZZ, ZZZ; an affine base x, y
constexpr int gl_inputs(int op) {
  return op == GL_ADD ? 8 : (op == GL_MADD || op == GL_MADD_NEG) ? 6 : op == GL_DBL_AFFINE ? 2 : 4;
}

#ifdef BH_FP2_KARATSUBA
constexpr uint32_t GL_KARATSUBA = 1;
#else
constexpr uint32_t GL_KARATSUBA = 0;
#endif

template <class C, int OP>
__global__ void __launch_bounds__(64) k_selftest_group_law(const uint32_t* in, uint32_t* out, uint32_t n,
                                                           uint32_t* info) {
  using T = typename C::T;
  constexpr int FW = sizeof(T) / 4, NIN = gl_inputs(OP);
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t == 0) {  // the macros this unit was compiled with
    info[0] = (uint32_t)BH_COLUMN_CHAIN;
    info[1] = GL_KARATSUBA;
  }
  if (t >= n) return;
  T f[NIN];
#pragma unroll
  for (int k = 0; k < NIN; k++)
#pragma unroll
    for (int l = 0; l < FW; l++) reinterpret_cast<uint32_t*>(&f[k])[l] = in[((size_t)t * NIN + k) * FW + l];
  typename C::P r;
  if constexpr (OP == GL_MADD || OP == GL_MADD_NEG) {
    const typename C::P p{f[0], f[1], f[2], f[3]};
    typename C::A a{f[4], f[5]};
    if constexpr (OP == GL_MADD_NEG) a = C::neg_affine(a);
    r = C::madd(p, a);
  } else if constexpr (OP == GL_ADD) {
    r = C::add(typename C::P{f[0], f[1], f[2], f[3]}, typename C::P{f[4], f[5], f[6], f[7]});
  } else if constexpr (OP == GL_DBL) {
    r = C::dbl(typename C::P{f[0], f[1], f[2], f[3]});
  } else if constexpr (OP == GL_DBL_AFFINE) {
    r = C::dbl_affine(typename C::A{f[0], f[1]});
  } else {
    r = C::reduce(typename C::P{f[0], f[1], f[2], f[3]});
  }
  const T* res[4] = {&r.X, &r.Y, &r.ZZ, &r.ZZZ};
#pragma unroll
  for (int k = 0; k < 4; k++)
#pragma unroll
    for (int l = 0; l < FW; l++) out[((size_t)t * 4 + k) * FW + l] = reinterpret_cast<const uint32_t*>(res[k])[l];
}

template <class C, int OP>
bh_status selftest_group_law_op(const uint32_t* in, size_t n, uint32_t* out, uint32_t* unit_info) {
  constexpr size_t FW = sizeof(typename C::T) / 4;
  const size_t in_b = n * gl_inputs(OP) * FW * 4, out_b = n * 4 * FW * 4;
  bh::DevBuf din, dout, dinfo;
  BH_TRY_HIP(din.alloc(in_b));
  BH_TRY_HIP(dout.alloc(out_b));
  BH_TRY_HIP(dinfo.alloc(8));
  BH_TRY_HIP(hipMemcpy(din.p, in, in_b, hipMemcpyHostToDevice));
  BH_TRY_HIP(hipMemset(dinfo.p, 0xff, 8));
  hipLaunchKernelGGL((k_selftest_group_law<C, OP>), dim3((unsigned)((n + 63) / 64)), dim3(64), 0, nullptr,
                     din.as<uint32_t>(), dout.as<uint32_t>(), (uint32_t)n, dinfo.as<uint32_t>());
  BH_TRY_HIP(hipGetLastError());
  BH_TRY_HIP(hipMemcpy(out, dout.p, out_b, hipMemcpyDeviceToHost));
  BH_TRY_HIP(hipMemcpy(unit_info, dinfo.p, 8, hipMemcpyDeviceToHost));
  return BH_OK;
}

// n cases of gl_inputs(op) field elements (raw 29-bit limbs: 14 per Fp, 2 x 14 per Fp2) -> the
// unreduced X, Y, ZZ, ZZZ of the result; unit_info[0] = BH_COLUMN_CHAIN, [1] = BH_FP2_KARATSUBA defined
template <class C>
bh_status selftest_group_law_unit(int device, int op, const uint32_t* in, size_t n, uint32_t* out,
                                  uint32_t* unit_info) {
  if (op < 0 || op >= GL_OPS || !in || !out || !unit_info || !n || n > (1u << 20)) return BH_ERR_INVALID_ARGUMENT;
  BH_TRY_HIP(hipSetDevice(device));
  switch (op) {
    case GL_MADD: return selftest_group_law_op<C, GL_MADD>(in, n, out, unit_info);
    case GL_MADD_NEG: return selftest_group_law_op<C, GL_MADD_NEG>(in, n, out, unit_info);
    case GL_ADD: return selftest_group_law_op<C, GL_ADD>(in, n, out, unit_info);
    case GL_DBL: return selftest_group_law_op<C, GL_DBL>(in, n, out, unit_info);
    case GL_DBL_AFFINE: return selftest_group_law_op<C, GL_DBL_AFFINE>(in, n, out, unit_info);
    default: return selftest_group_law_op<C, GL_REDUCE>(in, n, out, unit_info);
  }
}
}  // namespace
