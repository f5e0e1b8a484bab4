// bh_selftest_ntt_butterfly: the NTT's butterflies, reductions and store-path transformations
// (ntt_butterfly.cuh, what k_ntt_pass runs between its LDS loads and stores) on caller-chosen raw
// limbs (tests/test_gpu_ntt_butterfly.py; not part of the public ABI, declared in api_internal.h).
//
// The butterflies keep sums and differences limb-wise, feed fe_mul<FrCfg> unnormalised operands,
// reduce with an FP64 quotient and let DIT values grow lazily; a transform only ever meets those
// paths at pseudo-random representatives.  Here the test chooses every operand's limbs -- the
// contract's maxima, the orderings that make a difference negative before its bias, a top limb
// that wraps -- and reads the raw result.  One case per thread, one kernel per kind.
#include "api_internal.h"
#include "ntt_butterfly.cuh"

namespace {
enum : int {
  NB_DIF2 = 0, NB_DIF2_UNIT = 1, NB_DIT2 = 2, NB_DIT2_UNIT = 3,
  NB_DIF4 = 4, NB_DIF4_UNIT = 5, NB_DIT4 = 6, NB_DIT4_UNIT = 7,
  NB_QREDUCE = 8, NB_NORM = 9,
  NB_STORE_PLAIN = 10, NB_STORE_SCALARS = 11, NB_STORE_PRODUCT = 12,
  NB_KINDS = 13
};
constexpr int NL = FrCfg::N;  // words per operand

// operands (9 raw limbs each) and output words per case
constexpr int nb_inputs(int kind) {
  return kind <= NB_DIT2_UNIT ? 3 : kind <= NB_DIT4_UNIT ? 7 : kind <= NB_NORM ? 1 : 3;
}
constexpr int nb_outputs(int kind) {
  return kind <= NB_DIT2_UNIT ? 2 * NL : kind <= NB_DIT4_UNIT ? 4 * NL : kind == NB_STORE_SCALARS ? 8 : NL;
}

template <int KIND>
__global__ void __launch_bounds__(64) k_selftest_ntt_butterfly(const uint32_t* in, uint32_t* out, uint32_t n) {
  constexpr int NIN = nb_inputs(KIND), NOUT = nb_outputs(KIND);
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  DFr f[NIN];
#pragma unroll
  for (int k = 0; k < NIN; k++)
#pragma unroll
    for (int l = 0; l < NL; l++) f[k].v[l] = in[((size_t)t * NIN + k) * NL + l];
  uint32_t* dst = out + (size_t)t * NOUT;
  auto put = [&](int k, const DFr& v) {
#pragma unroll
    for (int l = 0; l < NL; l++) dst[k * NL + l] = v.v[l];
  };
  auto op = [&](int k) { return [&f, k] { return f[k]; }; };  // an operand as the callable the functions take
  if constexpr (KIND <= NB_DIT2_UNIT) {  // x, y, w
    constexpr bool unit = KIND == NB_DIF2_UNIT || KIND == NB_DIT2_UNIT;
    DFr nx, ny;
    if constexpr (KIND <= NB_DIF2_UNIT) bh::ntt_dif2(f[0], f[1], op(2), unit, nx, ny);
    else bh::ntt_dit2(f[0], f[1], op(2), unit, nx, ny);
    put(0, nx);
    put(1, ny);
  } else if constexpr (KIND <= NB_DIT4_UNIT) {  // x0..x3, then DIF: wa0, wa1, wb; DIT: wa, wb0, wb1
    constexpr bool unit = KIND == NB_DIF4_UNIT || KIND == NB_DIT4_UNIT;
    const DFr x[4] = {f[0], f[1], f[2], f[3]};
    DFr y[4];
    if constexpr (KIND <= NB_DIF4_UNIT) bh::ntt_dif4(x, f[4], f[5], op(6), unit, y);
    else bh::ntt_dit4(x, op(4), op(5), op(6), unit, y);
#pragma unroll
    for (int q = 0; q < 4; q++) put(q, y[q]);
  } else if constexpr (KIND == NB_QREDUCE) {
    put(0, bh::fr_qreduce(f[0]));
  } else if constexpr (KIND == NB_NORM) {
    put(0, bh::lw_norm(f[0]));
  } else if constexpr (KIND == NB_STORE_PLAIN) {  // x, sub, flags (limb 0; bit 0: lazy, bit 1: sub is set)
    DFr x = f[0];
    bh::ntt_store_plain(x, (f[2].v[0] & 1u) != 0, (f[2].v[0] & 2u) != 0, op(1));
    put(0, x);
  } else if constexpr (KIND == NB_STORE_SCALARS) {  // x, sub, flags (bit 1: sub is set)
    DFr x = f[0];
    uint32_t w8[8];
    bh::ntt_store_scalars(x, (f[2].v[0] & 2u) != 0, op(1), w8);
#pragma unroll
    for (int l = 0; l < 8; l++) dst[l] = w8[l];
  } else {  // pa, x, k
    put(0, bh::ntt_store_product(f[0], f[1], f[2]));
  }
}

template <int KIND>
bh_status selftest_ntt_kind(const uint32_t* in, size_t n, uint32_t* out) {
  const size_t in_b = n * nb_inputs(KIND) * NL * 4, out_b = n * nb_outputs(KIND) * 4;
  bh::DevBuf din, dout;
  BH_TRY_HIP(din.alloc(in_b));
  BH_TRY_HIP(dout.alloc(out_b));
  BH_TRY_HIP(hipMemcpy(din.p, in, in_b, hipMemcpyHostToDevice));
  hipLaunchKernelGGL((k_selftest_ntt_butterfly<KIND>), dim3((unsigned)((n + 63) / 64)), dim3(64), 0, nullptr,
                     din.as<uint32_t>(), dout.as<uint32_t>(), (uint32_t)n);
  BH_TRY_HIP(hipGetLastError());
  BH_TRY_HIP(hipMemcpy(out, dout.p, out_b, hipMemcpyDeviceToHost));
  return BH_OK;
}
}  // namespace

// n cases of nb_inputs(kind) operands (9 raw limbs each, used exactly as given) -> nb_outputs(kind)
// words per case.  kind 0..3: radix-2 DIF, DIF with the unit twiddle, DIT, DIT unit (x, y, w ->
// nx, ny); 4..7: radix-4 DIF, DIF with unit_b, DIT, DIT with unit_a (x0..x3 and wa0, wa1, wb (DIF)
// or wa, wb0, wb1 (DIT) -> y0..y3); 8: fr_qreduce, 9: lw_norm (x -> 9 limbs); 10: the plain store
// (x, sub, flags -> 9 limbs; flags' limb 0: bit 0 lazy, bit 1 sub is set); 11: the SCALARS epilogue
// (x, sub, flags -> 8 packed words); 12: the PRODUCT epilogue (pa, x, k -> 9 limbs).  A twiddle
// that a unit kind switches off is not read.
extern "C" bh_status bh_selftest_ntt_butterfly(int device, int kind, const uint32_t* in, size_t n, uint32_t* out) {
  if (kind < 0 || kind >= NB_KINDS || !in || !out || !n || n > (1u << 20)) return BH_ERR_INVALID_ARGUMENT;
  BH_TRY_HIP(hipSetDevice(device));
  switch (kind) {
    case NB_DIF2: return selftest_ntt_kind<NB_DIF2>(in, n, out);
    case NB_DIF2_UNIT: return selftest_ntt_kind<NB_DIF2_UNIT>(in, n, out);
    case NB_DIT2: return selftest_ntt_kind<NB_DIT2>(in, n, out);
    case NB_DIT2_UNIT: return selftest_ntt_kind<NB_DIT2_UNIT>(in, n, out);
    case NB_DIF4: return selftest_ntt_kind<NB_DIF4>(in, n, out);
    case NB_DIF4_UNIT: return selftest_ntt_kind<NB_DIF4_UNIT>(in, n, out);
    case NB_DIT4: return selftest_ntt_kind<NB_DIT4>(in, n, out);
    case NB_DIT4_UNIT: return selftest_ntt_kind<NB_DIT4_UNIT>(in, n, out);
    case NB_QREDUCE: return selftest_ntt_kind<NB_QREDUCE>(in, n, out);
    case NB_NORM: return selftest_ntt_kind<NB_NORM>(in, n, out);
    case NB_STORE_PLAIN: return selftest_ntt_kind<NB_STORE_PLAIN>(in, n, out);
    case NB_STORE_SCALARS: return selftest_ntt_kind<NB_STORE_SCALARS>(in, n, out);
    default: return selftest_ntt_kind<NB_STORE_PRODUCT>(in, n, out);
  }
}
