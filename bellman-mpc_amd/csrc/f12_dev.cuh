// Device helpers of the Fp12 arithmetic on the word-major lane workspace, shared by the Miller loop
// and final exponentiation (pairing_dev.hip) and the target group's kernels (gt.hip): the packed
// Fp2 load and store, the Fp2 inversion, the fold of the part of a product that wrapped past
// w^6 = xi, and the dense product.  Fp12 = Fp2[w]/(w^6 - xi), xi = 1 + u, a value the six Fp2
// coefficients of sum_k c_k w^k: 144 packed words c[0].c0, c[0].c1, ..., c[5].c1, word w of lane l
// at w * stride + l.
//
// Plain C++ over field.cuh's templates; its lazy bounds (products < 2p for inputs < 128p) are
// tracked in the comments next to each fe_sub<K>.  Everything here has internal linkage: each unit
// that includes the header compiles its own copy into its own kernels (a device function cannot be
// shared between translation units built without relocatable device code).
#pragma once
#include "group_host.h"

namespace bh {

namespace {

using F2 = Fp2Ops;
constexpr int FW = 144;  // packed words of an Fp12 value: c[0].c0, c[0].c1, ..., c[5].c1, 12 each

// ---------------------------------------------------------------- word-major lane storage
__device__ __forceinline__ DFp2 ld_fp2(const uint32_t* base, size_t stride, size_t lane, int word0) {
  uint32_t w[24];
#pragma unroll
  for (int j = 0; j < 24; j++) w[j] = base[(size_t)(word0 + j) * stride + lane];
  return F2::unpack(w);
}
// x < 2^384 (8p): every caller stores a product (< 2p) or a fully reduced value
__device__ __forceinline__ void st_fp2(uint32_t* base, size_t stride, size_t lane, int word0, const DFp2& x) {
  uint32_t w[24];
  F2::pack(x, w);
#pragma unroll
  for (int j = 0; j < 24; j++) base[(size_t)(word0 + j) * stride + lane] = w[j];
}

// (a + bu)^-1 = (a - bu) / (a^2 + b^2), the inversion in Fp by Fermat: crs.hip's Inv<Fp2Ops> (a
// device function cannot be shared between translation units built without relocatable device code)
__device__ DFp2 fp2_inv(const DFp2& x) {
  // p - 2, little-endian 32-bit words
  constexpr uint32_t E[12] = {0xffffaaa9u, 0xb9feffffu, 0xb153ffffu, 0x1eabfffeu, 0xf6b0f624u, 0x6730d2a0u,
                              0xf38512bfu, 0x64774b84u, 0x434bacd7u, 0x4b1ba7b6u, 0x397fe69au, 0x1a0111eau};
  const DFp t = fe_add<FpCfg>(fe_sqr<FpCfg>(x.c0), fe_sqr<FpCfg>(x.c1));
  DFp r = fe_one<FpCfg>();
#pragma unroll 1
  for (int w = 11; w >= 0; w--) {
#pragma unroll 1
    for (int b = 31; b >= 0; b--) {
      r = fe_sqr<FpCfg>(r);
      if ((E[w] >> b) & 1u) r = fe_mul<FpCfg>(r, t);
    }
  }
  DFp2 o;
  o.c0 = fe_mul<FpCfg>(x.c0, r);
  o.c1 = fe_mul<FpCfg>(fe_neg<FpCfg, 2>(x.c1), r);  // x.c1 < 2p at both call sites
  return o;
}

// ---------------------------------------------------------------- Fp12 products
// (U + xi W) for the unwrapped part U and the part W that wrapped past w^6 = xi = 1 + u:
// xi W = (W0 - W1) + (W0 + W1) u.  WK: W's components are < WK p.
template <uint32_t WK>
__device__ __forceinline__ DFp2 fold_xi(const DFp2& U, const DFp2& W) {
  DFp2 c;
  c.c0 = fe_add<FpCfg>(U.c0, fe_sub<FpCfg, WK>(W.c0, W.c1));
  c.c1 = fe_add<FpCfg>(U.c1, fe_add<FpCfg>(W.c0, W.c1));
  return c;
}

// out[io] = a[ia] * b[ib], all coefficients: c_k = sum_i a_i b_(k-i mod 6), the terms with i > k
// times xi.  out must not be a or b's buffer.  Bounds: U sums <= 6 products (< 12p), W <= 5
// (< 10p, so fe_sub<16>); the folded coefficient is < 12p + 10p + 16p = 38p < 128p (reduce).
__device__ void f12_mul_dense(const uint32_t* a, size_t ia, const uint32_t* b, size_t ib, uint32_t* out, size_t io,
                              size_t stride) {
#pragma unroll 1
  for (int k = 0; k < 6; k++) {
    DFp2 U = F2::zero(), W = F2::zero();
#pragma unroll 1
    for (int i = 0; i < 6; i++) {
      const bool wrap = i > k;
      const int j = wrap ? k - i + 6 : k - i;
      const DFp2 prod = F2::mul(ld_fp2(a, stride, ia, 24 * i), ld_fp2(b, stride, ib, 24 * j));
      if (wrap) W = F2::add(W, prod);
      else U = F2::add(U, prod);
    }
    st_fp2(out, stride, io, 24 * k, F2::reduce(fold_xi<16>(U, W)));
  }
}

}  // namespace

}  // namespace bh
