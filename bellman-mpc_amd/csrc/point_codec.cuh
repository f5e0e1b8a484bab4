// Device helpers shared by the decoders of compressed points: the proof decoder (proofs_dev.hip) and
// the point-vector codec (point_codec.hip).  Constants derived from p, the canonical / Montgomery
// conversions and comparisons of the encoding's rules (range check, lex_largest), the fixed-exponent
// chains and the square roots over Fp and Fp2, the curve equation's right-hand side and the
// big-endian coordinate load.
//
// Square roots.  p = 3 mod 4.  Fp: y = a^((p+1)/4), a square iff y^2 = a.  Fp2 = Fp[u]/(u^2 + 1)
// (Adj, Rodriguez-Henriquez, "Square root computation over even extension fields", algorithm 9,
// the method of verify.cpp): a1 = a^((p-3)/4), x0 = a1 a, alpha = a1 x0 = a^((p-1)/2); alpha = -1:
// x = u x0, else x = (1 + alpha)^((p-1)/2) x0; a square iff x^2 = a.  a = 0 needs no case of its
// own (every intermediate is 0 except (1 + alpha)^... = 1).  Which of the two roots comes out does
// not matter: the sign flag selects by lex_largest on canonical values.  The exponents are
// compile-time constants, so the branch on an exponent bit is wave-uniform; each bit loop is
// #pragma unroll 1 around one squaring and one product.
//
// Plain C++ over field.cuh's templates; its lazy bounds (products < 2p for inputs < 128p) are
// tracked in the comments next to each fe_sub<K>.  Everything here has internal linkage: each unit
// that includes the header compiles its own copy into its own kernels.
#pragma once
#include "group_host.h"

namespace bh {

namespace {

using F2 = Fp2Ops;

// ---------------------------------------------------------------- constants derived from p
struct Exp12 {
  uint32_t w[12];
};
// (p + add) >> shift as 12 little-endian words; add in {+1, -1, -3} leaves p's low word without
// carry or borrow (p = ...aaab)
constexpr Exp12 p_exponent(int add, int shift) {
  uint64_t t[6] = {};
  for (int i = 0; i < 6; i++) t[i] = hostc::FP_P[i];
  t[0] = add >= 0 ? t[0] + (uint64_t)add : t[0] - (uint64_t)(-add);
  Exp12 e{};
  for (int i = 0; i < 6; i++) {
    const uint64_t v = (t[i] >> shift) | (i + 1 < 6 ? t[i + 1] << (64 - shift) : 0);
    e.w[2 * i] = (uint32_t)v;
    e.w[2 * i + 1] = (uint32_t)(v >> 32);
  }
  return e;
}
enum : int { EXP_P1_4 = 0, EXP_P3_4 = 1, EXP_P1_2 = 2 };  // (p+1)/4, (p-3)/4, (p-1)/2

__device__ __forceinline__ uint32_t exponent_word(int which, int w) {
  constexpr Exp12 E[3] = {p_exponent(1, 2), p_exponent(-3, 2), p_exponent(-1, 1)};
  return E[which].w[w];
}

// (p - 1) / 2 in 29-bit limbs (p is odd: p >> 1)
struct HalfLimbs {
  uint32_t v[FpCfg::N];
};
constexpr HalfLimbs half_p() {
  HalfLimbs l{};
  for (int i = 0; i < FpCfg::N; i++)
    l.v[i] = (FpCfg::P[i] >> 1) | (i + 1 < FpCfg::N ? (FpCfg::P[i + 1] & 1u) << (FpCfg::BITS - 1) : 0u);
  return l;
}
struct HalfP {
  static constexpr HalfLimbs value = half_p();
};

// ---------------------------------------------------------------- canonical values
// x >= p for normalised limbs (any value below 2^406)
__device__ __forceinline__ bool fe_geq_p(const DFp& x) {
  int32_t c = 0;
#pragma unroll
  for (int i = 0; i < FpCfg::N; i++) {
    const int32_t s = (int32_t)x.v[i] - (int32_t)KP<FpCfg, 1>::value.v[i] + c;
    c = s >> FpCfg::BITS;
  }
  return c >= 0;
}
// a > (p - 1) / 2 for a canonical (not Montgomery) value: fp_lex_largest of host_arith.h
__device__ __forceinline__ bool fe_gt_half(const DFp& a) {
  int32_t c = 0;
#pragma unroll
  for (int i = 0; i < FpCfg::N; i++) {
    const int32_t s = (int32_t)HalfP::value.v[i] - (int32_t)a.v[i] + c;
    c = s >> FpCfg::BITS;
  }
  return c < 0;
}
__device__ __forceinline__ DFp fe_r2() {
  DFp r2;
#pragma unroll
  for (int k = 0; k < FpCfg::N; k++) r2.v[k] = FpCfg::R2[k];
  return r2;
}
// canonical limbs (< p) -> Montgomery, < 2p
__device__ __forceinline__ DFp to_mont(const DFp& c) { return fe_mul<FpCfg>(c, fe_r2()); }
// Montgomery, fully reduced -> canonical limbs in [0, p) (fe_from_mont leaves <= p)
__device__ __forceinline__ DFp to_canonical(const DFp& m) { return fe_csub<FpCfg, 1>(fe_from_mont<FpCfg>(m)); }

// lex_largest of host_arith.h on fully reduced Montgomery values
__device__ __forceinline__ bool lex_largest(const DFp& y) { return fe_gt_half(to_canonical(y)); }
__device__ __forceinline__ bool lex_largest(const DFp2& y) {
  const DFp c1 = to_canonical(y.c1);
  return fe_gt_half(c1) || (fe_is_zero_canonical<FpCfg>(c1) && fe_gt_half(to_canonical(y.c0)));
}

// ---------------------------------------------------------------- fixed-exponent chains
// a^e for one of the exponents above; a < 128p, the result < 2p
__device__ DFp fp_pow(const DFp& a, int which) {
  DFp r = fe_one<FpCfg>();
#pragma unroll 1
  for (int w = 11; w >= 0; w--) {
    const uint32_t e = exponent_word(which, w);
#pragma unroll 1
    for (int b = 31; b >= 0; b--) {
      r = fe_sqr<FpCfg>(r);
      if ((e >> b) & 1u) r = fe_mul<FpCfg>(r, a);
    }
  }
  return r;
}
__device__ DFp2 fp2_pow(const DFp2& a, int which) {
  DFp2 r = F2::one();
#pragma unroll 1
  for (int w = 11; w >= 0; w--) {
    const uint32_t e = exponent_word(which, w);
#pragma unroll 1
    for (int b = 31; b >= 0; b--) {
      r = F2::sqr(r);
      if ((e >> b) & 1u) r = F2::mul(r, a);
    }
  }
  return r;
}

// The square-root routines of the decode kernels (and of bh_selftest_field_sqrt).  a < 8p in
// Montgomery form; *root (< 2p) is a root of a exactly when the return value is true.
__device__ bool field_sqrt(const DFp& a, DFp* root) {
  const DFp y = fp_pow(a, EXP_P1_4);
  *root = y;
  // y^2 < 2p, a < 8p: the difference is < 10p, below is_zero's 128p
  return fe_is_zero<FpCfg>(fe_sub<FpCfg, 8>(fe_sqr<FpCfg>(y), a));
}
__device__ bool field_sqrt(const DFp2& a, DFp2* root) {
  const DFp2 a1 = fp2_pow(a, EXP_P3_4);
  const DFp2 x0 = F2::mul(a1, a);
  const DFp2 alpha = F2::mul(a1, x0);
  // alpha + 1: components < 2p + p = 3p (is_zero below 128p; fp2_pow takes < 128p)
  const DFp2 alpha1{fe_add<FpCfg>(alpha.c0, fe_one<FpCfg>()), alpha.c1};
  const bool minus_one = F2::is_zero(alpha1);
  const DFp2 b = fp2_pow(alpha1, EXP_P1_2);  // 0 when alpha = -1: replaced below
  const DFp2 bx = F2::mul(b, x0);
  const DFp2 ux{fe_neg<FpCfg, 2>(x0.c1), x0.c0};  // u x0 = -x0.c1 + x0.c0 u; x0.c1 < 2p
  const DFp2 x = F2::select(minus_one, ux, bx);
  *root = x;
  // x^2 < 2p, a < 8p per component: the difference is < 10p
  return F2::is_zero(F2::sub<8>(F2::sqr(x), a));
}

// the curve constant in Montgomery form: 4 over Fp, 4 + 4u over Fp2; components < 4p
__device__ __forceinline__ DFp four() {
  const DFp two = fe_add<FpCfg>(fe_one<FpCfg>(), fe_one<FpCfg>());
  return fe_add<FpCfg>(two, two);
}
__device__ __forceinline__ DFp curve_rhs(const DFp& x) {  // x^3 + 4 < 6p for x < 128p
  return fe_add<FpCfg>(fe_mul<FpCfg>(fe_sqr<FpCfg>(x), x), four());
}
__device__ __forceinline__ DFp2 curve_rhs(const DFp2& x) {  // x^3 + 4 + 4u, components < 6p
  const DFp2 x3 = F2::mul(F2::sqr(x), x);
  return DFp2{fe_add<FpCfg>(x3.c0, four()), fe_add<FpCfg>(x3.c1, four())};
}

// One 48-byte big-endian coordinate at a word-aligned address as 12 little-endian words; its top
// three bits (the encoding's flags) are returned and, where `mask` is set, cleared.
__device__ __forceinline__ uint32_t ld_coordinate(const uint32_t* src, bool mask, uint32_t w[12]) {
#pragma unroll
  for (int i = 0; i < 12; i++) w[i] = __builtin_bswap32(src[11 - i]);
  const uint32_t flags = w[11] >> 29;
  if (mask) w[11] &= 0x1fffffffu;
  return flags;
}

}  // namespace

}  // namespace bh
