// Vectors of target-group values on the device: e(P_i, Q_i) per element, gt + gt, -gt,
// gt * Scalar and the 576-byte gt_format of the reference's gt_bytes.rs (32-74, 208-245), whose
// values are those of the bls12_381 crate.  With e0(P, Q) the value of this library's own
// convention (pairing_dev.hip: the loop over |x|, lines scaled by w^3, the exact exponent
// (p^12 - 1) / r), crate(P, Q) = conj(e0(P, Q))^3: the conjugate for the sign of x, the cube for the
// "3 h" hard part (final_exp_chain.h).  A bh_gt holds crate values on the library's flat basis
// sum_k c_k w^k (the crate's c0 + c1 w over Fp6 = (a0, a1, a2) is [c0.a0, c1.a0, c0.a1, c1.a1,
// c0.a2, c1.a2]), fully reduced, in the word-major lane layout of the pairing workspace (gt.h).
//
// A Gt value lies in the cyclotomic subgroup, f^(p^4 - p^2 + 1) = 1, so its inverse is its
// conjugate and its square needs three squarings in Fp4 = Fp2[s]/(s^2 - xi), s = w^3 (Granger,
// Scott, "Faster squaring in the cyclotomic subgroup of sixth degree extensions"): with
// A = c0 + c3 s, B = c1 + c4 s, C = c2 + c5 s and bar: s -> -s,
//   f^2 = (3 A^2 - 2 Abar) + (3 s C^2 + 2 Bbar) w + (3 B^2 - 2 Cbar) w^2,
// each Fp4 square (x + y s)^2 = (x^2 + xi y^2) + ((x + y)^2 - x^2 - y^2) s three Fp2 squarings: 9 Fp2
// squarings against the 36 Fp2 products of f12_mul_dense(a, a).
//
//   k_gt_cyc_sqr    that formula on n arbitrary Fp12 values (bh_selftest_gt_cyclotomic_square: a
//                   polynomial map, so tests/gt_values.py's model predicts it for any input)
//   k_gt_table      g^1 .. g^8 of a chunk's lanes in table slots of a global workspace
//   k_gt_pow_win    windows [hi, lo] of g^k: signed 4-bit digits by the biased-nibble recoding of
//                   k_varbase_mul_win (digit_j = nibble_j(k + 0x88..8) - 8, no carry chain), per
//                   window four cyclotomic squarings and at most one dense product with a table
//                   entry, conjugated on load for a negative digit; the first window only loads.
//                   The accumulator is double-buffered in global memory; all state is in memory, so
//                   the host splits the 64 windows over launches (GT_WINDOWS_PER_LAUNCH).
//   k_gt_finish     slot 0 after the final exponentiation's chain, m = e0, to conj(m)^3
//   k_gt_mul, k_gt_conj, k_gt_decode, k_gt_encode, k_gt_cyclotomic, k_gt_is_one
//                   the elementwise product, the copy (conjugating or not) between two layouts, the
//                   codec between bytes and Montgomery words with a status word per lane for a
//                   coefficient >= p, and the two halves of the membership test.
// The sum of a vector is pairing_dev.hip's k_f12_product on a copy.
//
// Plain C++ over field.cuh's templates; its lazy bounds (products < 2p for inputs < 128p) are
// tracked in the comments next to each fe_sub<K>.  Every value at rest is fully reduced (< p).
#include <string.h>

#include <algorithm>
#include <memory>

#include "f12_dev.cuh"
#include "final_exp_chain.h"
#include "gt.h"
#include "pairing_dev.h"
#include "point_codec.cuh"
#include "varbase.h"

using namespace bh;

namespace bh {

namespace {

// ---------------------------------------------------------------- device functions
// Both functions below are inlined into their kernels, one body per kernel: a called device
// function keeps a frame in the private segment (f12_mul_dense's 8 B per lane in pairing_dev.hip's
// kernels are that), and these kernels have no scratch.
//
// out[io] = the cyclotomic-squaring formula of a[ia]; out must not be a's buffer.  a's
// coefficients are < p.
__device__ __forceinline__ void gt_cyc_sqr(const uint32_t* a, size_t ia, uint32_t* out, size_t io, size_t stride) {
#pragma unroll 1
  for (int t = 0; t < 3; t++) {  // A = (c0, c3), B = (c1, c4), C = (c2, c5)
    // x^2 + xi y^2 goes to coefficient 2 t, ((x + y)^2 - x^2 - y^2) s to 2 t + 3; C's square is
    // multiplied by s first: s (S0 + S1 s) = xi S1 + S0 s, coefficients 1 and 4
    const int d0 = 2 * t, d1 = t == 2 ? 1 : 2 * t + 3;
    // the three Fp2 squarings x^2, y^2, (x + y)^2 around one body; the operands are reloaded, so
    // that only the two sums stay live across a squaring
    DFp2 S0 = F2::zero(), S1 = F2::zero();
#pragma unroll 1
    for (int q = 0; q < 3; q++) {
      DFp2 v = ld_fp2(a, stride, ia, 24 * (q == 1 ? t + 3 : t));
      if (q == 2) v = F2::add(v, ld_fp2(a, stride, ia, 24 * (t + 3)));  // x + y < 2p
      const DFp2 sq = F2::sqr(v);                                       // < 2p
      if (q == 0) {
        S0 = sq;
        S1 = F2::sub<2>(S1, sq);  // -x^2: 2p - sq <= 2p
      } else if (q == 1) {
        // S0 = x^2 + xi y^2, xi y^2 = (c0 - c1) + (c0 + c1) u: sq.c1 < 2p, < 2p + 4p = 6p; < 6p
        S0.c0 = fe_add<FpCfg>(S0.c0, fe_sub<FpCfg, 2>(sq.c0, sq.c1));
        S0.c1 = fe_add<FpCfg>(S0.c1, fe_add<FpCfg>(sq.c0, sq.c1));
        S1 = F2::sub<2>(S1, sq);  // -x^2 - y^2: <= 2p + 2p = 4p
      } else {
        S1 = F2::add(S1, sq);  // (x + y)^2 - x^2 - y^2 < 4p + 2p = 6p
      }
    }
    // xi S1: S1.c1 < 6p <= 8p: c0 < 6p + 8p = 14p, c1 < 12p
    const DFp2 X1{fe_sub<FpCfg, 8>(S1.c0, S1.c1), fe_add<FpCfg>(S1.c0, S1.c1)};
    const DFp2 H = F2::select(t == 2, X1, S1);  // < 14p
    const DFp2 c0 = ld_fp2(a, stride, ia, 24 * d0), c1 = ld_fp2(a, stride, ia, 24 * d1);
    // 3 S0 - 2 c: 3 S0 < 18p, 2 c < 2p: < 20p
    const DFp2 r0 = F2::sub<2>(F2::add(F2::add(S0, S0), S0), F2::add(c0, c0));
    // 3 H + 2 c < 42p + 2p = 44p
    const DFp2 r1 = F2::add(F2::add(F2::add(H, H), H), F2::add(c1, c1));
    st_fp2(out, stride, io, 24 * d0, F2::reduce(r0));
    st_fp2(out, stride, io, 24 * d1, F2::reduce(r1));
  }
}

// f12_mul_dense (f12_dev.cuh) with b[ib] conjugated on load when conj_b: its odd coefficients
// negated (b's coefficients < p, so p - c <= p).  The bounds are f12_mul_dense's.  Every product of
// this unit goes through it, conjugating or not, so that it is inlined.
__device__ __forceinline__ void gt_mul_entry(const uint32_t* a, size_t ia, const uint32_t* b, size_t ib, bool conj_b,
                                             uint32_t* out, size_t io, size_t stride) {
#pragma unroll 1
  for (int k = 0; k < 6; k++) {
    DFp2 U = F2::zero(), W = F2::zero();
#pragma unroll 1
    for (int i = 0; i < 6; i++) {
      const bool wrap = i > k;
      const int j = wrap ? k - i + 6 : k - i;
      DFp2 bj = ld_fp2(b, stride, ib, 24 * j);
      const DFp2 nb{fe_neg<FpCfg, 1>(bj.c0), fe_neg<FpCfg, 1>(bj.c1)};
      bj = F2::select(conj_b && (j & 1), nb, bj);
      const DFp2 prod = F2::mul(ld_fp2(a, stride, ia, 24 * i), bj);
      if (wrap) W = F2::add(W, prod);
      else U = F2::add(U, prod);
    }
    st_fp2(out, stride, io, 24 * k, F2::reduce(fold_xi<16>(U, W)));
  }
}

__device__ __forceinline__ void copy_value(const uint32_t* src, size_t sstride, uint32_t* dst, size_t dstride,
                                           size_t lane) {
  for (int w = 0; w < FW; w++) dst[(size_t)w * dstride + lane] = src[(size_t)w * sstride + lane];
}

// ---------------------------------------------------------------- kernels
__global__ void __launch_bounds__(64) k_gt_cyc_sqr(const uint32_t* a, uint32_t* out, size_t n, size_t stride) {
  const size_t lane = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (lane >= n) return;
  gt_cyc_sqr(a, lane, out, lane, stride);
}

constexpr int GT_TABLE = 8;            // table slots: g^1 .. g^8
constexpr int GT_SLOTS = GT_TABLE + 2;  // and the accumulator's two buffers

// slot m of the workspace = in^(m + 1): the copy, its cyclotomic square, then products by slot 0
__global__ void __launch_bounds__(64) k_gt_table(const uint32_t* in, size_t istride, uint32_t* ws, size_t n,
                                                 size_t stride) {
  const size_t lane = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (lane >= n) return;
  const size_t slot = (size_t)FW * stride;
  copy_value(in, istride, ws, stride, lane);
  gt_cyc_sqr(ws, lane, ws + slot, lane, stride);
#pragma unroll 1
  for (int m = 2; m < GT_TABLE; m++)
    gt_mul_entry(ws + (m - 1) * slot, lane, ws, lane, false, ws + m * slot, lane, stride);
}

// Windows hi .. lo (63 is the top one) of the lanes' powers.  scalars: 8 little-endian words per
// element at the stride sstride (8, or 0 for one shared exponent: every branch below is then
// wave-uniform).  Any exponent k with k + 0x88..8 < 2^256 is taken: a canonical scalar (k < r) is,
// and so is r itself, the membership test's exponent (r = 0x73ed..., and 0x73 + 0x88 + 1 < 0x100).
// The accumulator is in slot GT_TABLE at every launch boundary.
__global__ void __launch_bounds__(64) k_gt_pow_win(uint32_t* ws, size_t n, size_t stride, const uint32_t* scalars,
                                                   int sstride, int hi, int lo) {
  const size_t lane = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (lane >= n) return;
  const uint4* sp = reinterpret_cast<const uint4*>(scalars + lane * (size_t)sstride);
  const uint4 s0 = sp[0], s1 = sp[1];
  uint32_t s[8] = {s0.x, s0.y, s0.z, s0.w, s1.x, s1.y, s1.z, s1.w};
  uint64_t carry = 0;
#pragma unroll
  for (int w = 0; w < 8; w++) {
    const uint64_t t = (uint64_t)s[w] + 0x88888888u + carry;
    s[w] = (uint32_t)t;
    carry = t >> 32;
  }
  // window hi to the top nibble of s[7]
  const int lead = 4 * (63 - hi);
  for (int k = 0; k < (lead >> 5); k++) {
#pragma unroll
    for (int w = 7; w > 0; w--) s[w] = s[w - 1];
    s[0] = 0;
  }
  const int rem = lead & 31;
  if (rem) {
#pragma unroll
    for (int w = 7; w > 0; w--) s[w] = (s[w] << rem) | (s[w - 1] >> (32 - rem));
    s[0] <<= rem;
  }
  const size_t slot = (size_t)FW * stride;
  uint32_t* acc = ws + GT_TABLE * slot;
  int cur = 0;  // which buffer holds the accumulator (0 at every launch boundary)
#pragma unroll 1
  for (int j = hi; j >= lo; j--) {
    const int d = (int)(s[7] >> 28) - 8;  // in [-8, 7]
#pragma unroll
    for (int w = 7; w > 0; w--) s[w] = (s[w] << 4) | (s[w - 1] >> 28);
    s[0] <<= 4;
    const int m = (d < 0 ? -d : d ? d : 1) - 1;
    if (j == 63) {  // the first window: the entry itself, or one
#pragma unroll 1
      for (int k = 0; k < 6; k++) {
        DFp2 c = ld_fp2(ws + m * slot, stride, lane, 24 * k);  // < p
        if (k & 1) c = F2::select(d < 0, F2::neg_canonical(c), c);
        if (!d) c = k ? F2::zero() : F2::one();
        st_fp2(acc, stride, lane, 24 * k, c);
      }
      continue;
    }
#pragma unroll 1
    for (int t = 0; t < 4; t++) {
      gt_cyc_sqr(acc + cur * slot, lane, acc + (cur ^ 1) * slot, lane, stride);
      cur ^= 1;
    }
    if (d) {
      gt_mul_entry(acc + cur * slot, lane, ws + m * slot, lane, d < 0, acc + (cur ^ 1) * slot, lane, stride);
      cur ^= 1;
    }
  }
  if (cur) copy_value(acc + slot, stride, acc, stride, lane);  // (a zero digit skips its product)
}

// slot 0 of the final exponentiation's workspace, m, to conj(m)^3 in the vector out: m^2 by the
// cyclotomic formula (m is in the cyclotomic subgroup after the chain's easy part; zero stays
// zero), m^3 by one dense product
__global__ void __launch_bounds__(64) k_gt_finish(uint32_t* ws, size_t n, size_t stride, uint32_t* out,
                                                  size_t ostride) {
  const size_t lane = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (lane >= n) return;
  const size_t slot = (size_t)FW * stride;
  gt_cyc_sqr(ws, lane, ws + slot, lane, stride);
  gt_mul_entry(ws + slot, lane, ws, lane, false, ws + 2 * slot, lane, stride);
#pragma unroll 1
  for (int k = 0; k < 6; k++) {
    const DFp2 c = ld_fp2(ws + 2 * slot, stride, lane, 24 * k);  // < p
    st_fp2(out, ostride, lane, 24 * k, (k & 1) ? F2::neg_canonical(c) : c);
  }
}

__global__ void __launch_bounds__(64) k_gt_mul(const uint32_t* a, const uint32_t* b, uint32_t* out, size_t n,
                                               size_t stride) {
  const size_t lane = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (lane >= n) return;
  gt_mul_entry(a, lane, b, lane, false, out, lane, stride);
}

// dst = src, or its conjugate, between two layouts
__global__ void __launch_bounds__(64) k_gt_conj(const uint32_t* src, size_t sstride, uint32_t* dst, size_t dstride,
                                                size_t n, int conj) {
  const size_t lane = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (lane >= n) return;
  if (!conj) {
    copy_value(src, sstride, dst, dstride, lane);
    return;
  }
#pragma unroll 1
  for (int k = 0; k < 6; k++) {
    const DFp2 c = ld_fp2(src, sstride, lane, 24 * k);  // < p
    st_fp2(dst, dstride, lane, 24 * k, (k & 1) ? F2::neg_canonical(c) : c);
  }
}

// The Fp at position j (0..11) of a 576-byte record -> its first word in a value's 144.
// flat: c[0].c0, c[0].c1, ..., c[5].c1.  gt_format: the Fp2 coefficients of w^5, w^3, w^1, w^4, w^2,
// w^0, each c1 then c0.
__device__ __forceinline__ int record_word(int j, int gt_format) {
  if (!gt_format) return 12 * j;
  const int q = j >> 1, k = q < 3 ? 5 - 2 * q : 10 - 2 * q;
  return 24 * k + ((j & 1) ? 0 : 12);
}

// n records of twelve 48-byte big-endian coefficients -> fully reduced Montgomery words;
// status[lane] = 1 for a coefficient >= p (the lane's words are then defined but meaningless)
__global__ void __launch_bounds__(64) k_gt_decode(const uint32_t* in, size_t n, int gt_format, uint32_t* dst,
                                                  size_t dstride, uint32_t* status) {
  const size_t lane = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (lane >= n) return;
  bool bad = false;
#pragma unroll 1
  for (int j = 0; j < 12; j++) {
    uint32_t w[12];
#pragma unroll
    for (int i = 0; i < 12; i++) w[i] = __builtin_bswap32(in[lane * FW + 12 * j + 11 - i]);
    const DFp c = fe_unpack<FpCfg>(w);
    bad = bad || fe_geq_p(c);
    fe_pack<FpCfg>(fe_reduce_full<FpCfg>(to_mont(c)), w);  // c < 2^384 < 10p: the product < 2p
    const int w0 = record_word(j, gt_format);
#pragma unroll
    for (int i = 0; i < 12; i++) dst[(size_t)(w0 + i) * dstride + lane] = w[i];
  }
  status[lane] = bad;
}

__global__ void __launch_bounds__(64) k_gt_encode(const uint32_t* src, size_t sstride, size_t n, int gt_format,
                                                  uint32_t* out) {
  const size_t lane = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (lane >= n) return;
#pragma unroll 1
  for (int j = 0; j < 12; j++) {
    uint32_t w[12];
    const int w0 = record_word(j, gt_format);
#pragma unroll
    for (int i = 0; i < 12; i++) w[i] = src[(size_t)(w0 + i) * sstride + lane];
    fe_pack<FpCfg>(to_canonical(fe_unpack<FpCfg>(w)), w);
#pragma unroll
    for (int i = 0; i < 12; i++) out[lane * FW + 12 * j + 11 - i] = __builtin_bswap32(w[i]);
  }
}

// ok[lane] = frob^4(f) f == frob^2(f), i.e. f^(p^4 - p^2 + 1) = 1 (zero passes and fails the
// second half), through slots 0..3 of the workspace.  g2: final_exp_chain.h's frob^2 constants, 12
// packed words each.
__global__ void __launch_bounds__(64) k_gt_cyclotomic(const uint32_t* in, size_t istride, uint32_t* ws, size_t n,
                                                      size_t stride, const uint32_t* g2, uint32_t* ok) {
  const size_t lane = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (lane >= n) return;
  const size_t slot = (size_t)FW * stride;
  copy_value(in, istride, ws, stride, lane);
#pragma unroll 1
  for (int r = 0; r < 2; r++) {  // slot 1 = frob^2(f), slot 2 = frob^4(f)
#pragma unroll 1
    for (int k = 0; k < 6; k++) {
      const DFp2 c = ld_fp2(ws + r * slot, stride, lane, 24 * k);
      const DFp g = fe_unpack<FpCfg>(g2 + 12 * k);
      st_fp2(ws + (r + 1) * slot, stride, lane, 24 * k,
             F2::reduce(DFp2{fe_mul<FpCfg>(c.c0, g), fe_mul<FpCfg>(c.c1, g)}));
    }
  }
  gt_mul_entry(ws + 2 * slot, lane, ws, lane, false, ws + 3 * slot, lane, stride);
  uint32_t diff = 0;  // both sides are fully reduced: equal values have equal words
  for (int w = 0; w < FW; w++) diff |= ws[3 * slot + (size_t)w * stride + lane] ^ ws[slot + (size_t)w * stride + lane];
  ok[lane] = diff == 0;
}

// ok[lane] &= the accumulator is one
__global__ void __launch_bounds__(64) k_gt_is_one(const uint32_t* acc, size_t n, size_t stride, uint32_t* ok) {
  const size_t lane = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (lane >= n) return;
  uint32_t one[12], diff = 0;
  fe_pack<FpCfg>(fe_one<FpCfg>(), one);
  for (int w = 0; w < FW; w++) diff |= acc[(size_t)w * stride + lane] ^ (w < 12 ? one[w] : 0u);
  if (diff) ok[lane] = 0;
}

// ---------------------------------------------------------------- host
inline unsigned nb64(size_t n) { return (unsigned)((n + 63) / 64); }
inline size_t up64(size_t n) { return (std::max<size_t>(n, 1) + 63) / 64 * 64; }

// Lanes per pass of an exponentiation: the workspace holds GT_SLOTS values per lane, 5 760 B, so
// 360 MiB at this chunk.
constexpr size_t GT_CHUNK = (size_t)1 << 16;
// Windows per launch, from counted work in units of one dense Fp12 product (36 Fp2 products, about
// 108 Fp products' worth): a cyclotomic squaring is 9 Fp2 squarings, 18 Fp products, a sixth; a
// window is four of them and at most one product, 1.67 units; 16 windows are 26.7 units.
// k_fexp_steps was measured at 1.06 ms per 8 units at 2^14 lanes; scaled by the lane count, 3.5 ms
// per launch there and 14 ms at GT_CHUNK lanes, a tenth of the library's longest dispatch
// (k_varbase_mul_win<G2>, 147 ms per 2^20).  A count, not a measurement.
constexpr int GT_WINDOWS_PER_LAUNCH = 16;
constexpr size_t GT_MAX = (size_t)1 << 32;  // lanes of 64 stay within a 32-bit grid

// r, the membership test's exponent, as 8 little-endian words
constexpr uint32_t GT_R_WORDS[8] = {0x00000001u, 0xffffffffu, 0xfffe5bfeu, 0x53bda402u,
                                    0x09a1d805u, 0x3339d808u, 0x299d7d48u, 0x73eda753u};

bh_status gt_alloc(bh_ctx* ctx, size_t n, bh_gt* g) {
  g->ctx = ctx;
  g->n = n;
  g->stride = up64(n);
  BH_TRY_HIP(g->v.alloc((size_t)FW * g->stride * 4));
  return BH_OK;
}

struct PowWork {
  DevBuf ws;
  size_t stride = 0;
  bh_status alloc(size_t n) {
    stride = up64(std::min(n, GT_CHUNK));
    BH_TRY_HIP(ws.alloc((size_t)GT_SLOTS * FW * stride * 4));
    return BH_OK;
  }
  uint32_t* acc() const { return ws.as<uint32_t>() + (size_t)GT_TABLE * FW * stride; }
};

// the powers of the m lanes at `in` by the exponents at d_sc, left in w.acc(); enqueued
bh_status pow_enqueue(bh_ctx* ctx, const PowWork& w, const uint32_t* in, size_t istride, size_t m,
                      const uint32_t* d_sc, int sstride) {
  uint32_t* ws = w.ws.as<uint32_t>();
  hipLaunchKernelGGL(k_gt_table, dim3(nb64(m)), dim3(64), 0, ctx->stream, in, istride, ws, m, w.stride);
  BH_TRY_HIP(hipGetLastError());
  for (int hi = 63; hi >= 0; hi -= GT_WINDOWS_PER_LAUNCH) {
    hipLaunchKernelGGL(k_gt_pow_win, dim3(nb64(m)), dim3(64), 0, ctx->stream, ws, m, w.stride, d_sc, sstride, hi,
                       std::max(hi - GT_WINDOWS_PER_LAUNCH + 1, 0));
    BH_TRY_HIP(hipGetLastError());
  }
  return BH_OK;
}

// out[i] = a[i]^(scalar i), scalars on the device at the stride sstride (8 or 0); out is allocated
// here; returns synchronised
bh_status gt_pow(bh_ctx* ctx, const bh_gt* a, const uint32_t* d_sc, int sstride, bh_gt* out) {
  if (bh_status s = gt_alloc(ctx, a->n, out)) return s;
  if (!a->n) return BH_OK;
  PowWork w;
  if (bh_status s = w.alloc(a->n)) return s;
  for (size_t base = 0; base < a->n; base += GT_CHUNK) {
    const size_t m = std::min(GT_CHUNK, a->n - base);
    if (bh_status s = pow_enqueue(ctx, w, a->v.as<uint32_t>() + base, a->stride, m, d_sc + base * (size_t)sstride,
                                  sstride))
      return s;
    hipLaunchKernelGGL(k_gt_conj, dim3(nb64(m)), dim3(64), 0, ctx->stream, w.acc(), w.stride,
                       out->v.as<uint32_t>() + base, out->stride, m, 0);
    BH_TRY_HIP(hipGetLastError());
  }
  BH_TRY_HIP(hipStreamSynchronize(ctx->stream));  // the workspace is freed on return
  return BH_OK;
}

// frob^4(f) f = frob^2(f), then f^r = 1, for every element; returns synchronised
bh_status gt_check_members(bh_ctx* ctx, const bh_gt* a) {
  if (!a->n) return BH_OK;
  FexpTables t;  // for the frob^2 constants
  if (bh_status s = fexp_tables(ctx, &t)) return s;
  PowWork w;
  if (bh_status s = w.alloc(a->n)) return s;
  DevBuf ok, rw;
  BH_TRY_HIP(ok.alloc(a->n * 4));
  BH_TRY_HIP(rw.alloc(sizeof GT_R_WORDS));
  BH_TRY_HIP(hipMemcpyAsync(rw.p, GT_R_WORDS, sizeof GT_R_WORDS, hipMemcpyHostToDevice, ctx->stream));
  for (size_t base = 0; base < a->n; base += GT_CHUNK) {
    const size_t m = std::min(GT_CHUNK, a->n - base);
    const uint32_t* in = a->v.as<uint32_t>() + base;
    hipLaunchKernelGGL(k_gt_cyclotomic, dim3(nb64(m)), dim3(64), 0, ctx->stream, in, a->stride, w.ws.as<uint32_t>(), m,
                       w.stride, t.consts.as<uint32_t>() + 144, ok.as<uint32_t>() + base);
    BH_TRY_HIP(hipGetLastError());
    if (bh_status s = pow_enqueue(ctx, w, in, a->stride, m, rw.as<uint32_t>(), 0)) return s;
    hipLaunchKernelGGL(k_gt_is_one, dim3(nb64(m)), dim3(64), 0, ctx->stream, w.acc(), m, w.stride,
                       ok.as<uint32_t>() + base);
    BH_TRY_HIP(hipGetLastError());
  }
  std::vector<uint32_t> h(a->n);
  BH_TRY_HIP(hipMemcpyAsync(h.data(), ok.p, a->n * 4, hipMemcpyDeviceToHost, ctx->stream));
  BH_TRY_HIP(hipStreamSynchronize(ctx->stream));
  for (uint32_t v : h)
    if (!v) return BH_ERR_NOT_IN_SUBGROUP;
  return BH_OK;
}

// m records at the host address `bytes` -> dst (lane 0 of the call at dst[0]); raw and st: device
// staging of m records and m words.  Returns synchronised; BH_ERR_INVALID_ENCODING: a coefficient >= p.
bh_status decode_records(bh_ctx* ctx, const uint8_t* bytes, size_t m, int gt_format, uint32_t* dst, size_t dstride,
                         DevBuf& raw, DevBuf& st) {
  BH_TRY_HIP(hipMemcpyAsync(raw.p, bytes, m * 576, hipMemcpyHostToDevice, ctx->stream));
  hipLaunchKernelGGL(k_gt_decode, dim3(nb64(m)), dim3(64), 0, ctx->stream, raw.as<uint32_t>(), m, gt_format, dst,
                     dstride, st.as<uint32_t>());
  BH_TRY_HIP(hipGetLastError());
  std::vector<uint32_t> h(m);
  BH_TRY_HIP(hipMemcpyAsync(h.data(), st.p, m * 4, hipMemcpyDeviceToHost, ctx->stream));
  BH_TRY_HIP(hipStreamSynchronize(ctx->stream));
  for (uint32_t v : h)
    if (v) return BH_ERR_INVALID_ENCODING;
  return BH_OK;
}

// lanes [first, first + n) of src as records at the host address out; returns synchronised
bh_status encode_records(bh_ctx* ctx, const uint32_t* src, size_t sstride, size_t n, int gt_format, uint8_t* out) {
  const size_t chunk = std::min(n, MILLER_CHUNK);
  DevBuf raw;
  BH_TRY_HIP(raw.alloc(chunk * 576));
  for (size_t base = 0; base < n; base += chunk) {
    const size_t m = std::min(chunk, n - base);
    hipLaunchKernelGGL(k_gt_encode, dim3(nb64(m)), dim3(64), 0, ctx->stream, src + base, sstride, m, gt_format,
                       raw.as<uint32_t>());
    BH_TRY_HIP(hipGetLastError());
    BH_TRY_HIP(hipMemcpyAsync(out + 576 * base, raw.p, 576 * m, hipMemcpyDeviceToHost, ctx->stream));
    BH_TRY_HIP(hipStreamSynchronize(ctx->stream));
  }
  return BH_OK;
}

void gt_format_host(const Fp12& f, uint8_t out[576]) {
  static const int ORDER[6] = {5, 3, 1, 4, 2, 0};
  for (int q = 0; q < 6; q++) {
    fp_to_be(f.c[ORDER[q]].c1, out + 96 * q);
    fp_to_be(f.c[ORDER[q]].c0, out + 96 * q + 48);
  }
}

// the product of a's elements (one for none) on a copy; returns synchronised
bh_status gt_sum(bh_ctx* ctx, const bh_gt* a, uint8_t out[576]) {
  Fp12 r = f12_one();
  if (a->n) {
    const size_t slot = (size_t)FW * a->stride;
    DevBuf ws;
    BH_TRY_HIP(ws.alloc(3 * slot * 4));
    BH_TRY_HIP(hipMemcpyAsync(ws.p, a->v.p, slot * 4, hipMemcpyDeviceToDevice, ctx->stream));
    uint32_t* f = ws.as<uint32_t>();
    if (bh_status s = f12_lanes_product(ctx, f, f + slot, f + 2 * slot, a->stride, a->n, &r)) return s;
  }
  gt_format_host(r, out);
  return BH_OK;
}

// canonical scalars on the host -> the device; a scalar >= r: BH_ERR_INVALID_ARGUMENT
bh_status gt_scalars(bh_ctx* ctx, const uint64_t* scalars, size_t count, DevBuf* d_sc) {
  for (size_t i = 0; i < count; i++)
    if (!scalar_below_r(scalars + 4 * i)) return BH_ERR_INVALID_ARGUMENT;
  BH_TRY_HIP(d_sc->alloc(std::max<size_t>(count, 1) * 32));
  if (count) {
    BH_TRY_HIP(hipMemcpyAsync(d_sc->p, scalars, count * 32, hipMemcpyHostToDevice, ctx->stream));
    BH_TRY_HIP(hipStreamSynchronize(ctx->stream));
  }
  return BH_OK;
}

bool on_device(const bh_ctx* ctx, const bh_gt* g) { return g && g->ctx && g->ctx->device == ctx->device; }

// the final exponentiation's chain on slot 0 of ws, then conj(m)^3 into out at lane `base`; enqueued
bh_status finish_enqueue(bh_ctx* ctx, const FexpTables& t, uint32_t* ws, size_t m, size_t stride, bh_gt* out,
                         size_t base) {
  if (bh_status s = fexp_enqueue(ctx, t, ws, m, stride)) return s;
  hipLaunchKernelGGL(k_gt_finish, dim3(nb64(m)), dim3(64), 0, ctx->stream, ws, m, stride,
                     out->v.as<uint32_t>() + base, out->stride);
  BH_TRY_HIP(hipGetLastError());
  return BH_OK;
}

// the common prologue of an entry point that runs kernels (the caller has locked ctx->mu)
bh_status enter(bh_ctx* ctx) {
  BH_TRY_HIP(hipSetDevice(ctx->device));
  return scratch_check(ctx);
}

}  // namespace

void gt_kernels(std::vector<KernInfo>& v) {
  v.push_back({"k_gt_cyc_sqr", (const void*)k_gt_cyc_sqr, 64, 0});
  v.push_back({"k_gt_table", (const void*)k_gt_table, 64, 0});
  v.push_back({"k_gt_pow_win", (const void*)k_gt_pow_win, 64, 0});
  v.push_back({"k_gt_finish", (const void*)k_gt_finish, 64, 0});
  v.push_back({"k_gt_mul", (const void*)k_gt_mul, 64, 0});
  v.push_back({"k_gt_conj", (const void*)k_gt_conj, 64, 0});
  v.push_back({"k_gt_decode", (const void*)k_gt_decode, 64, 0});
  v.push_back({"k_gt_encode", (const void*)k_gt_encode, 64, 0});
  v.push_back({"k_gt_cyclotomic", (const void*)k_gt_cyclotomic, 64, 0});
  v.push_back({"k_gt_is_one", (const void*)k_gt_is_one, 64, 0});
}

}  // namespace bh

extern "C" {

bh_status bh_gt_pairing(bh_ctx* ctx, const bh_srs* g1, size_t off1, const bh_srs* g2, size_t off2, size_t n,
                        bh_gt** out) {
  if (!ctx || !g1 || !g2 || !out || !g1->ctx || !g2->ctx || g1->ctx->device != ctx->device ||
      g2->ctx->device != ctx->device)
    return BH_ERR_INVALID_ARGUMENT;
  if (g1->group != BH_G1 || g2->group != BH_G2) return BH_ERR_INVALID_ARGUMENT;
  if (off1 > g1->n || n > g1->n - off1 || off2 > g2->n || n > g2->n - off2) return BH_ERR_INVALID_ARGUMENT;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (bh_status s = enter(ctx)) return s;
  std::unique_ptr<bh_gt> r(new bh_gt());
  if (bh_status s = gt_alloc(ctx, n, r.get())) return s;
  if (n) {
    FexpTables t;
    if (bh_status s = fexp_tables(ctx, &t)) return s;
    for (size_t base = 0; base < n; base += MILLER_CHUNK) {
      const size_t m = std::min(MILLER_CHUNK, n - base);
      MillerWork w;
      if (bh_status s = miller_lanes(ctx, g1->pts.as<uint32_t>() + (off1 + base) * 24,
                                     g2->pts.as<uint32_t>() + (off2 + base) * 48, m, 1, FE_SLOTS, &w))
        return s;
      if (bh_status s = finish_enqueue(ctx, t, w.f.as<uint32_t>(), m, w.stride, r.get(), base)) return s;
      BH_TRY_HIP(hipStreamSynchronize(ctx->stream));  // the workspace is freed at the end of the pass
    }
  }
  *out = r.release();
  return BH_OK;
}

bh_status bh_gt_from_miller(bh_ctx* ctx, const uint8_t* f, size_t n, bh_gt** out) {
  if (!ctx || !out || (n && !f) || n > GT_MAX) return BH_ERR_INVALID_ARGUMENT;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (bh_status s = enter(ctx)) return s;
  std::unique_ptr<bh_gt> r(new bh_gt());
  if (bh_status s = gt_alloc(ctx, n, r.get())) return s;
  if (n) {
    FexpTables t;
    if (bh_status s = fexp_tables(ctx, &t)) return s;
    const size_t chunk = std::min(n, MILLER_CHUNK), stride = up64(chunk);
    DevBuf raw, st, ws;
    BH_TRY_HIP(raw.alloc(chunk * 576));
    BH_TRY_HIP(st.alloc(chunk * 4));
    BH_TRY_HIP(ws.alloc((size_t)FE_SLOTS * FW * stride * 4));
    for (size_t base = 0; base < n; base += chunk) {
      const size_t m = std::min(chunk, n - base);
      if (bh_status s = decode_records(ctx, f + 576 * base, m, 0, ws.as<uint32_t>(), stride, raw, st)) return s;
      if (bh_status s = finish_enqueue(ctx, t, ws.as<uint32_t>(), m, stride, r.get(), base)) return s;
    }
    BH_TRY_HIP(hipStreamSynchronize(ctx->stream));  // the workspace is freed on return
  }
  *out = r.release();
  return BH_OK;
}

bh_status bh_gt_upload(bh_ctx* ctx, const uint8_t* bytes, size_t n, int checked, bh_gt** out) {
  if (!ctx || !out || (n && !bytes) || n > GT_MAX) return BH_ERR_INVALID_ARGUMENT;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (bh_status s = enter(ctx)) return s;
  std::unique_ptr<bh_gt> r(new bh_gt());
  if (bh_status s = gt_alloc(ctx, n, r.get())) return s;
  if (n) {
    const size_t chunk = std::min(n, MILLER_CHUNK);
    DevBuf raw, st;
    BH_TRY_HIP(raw.alloc(chunk * 576));
    BH_TRY_HIP(st.alloc(chunk * 4));
    for (size_t base = 0; base < n; base += chunk) {
      const size_t m = std::min(chunk, n - base);
      if (bh_status s = decode_records(ctx, bytes + 576 * base, m, 1, r->v.as<uint32_t>() + base, r->stride, raw, st))
        return s;
    }
    if (checked)
      if (bh_status s = gt_check_members(ctx, r.get())) return s;
  }
  *out = r.release();
  return BH_OK;
}

bh_status bh_gt_read(const bh_gt* gt, size_t first, size_t n, uint8_t* out) {
  if (!gt || !gt->ctx || (n && !out) || first > gt->n || n > gt->n - first) return BH_ERR_INVALID_ARGUMENT;
  if (!n) return BH_OK;
  bh_ctx* ctx = gt->ctx;
  std::lock_guard<std::mutex> lk(ctx->mu);
  BH_TRY_HIP(hipSetDevice(ctx->device));
  return encode_records(ctx, gt->v.as<uint32_t>() + first, gt->stride, n, 1, out);
}

size_t bh_gt_len(const bh_gt* gt) { return gt ? gt->n : 0; }

bh_status bh_gt_free(bh_gt* gt) {
  if (!gt) return BH_OK;
  if (gt->ctx) (void)hipSetDevice(gt->ctx->device);
  delete gt;
  return BH_OK;
}

bh_status bh_gt_add(bh_ctx* ctx, const bh_gt* a, const bh_gt* b, bh_gt** out) {
  if (!ctx || !out || !on_device(ctx, a) || !on_device(ctx, b) || a->n != b->n) return BH_ERR_INVALID_ARGUMENT;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (bh_status s = enter(ctx)) return s;
  std::unique_ptr<bh_gt> r(new bh_gt());
  if (bh_status s = gt_alloc(ctx, a->n, r.get())) return s;
  if (a->n) {
    hipLaunchKernelGGL(k_gt_mul, dim3(nb64(a->n)), dim3(64), 0, ctx->stream, a->v.as<uint32_t>(), b->v.as<uint32_t>(),
                       r->v.as<uint32_t>(), a->n, a->stride);
    BH_TRY_HIP(hipGetLastError());
    BH_TRY_HIP(hipStreamSynchronize(ctx->stream));
  }
  *out = r.release();
  return BH_OK;
}

bh_status bh_gt_neg(bh_ctx* ctx, const bh_gt* a, bh_gt** out) {
  if (!ctx || !out || !on_device(ctx, a)) return BH_ERR_INVALID_ARGUMENT;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (bh_status s = enter(ctx)) return s;
  std::unique_ptr<bh_gt> r(new bh_gt());
  if (bh_status s = gt_alloc(ctx, a->n, r.get())) return s;
  if (a->n) {
    hipLaunchKernelGGL(k_gt_conj, dim3(nb64(a->n)), dim3(64), 0, ctx->stream, a->v.as<uint32_t>(), a->stride,
                       r->v.as<uint32_t>(), r->stride, a->n, 1);
    BH_TRY_HIP(hipGetLastError());
    BH_TRY_HIP(hipStreamSynchronize(ctx->stream));
  }
  *out = r.release();
  return BH_OK;
}

bh_status bh_gt_mul_each(bh_ctx* ctx, const bh_gt* a, const uint64_t* scalars, size_t n_scalars, bh_gt** out) {
  if (!ctx || !out || !on_device(ctx, a) || (n_scalars && !scalars)) return BH_ERR_INVALID_ARGUMENT;
  if (n_scalars != a->n && n_scalars != 1) return BH_ERR_INVALID_ARGUMENT;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (bh_status s = enter(ctx)) return s;
  DevBuf d_sc;
  if (bh_status s = gt_scalars(ctx, scalars, n_scalars, &d_sc)) return s;
  std::unique_ptr<bh_gt> r(new bh_gt());
  if (bh_status s = gt_pow(ctx, a, d_sc.as<uint32_t>(), n_scalars == a->n ? 8 : 0, r.get())) return s;
  *out = r.release();
  return BH_OK;
}

bh_status bh_gt_sum(bh_ctx* ctx, const bh_gt* a, uint8_t out[576]) {
  if (!ctx || !out || !on_device(ctx, a)) return BH_ERR_INVALID_ARGUMENT;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (bh_status s = enter(ctx)) return s;
  return gt_sum(ctx, a, out);
}

bh_status bh_gt_multiexp(bh_ctx* ctx, const bh_gt* a, const uint64_t* scalars, uint8_t out[576]) {
  if (!ctx || !out || !on_device(ctx, a) || (a->n && !scalars)) return BH_ERR_INVALID_ARGUMENT;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (bh_status s = enter(ctx)) return s;
  DevBuf d_sc;
  if (bh_status s = gt_scalars(ctx, scalars, a->n, &d_sc)) return s;
  bh_gt powers;
  if (bh_status s = gt_pow(ctx, a, d_sc.as<uint32_t>(), 8, &powers)) return s;
  return gt_sum(ctx, &powers, out);
}

// tests/test_gpu_gt.py: the cyclotomic-squaring formula on n arbitrary Fp12 values, in and out in
// the flat 576-byte encoding of bh_miller_product
bh_status bh_selftest_gt_cyclotomic_square(bh_ctx* ctx, const uint8_t* in, size_t n, uint8_t* out) {
  if (!ctx || (n && (!in || !out)) || n > MILLER_CHUNK) return BH_ERR_INVALID_ARGUMENT;
  if (!n) return BH_OK;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (bh_status s = enter(ctx)) return s;
  const size_t stride = up64(n);
  DevBuf raw, st, ws;
  BH_TRY_HIP(raw.alloc(n * 576));
  BH_TRY_HIP(st.alloc(n * 4));
  BH_TRY_HIP(ws.alloc((size_t)2 * FW * stride * 4));
  uint32_t* a = ws.as<uint32_t>();
  if (bh_status s = decode_records(ctx, in, n, 0, a, stride, raw, st)) return s;
  hipLaunchKernelGGL(k_gt_cyc_sqr, dim3(nb64(n)), dim3(64), 0, ctx->stream, a, a + (size_t)FW * stride, n, stride);
  BH_TRY_HIP(hipGetLastError());
  return encode_records(ctx, a + (size_t)FW * stride, stride, n, 0, out);
}

}  // extern "C"
