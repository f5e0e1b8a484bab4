// Device multi-Miller loop: prod_i f_{|x|,Q_i}(P_i) for affine G1 points P_i and affine twist
// points Q_i of two device vectors -- multi_miller_loop of the bls12_381 crate as the reference's
// verifier.rs and mpc.rs:787-804 use it, in exactly the conventions of verify.cpp (the host
// pairing) and oracle/pairing.py: Fp12 = Fp2[w]/(w^6 - xi), affine lines scaled by w^3,
//   l = (lam x_T - y_T) - lam x_P w^2 + y_P w^3,
// the 63 bits below the leading one of |x|, a pair with an identity contributing one.  Field
// arithmetic is exact and Fp12 is commutative, so the grouping below gives the host's value
// coefficient for coefficient (tests/test_gpu_pairing.py; the index algebra alone in
// tests/test_miller_batch_model_cpu.py).
//
//   k_miller_init    f = 1, T_k = Q_k and the lane's mask of pairs without an identity
//   k_miller_steps   bits [hi, lo] of the loop.  One lane owns K consecutive pairs and ONE Fp12
//                    value f: per bit one dense squaring of f, then for its K pairs a doubling step
//                    and, where |x| has a one, an addition step.  The K slopes of a step need K
//                    inversions, of 2 y_T (doubling) or x_Q - x_T (addition): Montgomery's trick as
//                    in k_normalize -- prefix products in a global scratch array, one Fermat
//                    inversion (about 460 Fp products) per lane and step, 3 Fp2 products per pair.
//   k_f12_product    the lanes' values multiplied by levels in the style of k_rowcol_sum: a thread
//                    takes the product of <= 8 values read at a stride, until <= 64 remain, which
//                    the host multiplies with f12_mul.
//   k_fexp_*         the final exponentiation of every lane's value, in place in the same workspace
//                    (final_exp_chain.h's program; further down), for bh_final_exponentiation_batch
//                    and the per-proof verdicts of bh_verify_each_device.
//
// State.  f is 12 Fp: it cannot stay in registers beside an Fp2 product's operands, and every
// output coefficient of a product reads several input coefficients, so f lives in a global
// workspace, packed (144 words) and double-buffered; T_k = (x_T, y_T) likewise (48 words per
// pair).  Both are word-major across lanes (word w of lane l at w * stride + l): a wave's loads
// are consecutive.  About 2 KB of traffic per lane and pair-step against tens of thousands of
// instructions.  Because all state is in memory the loop resumes at any bit: the host splits the
// 63 bits over launches of MILLER_BITS_PER_LAUNCH bits (below).
//
// Code size.  An Fp2 product is over a thousand instructions, so the Fp12 products are loops over
// the coefficient index (#pragma unroll 1) around ONE Fp2 product each, and the doubling and the
// addition step share one body (they differ in the numerator, the denominator and the x sum).
// The squaring of f is the dense product with both operands equal (36 Fp2 products instead of the
// 21 a dedicated squaring needs: 45 more Fp products against the > 1900 of a bit's 16 pair steps).
//
// Zero denominators.  For Q of order r no step divides by zero; a twist point of small order can
// (e.g. order 13: T = 12 Q = -Q at the second addition), and one zero would poison its lane's
// whole batch.  A zero denominator is replaced by one and raises a device flag; the host then
// returns BH_ERR_PAIRING_DEGENERATE and no value.
//
// Plain C++ over field.cuh's templates; its lazy bounds (products < 2p for inputs < 128p) are
// tracked in the comments next to each fe_sub<K>.
#include <string.h>

#include <algorithm>
#include <memory>

#include "f12_dev.cuh"
#include "final_exp_chain.h"
#include "group_host.h"
#include "pairing_dev.h"

using namespace bh;

namespace bh {

namespace {

constexpr int TW = 48;   // of a T record: x.c0, x.c1, y.c0, y.c1
constexpr int SW = 24;   // of a prefix product
constexpr uint64_t MILLER_X_ABS = 0xd201000000010000ull;

// ---------------------------------------------------------------- Fp12 products
// (ld_fp2, st_fp2, fp2_inv, fold_xi and f12_mul_dense: f12_dev.cuh)
// out = a * (l0 + l2 w^2 + yp w^3), yp in Fp: c_k = a_k l0 + a_(k-2) l2 + a_(k-3) yp with the
// same wrap.  Bounds: l0 < 3p, l2 <= 2p, yp < p and a's coefficients < p, every product < 2p;
// U sums <= 3 products (< 6p), W <= 2 (< 4p, so fe_sub<4>); folded < 6p + 4p + 4p = 14p (reduce).
__device__ void f12_mul_line(const uint32_t* a, uint32_t* out, size_t lane, size_t stride, const DFp2& l0,
                             const DFp2& l2, const DFp& yp) {
#pragma unroll 1
  for (int k = 0; k < 6; k++) {
    DFp2 U = F2::zero(), W = F2::zero();
#pragma unroll 1
    for (int t = 0; t < 2; t++) {  // l0 at shift 0, l2 at shift 2
      const bool wrap = 2 * t > k;
      const int j = wrap ? k - 2 * t + 6 : k - 2 * t;
      const DFp2 prod = F2::mul(ld_fp2(a, stride, lane, 24 * j), F2::select(t != 0, l2, l0));
      if (wrap) W = F2::add(W, prod);
      else U = F2::add(U, prod);
    }
    {
      const bool wrap = 3 > k;
      const int j = wrap ? k + 3 : k - 3;
      const DFp2 aj = ld_fp2(a, stride, lane, 24 * j);
      const DFp2 prod{fe_mul<FpCfg>(aj.c0, yp), fe_mul<FpCfg>(aj.c1, yp)};
      if (wrap) W = F2::add(W, prod);
      else U = F2::add(U, prod);
    }
    st_fp2(out, stride, lane, 24 * k, F2::reduce(fold_xi<4>(U, W)));
  }
}

// ---------------------------------------------------------------- kernels
struct MillerArgs {
  const uint32_t* g1;  // packed affine G1 records (24 words), pair i of the call at record i
  const uint32_t* g2;  // packed affine twist records (48 words)
  uint32_t* f;         // two Fp12 buffers of FW * stride words each
  uint32_t* T;         // K records of TW words per lane: word (k * TW + w) * stride + lane
  uint32_t* S;         // K prefix products of SW words per lane, the same layout
  uint32_t* mask;      // bit k: pair k of the lane has no identity
  uint32_t* flag;      // a zero denominator was met
  size_t n, lanes, stride;
  int K;
};

__global__ void __launch_bounds__(64) k_miller_init(MillerArgs A) {
  const size_t lane = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (lane >= A.lanes) return;
  const size_t i0 = lane * (size_t)A.K;
  const int cnt = (int)min((size_t)A.K, A.n - i0);
  uint32_t one[12];
  fe_pack<FpCfg>(fe_one<FpCfg>(), one);
  for (int w = 0; w < FW; w++) A.f[(size_t)w * A.stride + lane] = w < 12 ? one[w] : 0u;
  uint32_t m = 0;
  for (int k = 0; k < cnt; k++) {
    const uint32_t* p = A.g1 + (i0 + k) * 24;
    const uint32_t* q = A.g2 + (i0 + k) * 48;
    uint32_t nzp = 0, nzq = 0;
    for (int w = 0; w < 24; w++) nzp |= p[w];
    for (int w = 0; w < 48; w++) {
      const uint32_t v = q[w];
      nzq |= v;
      A.T[(size_t)(k * TW + w) * A.stride + lane] = v;
    }
    if (nzp && nzq) m |= 1u << k;  // the all-zero record is the identity
  }
  A.mask[lane] = m;
}

// The denominator of pair k's slope in a doubling (2 y_T) or addition (x_Q - x_T) step, < 2p; one
// for a pair with an identity, and for a zero denominator, which raises the flag (the prefix pass
// and the backward pass must see the same value, so both come here; the flag is idempotent).
__device__ __forceinline__ DFp2 step_denominator(const MillerArgs& A, size_t lane, int k, bool active, bool is_add,
                                                 const uint32_t* q) {
  if (!active) return F2::one();
  DFp2 d;
  if (is_add) {
    const DFp2 xt = ld_fp2(A.T, A.stride, lane, k * TW);
    d = F2::sub<1>(F2::unpack(q), xt);  // x_T is stored reduced (< p): < 2p
  } else {
    const DFp2 yt = ld_fp2(A.T, A.stride, lane, k * TW + 24);
    d = F2::add(yt, yt);
  }
  if (F2::is_zero(d)) {
    atomicOr(A.flag, 1u);
    return F2::one();
  }
  return d;
}

__global__ void __launch_bounds__(64) k_miller_steps(MillerArgs A, int bit_hi, int bit_lo) {
  const size_t lane = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (lane >= A.lanes) return;
  const size_t i0 = lane * (size_t)A.K;
  const int cnt = (int)min((size_t)A.K, A.n - i0);
  const uint32_t mask = A.mask[lane];
  const size_t fbuf = (size_t)FW * A.stride;
  int cur = 0;  // which buffer holds f (0 at every launch boundary)
#pragma unroll 1
  for (int bit = bit_hi; bit >= bit_lo; bit--) {
    f12_mul_dense(A.f + cur * fbuf, lane, A.f + cur * fbuf, lane, A.f + (cur ^ 1) * fbuf, lane, A.stride);
    cur ^= 1;
    const int nsub = 1 + (int)((MILLER_X_ABS >> bit) & 1);
#pragma unroll 1
    for (int sub = 0; sub < nsub; sub++) {  // the doubling step, then the addition step
      const bool is_add = sub != 0;
      // prefix products of the denominators: S[k] = d_0 ... d_(k-1)
      DFp2 acc = F2::one();
#pragma unroll 1
      for (int k = 0; k < cnt; k++) {
        const DFp2 d = step_denominator(A, lane, k, (mask >> k) & 1u, is_add, A.g2 + (i0 + k) * 48);
        st_fp2(A.S, A.stride, lane, k * SW, acc);
        acc = F2::mul(acc, d);
      }
      DFp2 inv = fp2_inv(acc);
#pragma unroll 1
      for (int k = cnt - 1; k >= 0; k--) {
        const bool active = (mask >> k) & 1u;
        const uint32_t* q = A.g2 + (i0 + k) * 48;
        const DFp2 d = step_denominator(A, lane, k, active, is_add, q);
        const DFp2 dinv = F2::mul(inv, ld_fp2(A.S, A.stride, lane, k * SW));  // 1 / d_k
        inv = F2::mul(inv, d);
        if (!active) continue;
        const DFp2 xt = ld_fp2(A.T, A.stride, lane, k * TW);
        const DFp2 yt = ld_fp2(A.T, A.stride, lane, k * TW + 24);
        DFp2 num, xsum;
        if (is_add) {
          const DFp2 xq = F2::unpack(q);
          num = F2::sub<1>(F2::unpack(q + 24), yt);  // y_Q - y_T, y_T < p: < 2p
          xsum = F2::add(xt, xq);                     // < 2p
        } else {
          const DFp2 x2 = F2::sqr(xt);
          num = F2::add(F2::add(x2, x2), x2);  // 3 x_T^2 < 6p
          xsum = F2::add(xt, xt);              // < 2p
        }
        const DFp2 lam = F2::mul(num, dinv);
        const uint32_t* p = A.g1 + (i0 + k) * 24;
        const DFp xp = fe_unpack<FpCfg>(p), yp = fe_unpack<FpCfg>(p + 12);
        const DFp2 l0 = F2::sub<1>(F2::mul(lam, xt), yt);  // lam x_T - y_T < 3p
        // -lam x_P: each product < 2p, so 2p - product, <= 2p
        const DFp2 l2{fe_neg<FpCfg, 2>(fe_mul<FpCfg>(lam.c0, xp)), fe_neg<FpCfg, 2>(fe_mul<FpCfg>(lam.c1, xp))};
        f12_mul_line(A.f + cur * fbuf, A.f + (cur ^ 1) * fbuf, lane, A.stride, l0, l2, yp);
        cur ^= 1;
        const DFp2 x3 = F2::sub<2>(F2::sqr(lam), xsum);                         // < 4p
        const DFp2 y3 = F2::sub<1>(F2::mul(lam, F2::sub<4>(xt, x3)), yt);  // x_T - x_3 < 5p; < 3p
        st_fp2(A.T, A.stride, lane, k * TW, F2::reduce(x3));
        st_fp2(A.T, A.stride, lane, k * TW + 24, F2::reduce(y3));
      }
    }
  }
  if (cur)  // the number of products differs between lanes (identities, a short last lane)
    for (int w = 0; w < FW; w++) A.f[(size_t)w * A.stride + lane] = A.f[fbuf + (size_t)w * A.stride + lane];
}

// One level of the product of m values: thread t < out leaves v[t] * v[t + out] * v[t + 2 out] ...
// (indices < m; out = ceil(m / 8), so at most 8 values) in v[t].  Nobody else reads v[t] (every
// other index a thread reads is >= out), so the level works in place; ping and pong hold the
// running product.
__global__ void __launch_bounds__(64) k_f12_product(uint32_t* v, uint32_t* ping, uint32_t* pong, size_t stride,
                                                    size_t m, size_t out) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= out) return;
  const uint32_t* a = v;
  int j = 1;
#pragma unroll 1
  for (size_t i = t + out; i < m; i += out, j++) {
    uint32_t* dst = (j & 1) ? ping : pong;
    f12_mul_dense(a, t, v, i, dst, t, stride);
    a = dst;
  }
  if (a != v)
    for (int w = 0; w < FW; w++) v[(size_t)w * stride + t] = a[(size_t)w * stride + t];
}

// ---------------------------------------------------------------- final exponentiation
// final_exp_chain.h's program, one lane per value, in place on FE_SLOTS Fp12 slots of the
// word-major workspace (word w of slot s of lane l at (s * FW + w) * stride + l).  Every slot
// holds fully reduced coefficients (< p): each step below stores through F2::reduce or
// neg_canonical, as f12_mul_dense and the Miller loop do.
struct FexpArgs {
  uint32_t* ws;
  const FeStep* prog;
  const uint32_t* consts;  // g1_0..5 (24 packed words each), then g2_0..5 (12 each), device Montgomery
  size_t n, stride;
};

__device__ __forceinline__ DFp fe_r2() {
  DFp r2;
#pragma unroll
  for (int k = 0; k < FpCfg::N; k++) r2.v[k] = FpCfg::R2[k];
  return r2;
}

__global__ void __launch_bounds__(64) k_fexp_steps(FexpArgs A, int lo, int hi) {
  const size_t lane = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (lane >= A.n) return;
  const size_t slot = (size_t)FW * A.stride;
#pragma unroll 1
  for (int s = lo; s < hi; s++) {
    const FeStep st = A.prog[s];
    uint32_t* dst = A.ws + st.dst * slot;
    const uint32_t* a = A.ws + st.a * slot;
    const uint32_t* b = A.ws + st.b * slot;
    if (st.op == FE_MUL) {
      f12_mul_dense(a, lane, b, lane, dst, lane, A.stride);
    } else if (st.op == FE_CONJ) {
#pragma unroll 1
      for (int k = 0; k < 6; k++) {
        const DFp2 c = ld_fp2(a, A.stride, lane, 24 * k);  // < p
        st_fp2(dst, A.stride, lane, 24 * k, (k & 1) ? F2::neg_canonical(c) : c);
      }
    } else if (st.op == FE_FROB) {
#pragma unroll 1
      for (int k = 0; k < 6; k++) {
        DFp2 c = ld_fp2(a, A.stride, lane, 24 * k);
        c.c1 = fe_neg<FpCfg, 1>(c.c1);  // c1 < p: p - c1 <= p
        st_fp2(dst, A.stride, lane, 24 * k, F2::reduce(F2::mul(c, F2::unpack(A.consts + 24 * k))));  // < 2p
      }
    } else if (st.op == FE_FROB2) {
#pragma unroll 1
      for (int k = 0; k < 6; k++) {
        const DFp2 c = ld_fp2(a, A.stride, lane, 24 * k);
        const DFp g = fe_unpack<FpCfg>(A.consts + 144 + 12 * k);
        st_fp2(dst, A.stride, lane, 24 * k, F2::reduce(DFp2{fe_mul<FpCfg>(c.c0, g), fe_mul<FpCfg>(c.c1, g)}));
      }
    } else if (st.op == FE_SCALE_INV) {
      const DFp2 inv = fp2_inv(ld_fp2(b, A.stride, lane, 0));  // its argument < p; both halves < 2p
#pragma unroll 1
      for (int k = 0; k < 6; k++)
        st_fp2(dst, A.stride, lane, 24 * k, F2::reduce(F2::mul(ld_fp2(a, A.stride, lane, 24 * k), inv)));
    } else {
      for (int w = 0; w < FW; w++) dst[(size_t)w * A.stride + lane] = a[(size_t)w * A.stride + lane];
    }
  }
}

// slot 0 of every lane times the value at index 0 of slot 2, through slot 1
__global__ void __launch_bounds__(64) k_fexp_scale(uint32_t* ws, size_t n, size_t stride) {
  const size_t lane = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (lane >= n) return;
  const size_t slot = (size_t)FW * stride;
  f12_mul_dense(ws, lane, ws + 2 * slot, 0, ws + slot, lane, stride);
  for (int w = 0; w < FW; w++) ws[(size_t)w * stride + lane] = ws[slot + (size_t)w * stride + lane];
}

// n values of 576 bytes (twelve 48-byte big-endian canonical coefficients) -> slot 0
__global__ void __launch_bounds__(64) k_fexp_load(const uint32_t* in, uint32_t* ws, size_t n, size_t stride) {
  const size_t lane = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (lane >= n) return;
#pragma unroll 1
  for (int j = 0; j < 12; j++) {
    uint32_t w[12];
#pragma unroll
    for (int i = 0; i < 12; i++) w[i] = __builtin_bswap32(in[lane * FW + 12 * j + 11 - i]);
    const DFp x = fe_reduce_full<FpCfg>(fe_mul<FpCfg>(fe_unpack<FpCfg>(w), fe_r2()));
    fe_pack<FpCfg>(x, w);
#pragma unroll
    for (int i = 0; i < 12; i++) ws[(size_t)(12 * j + i) * stride + lane] = w[i];
  }
}

// slot 0 -> the same byte form
__global__ void __launch_bounds__(64) k_fexp_store(const uint32_t* ws, uint32_t* out, size_t n, size_t stride) {
  const size_t lane = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (lane >= n) return;
#pragma unroll 1
  for (int j = 0; j < 12; j++) {
    uint32_t w[12];
#pragma unroll
    for (int i = 0; i < 12; i++) w[i] = ws[(size_t)(12 * j + i) * stride + lane];
    // out of Montgomery form: <= p, one conditional subtraction
    const DFp x = fe_csub<FpCfg, 1>(fe_from_mont<FpCfg>(fe_unpack<FpCfg>(w)));
    fe_pack<FpCfg>(x, w);
#pragma unroll
    for (int i = 0; i < 12; i++) out[lane * FW + 12 * j + 11 - i] = __builtin_bswap32(w[i]);
  }
}

// one for every value equal to one, else zero
__global__ void __launch_bounds__(64) k_fexp_is_one(const uint32_t* ws, uint32_t* out, size_t n, size_t stride) {
  const size_t lane = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (lane >= n) return;
  uint32_t one[12], diff = 0;
  fe_pack<FpCfg>(fe_one<FpCfg>(), one);
  for (int w = 0; w < FW; w++) diff |= ws[(size_t)w * stride + lane] ^ (w < 12 ? one[w] : 0u);
  out[lane] = diff == 0;
}

inline unsigned nb64(size_t n) { return (unsigned)((n + 63) / 64); }

// Bits per launch.  All state is in memory, so the split costs one launch each.  At 2^20 pairs a
// bit is 2^20 x (1 or 2) pair steps of about 120 Fp products plus the lanes' inversions: the whole
// loop is estimated at a few hundred ms, so 8 launches keep every dispatch well below the
// library's longest (k_varbase_mul_win<G2>, 147 ms per 2^20); DESIGN.md section 11 has the
// measured figure.
constexpr int MILLER_BITS_PER_LAUNCH = 8;

}  // namespace

Fp12 f12_from_dev_words(const uint32_t* w) {
  Fp12 r;
  for (int i = 0; i < 6; i++) r.c[i] = Fp2{fp_from_dev_words(w + 24 * i), fp_from_dev_words(w + 24 * i + 12)};
  return r;
}

namespace {

// Pairs per lane.  A lane's step costs one inversion (460 Fp products) plus about 120 per pair, so
// a larger K does less work per pair, but only lanes run in parallel: while the lanes of K = 1
// would not fill the device (the waves the step kernel can keep resident), a larger K only makes
// every lane's serial chain longer.  So K is the smallest value whose lanes fit the resident
// waves once, capped at MILLER_MAX_K: 1 up to that many pairs, 16 from 16 times as many.
int choose_k(bh_ctx* ctx, size_t n) {
  hipDeviceProp_t prop;
  int blocks = 1;
  if (hipGetDeviceProperties(&prop, ctx->device) != hipSuccess) return MILLER_MAX_K;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&blocks, (const void*)k_miller_steps, 64, 0) != hipSuccess ||
      blocks < 1)
    blocks = 1;
  const size_t resident = (size_t)std::max(prop.multiProcessorCount, 1) * (size_t)blocks * 64;
  return (int)std::min<size_t>(MILLER_MAX_K, std::max<size_t>(1, (n + resident - 1) / resident));
}

}  // namespace

// (MillerWork and the contract: pairing_dev.h)
bh_status miller_lanes(bh_ctx* ctx, const uint32_t* g1, const uint32_t* g2, size_t n, int K, int fslots,
                       MillerWork* w) {
  MillerArgs A;
  A.g1 = g1;
  A.g2 = g2;
  A.n = n;
  A.K = K;
  A.lanes = (n + K - 1) / K;
  A.stride = (A.lanes + 63) / 64 * 64;
  w->lanes = A.lanes;
  w->stride = A.stride;
  BH_TRY_HIP(w->f.alloc((size_t)fslots * FW * A.stride * 4));
  BH_TRY_HIP(w->T.alloc((size_t)K * TW * A.stride * 4));
  BH_TRY_HIP(w->S.alloc((size_t)K * SW * A.stride * 4));
  BH_TRY_HIP(w->mask.alloc(A.stride * 4));
  BH_TRY_HIP(w->flag.alloc(4));
  A.f = w->f.as<uint32_t>();
  A.T = w->T.as<uint32_t>();
  A.S = w->S.as<uint32_t>();
  A.mask = w->mask.as<uint32_t>();
  A.flag = w->flag.as<uint32_t>();
  BH_TRY_HIP(hipMemsetAsync(w->flag.p, 0, 4, ctx->stream));
  hipLaunchKernelGGL(k_miller_init, dim3(nb64(A.lanes)), dim3(64), 0, ctx->stream, A);
  BH_TRY_HIP(hipGetLastError());
  for (int hi = 62; hi >= 0; hi -= MILLER_BITS_PER_LAUNCH) {
    hipLaunchKernelGGL(k_miller_steps, dim3(nb64(A.lanes)), dim3(64), 0, ctx->stream, A, hi,
                       std::max(hi - MILLER_BITS_PER_LAUNCH + 1, 0));
    BH_TRY_HIP(hipGetLastError());
  }
  uint32_t hflag = 0;
  BH_TRY_HIP(hipMemcpyAsync(&hflag, w->flag.p, 4, hipMemcpyDeviceToHost, ctx->stream));
  BH_TRY_HIP(hipStreamSynchronize(ctx->stream));
  return hflag ? BH_ERR_PAIRING_DEGENERATE : BH_OK;
}

bh_status f12_lanes_product(bh_ctx* ctx, uint32_t* f, uint32_t* ping, uint32_t* pong, size_t stride, size_t m,
                            Fp12* out) {
  while (m > 64) {
    const size_t o = (m + 7) / 8;
    hipLaunchKernelGGL(k_f12_product, dim3(nb64(o)), dim3(64), 0, ctx->stream, f, ping, pong, stride, m, o);
    BH_TRY_HIP(hipGetLastError());
    m = o;
  }
  std::vector<uint32_t> rows((size_t)FW * m), wd(FW);
  BH_TRY_HIP(hipMemcpy2DAsync(rows.data(), m * 4, f, stride * 4, m * 4, FW, hipMemcpyDeviceToHost, ctx->stream));
  BH_TRY_HIP(hipStreamSynchronize(ctx->stream));  // the workspace is freed on return
  Fp12 r = f12_one();
  for (size_t t = 0; t < m; t++) {
    for (int k = 0; k < FW; k++) wd[k] = rows[(size_t)k * m + t];
    r = f12_mul(r, f12_from_dev_words(wd.data()));
  }
  *out = r;
  return BH_OK;
}

namespace {

bh_status miller_chunk(bh_ctx* ctx, const uint32_t* g1, const uint32_t* g2, size_t n, int K, Fp12* out) {
  MillerWork w;
  bh_status s = miller_lanes(ctx, g1, g2, n, K, 2, &w);
  if (s) return s;
  uint32_t* f = w.f.as<uint32_t>();
  DevBuf pong;
  BH_TRY_HIP(pong.alloc((size_t)FW * w.stride * 4));
  return f12_lanes_product(ctx, f, f + (size_t)FW * w.stride, pong.as<uint32_t>(), w.stride, w.lanes, out);
}

void f12_to_bytes(const Fp12& f, uint8_t out[576]) {
  for (int i = 0; i < 6; i++) {
    fp_to_be(f.c[i].c0, out + 96 * i);
    fp_to_be(f.c[i].c1, out + 96 * i + 48);
  }
}

}  // namespace

// host Montgomery (R = 2^384) -> the device's packed words (the canonical value of c * 2^406)
void fp_to_dev_words(const Fp& x, uint32_t* w) {
  static const Fp K = [] {
    uint64_t two[6] = {2, 0, 0, 0, 0, 0}, e[1] = {406}, raw[6];
    to_int(pow_vartime(from_int<6>(two), e, 1), raw);  // canonical 2^406 mod p
    Fp out;
    memcpy(out.v, raw, sizeof raw);
    return out;
  }();
  const Fp t = mul(x, K);  // (c 2^384) (2^406) / 2^384 = c 2^406 mod p, the words themselves
  memcpy(w, t.v, 48);
}

// Steps per launch, in units of one dense Fp12 product (36 Fp2 products, about 108 Fp products' worth of
// work; the inversion step's Fermat ladder counts as four, the coefficient-wise steps as nothing).
// All state is in memory, so a split costs one launch: 49 launches for the chain.  Measured at 2^14
// lanes: 1.06 ms per launch; at MILLER_CHUNK lanes, 64 times as many, a launch stays under the
// library's longest dispatch (k_varbase_mul_win<G2>, 147 ms per 2^20) even if it scaled with the
// lane count from there.
constexpr int FEXP_PRODUCTS_PER_LAUNCH = 8;

// (FexpTables and the contract of the two functions: pairing_dev.h)
bh_status fexp_tables(bh_ctx* ctx, FexpTables* t) {
  const std::vector<FeStep>& p = fe_program();
  const FeConsts& C = fe_consts();
  uint32_t cw[6 * 24 + 6 * 12];
  for (int k = 0; k < 6; k++) {
    fp_to_dev_words(C.g1[k].c0, cw + 24 * k);
    fp_to_dev_words(C.g1[k].c1, cw + 24 * k + 12);
    fp_to_dev_words(C.g2[k], cw + 144 + 12 * k);
  }
  BH_TRY_HIP(t->prog.alloc(p.size() * sizeof(FeStep)));
  BH_TRY_HIP(t->consts.alloc(sizeof cw));
  BH_TRY_HIP(hipMemcpyAsync(t->prog.p, p.data(), p.size() * sizeof(FeStep), hipMemcpyHostToDevice, ctx->stream));
  BH_TRY_HIP(hipMemcpyAsync(t->consts.p, cw, sizeof cw, hipMemcpyHostToDevice, ctx->stream));
  BH_TRY_HIP(hipStreamSynchronize(ctx->stream));  // both sources are about to go away
  int lo = 0, weight = 0;
  for (int s = 0; s < (int)p.size(); s++) {
    weight += p[s].op == FE_MUL ? 1 : p[s].op == FE_SCALE_INV ? 4 : 0;
    if (weight >= FEXP_PRODUCTS_PER_LAUNCH || s + 1 == (int)p.size()) {
      t->launches.push_back({lo, s + 1});
      lo = s + 1;
      weight = 0;
    }
  }
  return BH_OK;
}

bh_status fexp_enqueue(bh_ctx* ctx, const FexpTables& t, uint32_t* ws, size_t n, size_t stride) {
  FexpArgs A;
  A.ws = ws;
  A.prog = t.prog.as<FeStep>();
  A.consts = t.consts.as<uint32_t>();
  A.n = n;
  A.stride = stride;
  for (const auto& l : t.launches) {
    hipLaunchKernelGGL(k_fexp_steps, dim3(nb64(n)), dim3(64), 0, ctx->stream, A, l.first, l.second);
    BH_TRY_HIP(hipGetLastError());
  }
  return BH_OK;
}

namespace {

// a coefficient >= p among the 12 n big-endian 48-byte values
bool f12_bytes_canonical(const uint8_t* f, size_t n) {
  uint8_t pb[48];
  for (int i = 0; i < 48; i++) pb[i] = (uint8_t)(hostc::FP_P[5 - i / 8] >> (8 * (7 - i % 8)));
  for (size_t i = 0; i < 12 * n; i++)
    if (memcmp(f + 48 * i, pb, 48) >= 0) return false;
  return true;
}

bh_status final_exponentiation_batch(bh_ctx* ctx, const uint8_t* f, size_t n, uint8_t* out) {
  if (!f12_bytes_canonical(f, n)) return BH_ERR_INVALID_ENCODING;
  FexpTables t;
  bh_status s = fexp_tables(ctx, &t);
  if (s) return s;
  const size_t chunk = std::min(n, MILLER_CHUNK), stride = (chunk + 63) / 64 * 64;
  DevBuf io, ws;
  BH_TRY_HIP(io.alloc(chunk * 576));
  BH_TRY_HIP(ws.alloc((size_t)FE_SLOTS * FW * stride * 4));
  for (size_t base = 0; base < n; base += chunk) {
    const size_t m = std::min(chunk, n - base);
    BH_TRY_HIP(hipMemcpyAsync(io.p, f + 576 * base, 576 * m, hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(k_fexp_load, dim3(nb64(m)), dim3(64), 0, ctx->stream, io.as<uint32_t>(), ws.as<uint32_t>(), m,
                       stride);
    BH_TRY_HIP(hipGetLastError());
    if ((s = fexp_enqueue(ctx, t, ws.as<uint32_t>(), m, stride))) return s;
    hipLaunchKernelGGL(k_fexp_store, dim3(nb64(m)), dim3(64), 0, ctx->stream, ws.as<uint32_t>(), io.as<uint32_t>(), m,
                       stride);
    BH_TRY_HIP(hipGetLastError());
    BH_TRY_HIP(hipMemcpyAsync(out + 576 * base, io.p, 576 * m, hipMemcpyDeviceToHost, ctx->stream));
    BH_TRY_HIP(hipStreamSynchronize(ctx->stream));
  }
  return BH_OK;
}

bh_status miller_product_abi(bh_ctx* ctx, const bh_srs* g1, size_t off1, const bh_srs* g2, size_t off2, size_t n, int K,
                             uint8_t* out) {
  if (!ctx || !g1 || !g2 || !out || !g1->ctx || !g2->ctx || g1->ctx->device != ctx->device ||
      g2->ctx->device != ctx->device)
    return BH_ERR_INVALID_ARGUMENT;
  if (g1->group != BH_G1 || g2->group != BH_G2) return BH_ERR_INVALID_ARGUMENT;
  if (off1 > g1->n || n > g1->n - off1 || off2 > g2->n || n > g2->n - off2) return BH_ERR_INVALID_ARGUMENT;
  std::lock_guard<std::mutex> lk(ctx->mu);
  BH_TRY_HIP(hipSetDevice(ctx->device));
  bh_status s = scratch_check(ctx);
  if (s) return s;
  Fp12 f;
  if ((s = miller_product_device(ctx, g1, off1, g2, off2, n, K, &f))) return s;
  f12_to_bytes(f, out);
  return BH_OK;
}

}  // namespace

void pairing_kernels(std::vector<KernInfo>& v) {
  v.push_back({"k_miller_init", (const void*)k_miller_init, 64, 0});
  v.push_back({"k_miller_steps", (const void*)k_miller_steps, 64, 0});
  v.push_back({"k_f12_product", (const void*)k_f12_product, 64, 0});
  v.push_back({"k_fexp_steps", (const void*)k_fexp_steps, 64, 0});
  v.push_back({"k_fexp_scale", (const void*)k_fexp_scale, 64, 0});
  v.push_back({"k_fexp_load", (const void*)k_fexp_load, 64, 0});
  v.push_back({"k_fexp_store", (const void*)k_fexp_store, 64, 0});
  v.push_back({"k_fexp_is_one", (const void*)k_fexp_is_one, 64, 0});
}

bh_status pairing_each_is_one(bh_ctx* ctx, const uint32_t* g1, const uint32_t* g2, size_t lanes, int K,
                              const Fp12& scale, uint32_t* verdict) {
  if (K < 1 || K > MILLER_MAX_K) return BH_ERR_INVALID_ARGUMENT;
  if (!lanes) return BH_OK;
  FexpTables t;
  bh_status s = fexp_tables(ctx, &t);
  if (s) return s;
  uint32_t sw[FW];
  for (int i = 0; i < 6; i++) {
    fp_to_dev_words(scale.c[i].c0, sw + 24 * i);
    fp_to_dev_words(scale.c[i].c1, sw + 24 * i + 12);
  }
  DevBuf ok;
  BH_TRY_HIP(ok.alloc(std::min(lanes, MILLER_CHUNK) * 4));
  for (size_t base = 0; base < lanes; base += MILLER_CHUNK) {
    const size_t m = std::min(MILLER_CHUNK, lanes - base);
    MillerWork w;
    if ((s = miller_lanes(ctx, g1 + base * K * 24, g2 + base * K * 48, m * K, K, FE_SLOTS, &w))) return s;
    uint32_t* ws = w.f.as<uint32_t>();
    // the constant at index 0 of slot 2, which the chain overwrites only later
    BH_TRY_HIP(hipMemcpy2DAsync(ws + 2 * (size_t)FW * w.stride, w.stride * 4, sw, 4, 4, FW, hipMemcpyHostToDevice,
                                ctx->stream));
    hipLaunchKernelGGL(k_fexp_scale, dim3(nb64(m)), dim3(64), 0, ctx->stream, ws, m, w.stride);
    BH_TRY_HIP(hipGetLastError());
    if ((s = fexp_enqueue(ctx, t, ws, m, w.stride))) return s;
    hipLaunchKernelGGL(k_fexp_is_one, dim3(nb64(m)), dim3(64), 0, ctx->stream, ws, ok.as<uint32_t>(), m, w.stride);
    BH_TRY_HIP(hipGetLastError());
    BH_TRY_HIP(hipMemcpyAsync(verdict + base, ok.p, m * 4, hipMemcpyDeviceToHost, ctx->stream));
    BH_TRY_HIP(hipStreamSynchronize(ctx->stream));  // the workspace is freed at the end of the pass
  }
  return BH_OK;
}

bh_status miller_product_device(bh_ctx* ctx, const bh_srs* g1, size_t off1, const bh_srs* g2, size_t off2, size_t n,
                                int K, Fp12* out) {
  if (K < 0 || K > MILLER_MAX_K) return BH_ERR_INVALID_ARGUMENT;
  Fp12 r = f12_one();
  for (size_t base = 0; base < n; base += MILLER_CHUNK) {
    const size_t k = std::min(MILLER_CHUNK, n - base);
    Fp12 part;
    bh_status s = miller_chunk(ctx, g1->pts.as<uint32_t>() + (off1 + base) * 24,
                               g2->pts.as<uint32_t>() + (off2 + base) * 48, k, K ? K : choose_k(ctx, k), &part);
    if (s) return s;
    r = f12_mul(r, part);
  }
  *out = r;
  return BH_OK;
}

}  // namespace bh

extern "C" {

bh_status bh_miller_product(bh_ctx* ctx, const bh_srs* g1, size_t off1, const bh_srs* g2, size_t off2, size_t n,
                            uint8_t out[576]) {
  return miller_product_abi(ctx, g1, off1, g2, off2, n, 0, out);
}

bh_status bh_selftest_miller_product(bh_ctx* ctx, const bh_srs* g1, size_t off1, const bh_srs* g2, size_t off2,
                                     size_t n, int K, uint8_t out[576]) {
  if (K < 1) return BH_ERR_INVALID_ARGUMENT;
  return miller_product_abi(ctx, g1, off1, g2, off2, n, K, out);
}

bh_status bh_final_exponentiation(const uint8_t f[576], uint8_t out[576]) {
  if (!f || !out) return BH_ERR_INVALID_ARGUMENT;
  Fp12 a;
  for (int i = 0; i < 6; i++)
    if (!fp_from_be(f + 96 * i, &a.c[i].c0) || !fp_from_be(f + 96 * i + 48, &a.c[i].c1))
      return BH_ERR_INVALID_ENCODING;  // a coefficient >= p
  f12_to_bytes(final_exponentiation(a), out);
  return BH_OK;
}

bh_status bh_selftest_final_exponentiation_chain(const uint8_t f[576], uint8_t out[576]) {
  if (!f || !out) return BH_ERR_INVALID_ARGUMENT;
  Fp12 a;
  for (int i = 0; i < 6; i++)
    if (!fp_from_be(f + 96 * i, &a.c[i].c0) || !fp_from_be(f + 96 * i + 48, &a.c[i].c1))
      return BH_ERR_INVALID_ENCODING;
  f12_to_bytes(fe_chain_host(a), out);
  return BH_OK;
}

bh_status bh_final_exponentiation_batch(bh_ctx* ctx, const uint8_t* f, size_t n, uint8_t* out) {
  if (!ctx || (n && (!f || !out))) return BH_ERR_INVALID_ARGUMENT;
  if (!n) return BH_OK;
  std::lock_guard<std::mutex> lk(ctx->mu);
  BH_TRY_HIP(hipSetDevice(ctx->device));
  bh_status s = scratch_check(ctx);
  if (s) return s;
  return final_exponentiation_batch(ctx, f, n, out);
}

}  // extern "C"
