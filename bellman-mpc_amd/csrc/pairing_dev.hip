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

#include "group_host.h"
#include "pairing_dev.h"

using namespace bh;

namespace bh {

namespace {

using F2 = Fp2Ops;
constexpr int FW = 144;  // packed words of an Fp12 value: c[0].c0, c[0].c1, ..., c[5].c1, 12 each
constexpr int TW = 48;   // of a T record: x.c0, x.c1, y.c0, y.c1
constexpr int SW = 24;   // of a prefix product
constexpr uint64_t MILLER_X_ABS = 0xd201000000010000ull;

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
  o.c1 = fe_mul<FpCfg>(fe_neg<FpCfg, 2>(x.c1), r);  // x.c1 < 2p at the one call site
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

inline unsigned nb64(size_t n) { return (unsigned)((n + 63) / 64); }

// Bits per launch.  All state is in memory, so the split costs one launch each.  At 2^20 pairs a
// bit is 2^20 x (1 or 2) pair steps of about 120 Fp products plus the lanes' inversions: the whole
// loop is estimated at a few hundred ms, so 8 launches keep every dispatch well below the
// library's longest (k_varbase_mul_win<G2>, 147 ms per 2^20); DESIGN.md section 11 has the
// measured figure.
constexpr int MILLER_BITS_PER_LAUNCH = 8;
// pairs per call of the loop (the workspace: 752 B per pair at K = 16, plus 1.7 KB per lane)
constexpr size_t MILLER_CHUNK = (size_t)1 << 20;

Fp12 f12_from_dev_words(const uint32_t* w) {
  Fp12 r;
  for (int i = 0; i < 6; i++) r.c[i] = Fp2{fp_from_dev_words(w + 24 * i), fp_from_dev_words(w + 24 * i + 12)};
  return r;
}

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

bh_status miller_chunk(bh_ctx* ctx, const uint32_t* g1, const uint32_t* g2, size_t n, int K, Fp12* out) {
  MillerArgs A;
  A.g1 = g1;
  A.g2 = g2;
  A.n = n;
  A.K = K;
  A.lanes = (n + K - 1) / K;
  A.stride = (A.lanes + 63) / 64 * 64;
  DevBuf f, pong, T, S, mask, flag;
  BH_TRY_HIP(f.alloc(2 * (size_t)FW * A.stride * 4));
  BH_TRY_HIP(pong.alloc((size_t)FW * A.stride * 4));
  BH_TRY_HIP(T.alloc((size_t)K * TW * A.stride * 4));
  BH_TRY_HIP(S.alloc((size_t)K * SW * A.stride * 4));
  BH_TRY_HIP(mask.alloc(A.stride * 4));
  BH_TRY_HIP(flag.alloc(4));
  A.f = f.as<uint32_t>();
  A.T = T.as<uint32_t>();
  A.S = S.as<uint32_t>();
  A.mask = mask.as<uint32_t>();
  A.flag = flag.as<uint32_t>();
  BH_TRY_HIP(hipMemsetAsync(flag.p, 0, 4, ctx->stream));
  hipLaunchKernelGGL(k_miller_init, dim3(nb64(A.lanes)), dim3(64), 0, ctx->stream, A);
  BH_TRY_HIP(hipGetLastError());
  for (int hi = 62; hi >= 0; hi -= MILLER_BITS_PER_LAUNCH) {
    hipLaunchKernelGGL(k_miller_steps, dim3(nb64(A.lanes)), dim3(64), 0, ctx->stream, A, hi,
                       std::max(hi - MILLER_BITS_PER_LAUNCH + 1, 0));
    BH_TRY_HIP(hipGetLastError());
  }
  uint32_t hflag = 0;
  BH_TRY_HIP(hipMemcpyAsync(&hflag, flag.p, 4, hipMemcpyDeviceToHost, ctx->stream));
  BH_TRY_HIP(hipStreamSynchronize(ctx->stream));
  if (hflag) return BH_ERR_PAIRING_DEGENERATE;
  size_t m = A.lanes;
  while (m > 64) {
    const size_t o = (m + 7) / 8;
    hipLaunchKernelGGL(k_f12_product, dim3(nb64(o)), dim3(64), 0, ctx->stream, A.f, A.f + (size_t)FW * A.stride,
                       pong.as<uint32_t>(), A.stride, m, o);
    BH_TRY_HIP(hipGetLastError());
    m = o;
  }
  std::vector<uint32_t> rows((size_t)FW * m), w(FW);
  BH_TRY_HIP(hipMemcpy2DAsync(rows.data(), m * 4, A.f, A.stride * 4, m * 4, FW, hipMemcpyDeviceToHost, ctx->stream));
  BH_TRY_HIP(hipStreamSynchronize(ctx->stream));  // the workspace is freed on return
  Fp12 r = f12_one();
  for (size_t t = 0; t < m; t++) {
    for (int k = 0; k < FW; k++) w[k] = rows[(size_t)k * m + t];
    r = f12_mul(r, f12_from_dev_words(w.data()));
  }
  *out = r;
  return BH_OK;
}

void f12_to_bytes(const Fp12& f, uint8_t out[576]) {
  for (int i = 0; i < 6; i++) {
    fp_to_be(f.c[i].c0, out + 96 * i);
    fp_to_be(f.c[i].c1, out + 96 * i + 48);
  }
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

}  // extern "C"
