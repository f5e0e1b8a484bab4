// Per-element variable-base scalar multiplication: out[i] = k_i * P_i for a device vector of
// distinct, unknown points -- the player's side of a ceremony round (make_new_tau_paramter,
// reference groth16/mpc.rs:677-706, and the z_i * O_i of the batched verification), which neither
// k_fixed_base (one known base, host-built table) nor the MSM (which sums) can do.
//
//   k_varbase_multiples + k_varbase_mul_win
//                   one lane per point, a fixed signed window (w = 4) over a per-chunk table of
//                   1P .. 8P in a global workspace: 4 doublings and one madd per window.  The
//                   scalar lives in eight registers shifted left one window per step (no
//                   indexed private array); every lane of a wave runs the same W steps, a zero
//                   digit skips its one addition.  Scalar stride 8 words (per element) or 0 (one
//                   scalar for the vector: every branch is then wave-uniform).  The plain
//                   double-and-add it was developed from measured 0.80x (G1) / 0.55x (G2) of its
//                   points/s at 2^20 and was removed (profiles/mpc_ab_varbase_window_2p20.txt).
//   k_varbase_sub   out[i] = A[lo2 + i] - A[lo1 + i] (matrixed_h, mpc.rs:631-635)
//   k_varbase_powers a * x^i as canonical scalars, from split power tables like k_r1cs_powers
// A result that is the identity (a zero scalar, equal points) raises a device flag that the host
// reads before k_normalize runs: a zero ZZ would poison a whole inversion chunk.
#include <string.h>

#include <algorithm>
#include <memory>

#include "crs.h"
#include "ntt_common.cuh"
#include "r1cs.h"
#include "varbase.h"

using namespace bh;

namespace bh {

template <class C>
struct VbField;
template <>
struct VbField<G1Ops> { using F = G1F; };
template <>
struct VbField<G2Ops> { using F = Fp2Ops; };

template <class C>
__device__ __forceinline__ typename C::A vb_load_affine(const uint32_t* base, size_t i) {
  using F = typename FieldOf<C>::F;
  constexpr int PW = F::PACKED_WORDS;
  typename C::A a;
  a.x = F::unpack(base + i * 2 * PW);
  a.y = F::unpack(base + i * 2 * PW + PW);
  return a;
}

// k_varbase_multiples writes 1P .. 8P of every point of a chunk as XYZZ, digit-major (record
// d * n + i: the lanes of a wave read consecutive records),
// which k_normalize turns into an affine table like window_table does; k_varbase_mul_win then runs
// 4 doublings and one madd per window.  Signed digits without a carry chain: with the bias
// B = 0x88..8 added to the scalar once, digit_j = nibble_j(k + B) - 8 in [-8, 7].  All W nibbles are
// biased when top_biased (k < r keeps k + B below 2^256 for W = 64); otherwise the top window is
// left unbiased and W is chosen so that it only holds the carry (0 or 1).
template <class C>
__global__ void __launch_bounds__(256) k_varbase_multiples(const uint32_t* pts, size_t n, typename C::P* out) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const typename C::A a = vb_load_affine<C>(pts, i);
  typename C::P acc = C::from_affine(a);
  out[i] = acc;
  acc = C::dbl_affine(a);
  out[n + i] = acc;
  for (int d = 2; d < 8; d++) {
    acc = C::madd(acc, a);
    out[(size_t)d * n + i] = acc;
  }
}

template <class C>
__global__ void __launch_bounds__(256) k_varbase_mul_win(const uint32_t* table, const uint32_t* scalars, int stride,
                                                         size_t n, int W, int top_biased, typename C::P* out,
                                                         uint32_t* flag) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint4* sp = reinterpret_cast<const uint4*>(scalars + i * (size_t)stride);
  const uint4 s0 = sp[0], s1 = sp[1];
  uint32_t s[8] = {s0.x, s0.y, s0.z, s0.w, s1.x, s1.y, s1.z, s1.w};
  const int nbias = top_biased ? W : W - 1;  // biased nibbles, from the bottom
  uint64_t carry = 0;
#pragma unroll
  for (int w = 0; w < 8; w++) {
    const int cnt = min(max(nbias - 8 * w, 0), 8);
    const uint32_t bw = cnt == 8 ? 0x88888888u : (0x88888888u & ((1u << (4 * cnt)) - 1u));
    const uint64_t t = (uint64_t)s[w] + bw + carry;
    s[w] = (uint32_t)t;
    carry = t >> 32;
  }
  // window W - 1 to the top nibble of s[7]
  const int lead = 256 - 4 * W;
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
  typename C::P acc = C::identity();
  for (int j = 0; j < W; j++) {
    if (j) {
#pragma unroll 1
      for (int t = 0; t < 4; t++) acc = C::dbl(acc);
    }
    const int d = (int)(s[7] >> 28) - ((j || top_biased) ? 8 : 0);
    if (d) {
      const int m = min(d < 0 ? -d : d, 8) - 1;  // (an unbiased top digit is 0 or 1)
      typename C::A t = vb_load_affine<C>(table, (size_t)m * n + i);
      if (d < 0) t = C::neg_affine(t);
      acc = C::madd(acc, t);
    }
#pragma unroll
    for (int w = 7; w > 0; w--) s[w] = (s[w] << 4) | (s[w - 1] >> 28);
    s[0] <<= 4;
  }
  if (C::is_identity(acc)) atomicOr(flag, 1u);
  out[i] = acc;
}

template <class C>
__global__ void __launch_bounds__(256) k_varbase_sub(const uint32_t* pts, size_t lo1, size_t lo2, size_t n,
                                                     typename C::P* out, uint32_t* flag) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const typename C::P acc =
      C::madd(C::from_affine(vb_load_affine<C>(pts, lo2 + i)), C::neg_affine(vb_load_affine<C>(pts, lo1 + i)));
  if (C::is_identity(acc)) atomicOr(flag, 1u);
  out[i] = acc;
}

// out[i] = factor(i) = lo[i & mask] * hi[i >> lo_bits] as a canonical scalar (hi carries a)
__global__ void __launch_bounds__(256) k_varbase_powers(uint32_t* out, uint32_t n, const uint32_t* lo,
                                                        const uint32_t* hi, int lo_bits) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  st_packed(out, i, fe_csub<FrCfg, 1>(fe_from_mont<FrCfg>(pow_factor(lo, hi, lo_bits, i))));
}

void varbase_kernels(std::vector<KernInfo>& v) {
  v.push_back({"k_varbase_multiples<G1>", (const void*)k_varbase_multiples<G1Ops>, 256, 0});
  v.push_back({"k_varbase_multiples<G2>", (const void*)k_varbase_multiples<G2Ops>, 256, 0});
  v.push_back({"k_varbase_mul_win<G1>", (const void*)k_varbase_mul_win<G1Ops>, 256, 0});
  v.push_back({"k_varbase_mul_win<G2>", (const void*)k_varbase_mul_win<G2Ops>, 256, 0});
  v.push_back({"k_varbase_sub<G1>", (const void*)k_varbase_sub<G1Ops>, 256, 0});
  v.push_back({"k_varbase_sub<G2>", (const void*)k_varbase_sub<G2Ops>, 256, 0});
  v.push_back({"k_varbase_powers", (const void*)k_varbase_powers, 256, 0});
}

namespace {

inline unsigned nb(size_t n, unsigned bs) { return (unsigned)((n + bs - 1) / bs); }

constexpr size_t VB_CHUNK = (size_t)1 << 21;  // points per launch (the XYZZ scratch: 448 B each in G2)

void srs_init(bh_ctx* ctx, int group, size_t n, bh_srs* out) {
  out->ctx = ctx;
  out->group = group;
  out->n = n;
  out->identity_idx.clear();
}

// the XYZZ points of one chunk -> packed affine, unless the chunk's kernel flagged an identity
template <class C>
bh_status finish_chunk(bh_ctx* ctx, size_t k, void* d_xyzz, void* d_scr, uint32_t* d_flag, uint32_t* d_out) {
  uint32_t flag = 0;
  BH_TRY_HIP(hipGetLastError());
  BH_TRY_HIP(hipMemcpyAsync(&flag, d_flag, 4, hipMemcpyDeviceToHost, ctx->stream));
  BH_TRY_HIP(hipStreamSynchronize(ctx->stream));
  if (flag) return BH_ERR_UNEXPECTED_IDENTITY;
  BH_TRY_HIP(normalize_batch<C>(d_xyzz, k, d_scr, d_out, ctx->stream));
  BH_TRY_HIP(hipGetLastError());
  return BH_OK;
}

struct VbScratch {
  DevBuf xyzz, scr, flag;
  template <class C>
  bh_status alloc(bh_ctx* ctx, size_t n) {
    const size_t chunk = std::min(n, VB_CHUNK);
    BH_TRY_HIP(xyzz.alloc(chunk * sizeof(typename C::P)));
    BH_TRY_HIP(scr.alloc(chunk * sizeof(typename FieldOf<C>::F::T) + 64));
    BH_TRY_HIP(flag.alloc(4));
    BH_TRY_HIP(hipMemsetAsync(flag.p, 0, 4, ctx->stream));
    return BH_OK;
  }
};

}  // namespace

template <class C>
hipError_t varbase_multiples_table(const uint32_t* d_pts, size_t k, void* d_xyzz, void* d_scr, uint32_t* d_table,
                                   hipStream_t st) {
  hipLaunchKernelGGL(k_varbase_multiples<C>, dim3(nb(k, 256)), dim3(256), 0, st, d_pts, k,
                     reinterpret_cast<typename C::P*>(d_xyzz));
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  return normalize_batch<C>(d_xyzz, 8 * k, d_scr, d_table, st);
}
template hipError_t varbase_multiples_table<G1Ops>(const uint32_t*, size_t, void*, void*, uint32_t*, hipStream_t);
template hipError_t varbase_multiples_table<G2Ops>(const uint32_t*, size_t, void*, void*, uint32_t*, hipStream_t);

template <class C>
hipError_t varbase_mul_chunk(const uint32_t* d_pts, const uint32_t* d_sc, int stride, size_t k, int W, int top_biased,
                             void* d_xyzz, void* d_scr, uint32_t* d_table, uint32_t* d_flag, hipStream_t st) {
  using P = typename C::P;
  hipError_t e = varbase_multiples_table<C>(d_pts, k, d_xyzz, d_scr, d_table, st);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_varbase_mul_win<C>, dim3(nb(k, 256)), dim3(256), 0, st, d_table, d_sc, stride, k, W, top_biased,
                     reinterpret_cast<P*>(d_xyzz), d_flag);
  return hipGetLastError();
}
template hipError_t varbase_mul_chunk<G1Ops>(const uint32_t*, const uint32_t*, int, size_t, int, int, void*, void*,
                                             uint32_t*, uint32_t*, hipStream_t);
template hipError_t varbase_mul_chunk<G2Ops>(const uint32_t*, const uint32_t*, int, size_t, int, int, void*, void*,
                                             uint32_t*, uint32_t*, hipStream_t);

namespace {

// chunks of VB_WIN_CHUNK points; the table (8 affine records per point) and its XYZZ staging live
// in a workspace of the call
template <class C>
bh_status mul_win_t(bh_ctx* ctx, const bh_srs* in, const uint32_t* d_sc, int stride, int nbits, bh_srs* out) {
  using P = typename C::P;
  using T = typename FieldOf<C>::F::T;
  const size_t n = in->n;
  constexpr int words = HostOf<C>::WORDS;
  srs_init(ctx, in->group, n, out);
  BH_TRY_HIP(out->pts.alloc(std::max<size_t>(n, 1) * words * 4));
  if (!n) return BH_OK;
  const size_t chunk = std::min(n, VB_WIN_CHUNK);
  const int top_biased = nbits >= 253;
  const int W = top_biased ? 64 : (nbits + 3) / 4 + 1;
  DevBuf xyzz, scr, table, flag;
  BH_TRY_HIP(xyzz.alloc(8 * chunk * sizeof(P)));
  BH_TRY_HIP(scr.alloc(8 * chunk * sizeof(T) + 64));
  BH_TRY_HIP(table.alloc(8 * chunk * (size_t)words * 4));
  BH_TRY_HIP(flag.alloc(4));
  BH_TRY_HIP(hipMemsetAsync(flag.p, 0, 4, ctx->stream));
  for (size_t base = 0; base < n; base += chunk) {
    const size_t k = std::min(chunk, n - base);
    BH_TRY_HIP(varbase_mul_chunk<C>(in->pts.as<uint32_t>() + base * words, d_sc + base * (size_t)stride, stride, k, W,
                                    top_biased, xyzz.p, scr.p, table.as<uint32_t>(), flag.as<uint32_t>(), ctx->stream));
    if (bh_status s = finish_chunk<C>(ctx, k, xyzz.p, scr.p, flag.as<uint32_t>(), out->pts.as<uint32_t>() + base * words))
      return s;
  }
  BH_TRY_HIP(hipStreamSynchronize(ctx->stream));  // the workspace is freed on return
  return BH_OK;
}

template <class C>
bh_status sub_t(bh_ctx* ctx, const bh_srs* in, size_t lo1, size_t lo2, size_t n, bh_srs* out) {
  constexpr int words = HostOf<C>::WORDS;
  srs_init(ctx, in->group, n, out);
  BH_TRY_HIP(out->pts.alloc(std::max<size_t>(n, 1) * words * 4));
  if (!n) return BH_OK;
  VbScratch w;
  bh_status s = w.alloc<C>(ctx, n);
  if (s) return s;
  for (size_t base = 0; base < n; base += VB_CHUNK) {
    const size_t k = std::min(VB_CHUNK, n - base);
    hipLaunchKernelGGL(k_varbase_sub<C>, dim3(nb(k, 256)), dim3(256), 0, ctx->stream, in->pts.as<uint32_t>(),
                       lo1 + base, lo2 + base, k, reinterpret_cast<typename C::P*>(w.xyzz.p), w.flag.as<uint32_t>());
    if ((s = finish_chunk<C>(ctx, k, w.xyzz.p, w.scr.p, w.flag.as<uint32_t>(), out->pts.as<uint32_t>() + base * words)))
      return s;
  }
  BH_TRY_HIP(hipStreamSynchronize(ctx->stream));
  return BH_OK;
}

}  // namespace

bh_status varbase_mul(bh_ctx* ctx, const bh_srs* in, const uint32_t* d_sc, int stride, int nbits, bh_srs* out) {
  if (!in->identity_idx.empty()) return BH_ERR_UNEXPECTED_IDENTITY;
  if (nbits < 1 || nbits > 255 || (stride != 0 && stride != 8)) return BH_ERR_INVALID_ARGUMENT;
  return with_group(in->group,
                    [&](auto g) { return mul_win_t<typename decltype(g)::Ops>(ctx, in, d_sc, stride, nbits, out); });
}

bh_status varbase_sub(bh_ctx* ctx, const bh_srs* in, size_t lo1, size_t lo2, size_t n, bh_srs* out) {
  if (n > in->n || lo1 > in->n - n || lo2 > in->n - n) return BH_ERR_INVALID_ARGUMENT;
  for (size_t i : in->identity_idx)
    if ((i >= lo1 && i < lo1 + n) || (i >= lo2 && i < lo2 + n)) return BH_ERR_UNEXPECTED_IDENTITY;
  return with_group(in->group, [&](auto g) { return sub_t<typename decltype(g)::Ops>(ctx, in, lo1, lo2, n, out); });
}

bh_status varbase_power_scalars(bh_ctx* ctx, size_t n, const uint64_t a_w[4], const uint64_t x_w[4], int invert,
                                DevBuf* d_sc) {
  if (!scalar_below_r(a_w) || !scalar_below_r(x_w) || n > 0x7fffffffull) return BH_ERR_INVALID_ARGUMENT;
  if (scalar_is_zero(a_w) || scalar_is_zero(x_w)) return BH_ERR_UNEXPECTED_IDENTITY;  // a zero scalar: the identity
  Fr a = fr_from_canonical(a_w), x = fr_from_canonical(x_w);
  if (invert) {  // (a x^i)^-1 = a^-1 (x^-1)^i
    a = inv(a);
    x = inv(x);
  }
  BH_TRY_HIP(d_sc->alloc(std::max<size_t>(n, 1) * 32));
  if (!n) return BH_OK;
  int L = 0;
  while (((size_t)1 << L) < n) L++;
  const int lo_bits = (L + 1) / 2;
  DevBuf lo, hi;
  bh_status s = upload_split_table(ctx, lo, hi, x, a, L, lo_bits);
  if (s) return s;
  hipLaunchKernelGGL(k_varbase_powers, dim3(nb(n, 256)), dim3(256), 0, ctx->stream, d_sc->as<uint32_t>(), (uint32_t)n,
                     lo.as<uint32_t>(), hi.as<uint32_t>(), lo_bits);
  BH_TRY_HIP(hipGetLastError());
  BH_TRY_HIP(hipStreamSynchronize(ctx->stream));  // the tables are freed on return
  return BH_OK;
}

bh_status varbase_upload_scalars(bh_ctx* ctx, const uint64_t* scalars, size_t count, int nbits, DevBuf* d_sc) {
  if (nbits < 1 || nbits > 255) return BH_ERR_INVALID_ARGUMENT;
  for (size_t i = 0; i < count; i++)
    if (!scalar_below_r(scalars + 4 * i) || scalar_bits(scalars + 4 * i) > nbits) return BH_ERR_INVALID_ARGUMENT;
  BH_TRY_HIP(d_sc->alloc(std::max<size_t>(count, 1) * 32));
  if (count) {
    BH_TRY_HIP(hipMemcpyAsync(d_sc->p, scalars, count * 32, hipMemcpyHostToDevice, ctx->stream));
    BH_TRY_HIP(hipStreamSynchronize(ctx->stream));
  }
  return BH_OK;
}

}  // namespace bh

extern "C" {

bh_status bh_srs_mul_each_bounded(bh_ctx* ctx, const bh_srs* in, const uint64_t* scalars, size_t n_scalars, int nbits,
                                  bh_srs** out) {
  if (!ctx || !in || !out || !in->ctx || in->ctx->device != ctx->device || (n_scalars && !scalars)) return BH_ERR_INVALID_ARGUMENT;
  if (n_scalars != in->n && n_scalars != 1) return BH_ERR_INVALID_ARGUMENT;
  std::lock_guard<std::mutex> lk(ctx->mu);
  BH_TRY_HIP(hipSetDevice(ctx->device));
  bh_status s = scratch_check(ctx);
  if (s) return s;
  DevBuf d_sc;
  if ((s = varbase_upload_scalars(ctx, scalars, n_scalars, nbits, &d_sc))) return s;
  std::unique_ptr<bh_srs> r(new bh_srs());
  if ((s = varbase_mul(ctx, in, d_sc.as<uint32_t>(), n_scalars == in->n ? 8 : 0, nbits, r.get()))) return s;
  *out = r.release();
  return BH_OK;
}

bh_status bh_srs_mul_each(bh_ctx* ctx, const bh_srs* in, const uint64_t* scalars, size_t n, bh_srs** out) {
  if (!in || n != in->n) return BH_ERR_INVALID_ARGUMENT;
  return bh_srs_mul_each_bounded(ctx, in, scalars, n, 255, out);
}

bh_status bh_srs_mul_powers(bh_ctx* ctx, const bh_srs* in, const uint64_t a[4], const uint64_t x[4], int invert,
                            bh_srs** out) {
  if (!ctx || !in || !a || !x || !out || !in->ctx || in->ctx->device != ctx->device) return BH_ERR_INVALID_ARGUMENT;
  std::lock_guard<std::mutex> lk(ctx->mu);
  BH_TRY_HIP(hipSetDevice(ctx->device));
  bh_status s = scratch_check(ctx);
  if (s) return s;
  DevBuf d_sc;
  if ((s = varbase_power_scalars(ctx, in->n, a, x, invert, &d_sc))) return s;
  const uint64_t one[4] = {1, 0, 0, 0};
  std::unique_ptr<bh_srs> r(new bh_srs());
  if ((s = varbase_mul(ctx, in, d_sc.as<uint32_t>(), memcmp(x, one, 32) ? 8 : 0, 255, r.get()))) return s;
  *out = r.release();
  return BH_OK;
}

bh_status bh_srs_sub_range(bh_ctx* ctx, const bh_srs* in, size_t lo1, size_t lo2, size_t n, bh_srs** out) {
  if (!ctx || !in || !out || !in->ctx || in->ctx->device != ctx->device) return BH_ERR_INVALID_ARGUMENT;
  std::lock_guard<std::mutex> lk(ctx->mu);
  BH_TRY_HIP(hipSetDevice(ctx->device));
  bh_status s = scratch_check(ctx);
  if (s) return s;
  std::unique_ptr<bh_srs> r(new bh_srs());
  if ((s = varbase_sub(ctx, in, lo1, lo2, n, r.get()))) return s;
  *out = r.release();
  return BH_OK;
}

}  // extern "C"
