// The step between the ceremony's two rounds: a group-valued FFT of a device point vector
// (EvaluationDomain<Point<G>>, reference domain.rs:81-99 and 192-228) and the circuit's sparse
// matrices applied to point vectors (list_mul_matrix, groth16/mpc.rs:416-457, with the evaluation
// order of eval, generator.rs:411-510).
//
// The transform is radix-2 decimation in time in constant geometry.  Stage s = 0 .. L-1 reads the
// pair (u, v) = (x[2b], x[2b + 1]) of butterfly b < n/2 and writes y[b] = u + w v and
// y[b + n/2] = u - w v with w = omega^(b & ~(2^(L-1-s) - 1)): every stage has the same shape, one
// twiddle table omega^e, e < n/2, serves all of them, and the butterflies with w = 1 are the prefix
// b < 2^(L-1-s) of a stage (the whole first stage, n - 1 in all).  The first stage skips the
// multiplication; the later stages' prefixes multiply by one like the rest, because cutting a
// stage into a range that multiplies and one that does not measured slower than the multiplications
// it saves.
// A stage's array is kept split, its even elements in the first half and its odd ones in the
// second (element i at rotr(i)), so that u, v and the bases of the multiplication are read as
// consecutive records; the last stage writes natural order.  The input is gathered once:
// physical q <- in[bitrev(rotl(q))].
//
//   k_gfft_gather      that gather, one lane per 16 bytes
//   k_gfft_twiddles    a chunk's scalars: tw[(b0 + l) & ~mask], canonical, as k_varbase_powers wrote them
//   k_varbase_multiples + k_varbase_mul_win (varbase.hip)   t = w v
//   k_gfft_butterfly   u + t and u - t from two packed affine points in one lane: both share
//                      x_t - x_u, its square and cube and x_u times the square
//   k_normalize (crs.hip) between stages
// A butterfly output that is the identity raises the device flag, which the host reads before the
// normalisation: the call then returns BH_ERR_UNEXPECTED_IDENTITY and no vector.
//
// The matrix product, per matrix (A, B or C) and point vector, in chunks of whole segments:
//   k_gfft_gather_rows base i of the chunk = Lag[row[t0 + i]]
//   k_varbase_multiples + k_varbase_mul_win   coeff[t] / m (canonical) times that base, left as XYZZ
//   k_gfft_seg_sum     one lane per segment of at most R1CS_S terms adds its products
//   k_gfft_col_sum     one lane per column adds its (at most R1CS_S) partial sums
//   k_gfft_col_long    one wave per column of more partial sums
//   k_gfft_flags       per variable: is the sum the identity
//   k_gfft_compact     the identity filter (generator.rs:614-632) on XYZZ points, order kept
// Group addition is exact (curve.cuh), so the order of the partial sums does not matter.
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <memory>

#include "crs.h"
#include "group_fft.h"
#include "varbase.h"

using namespace bh;

namespace bh {

template <class C>
__device__ __forceinline__ typename C::A gf_load_affine(const uint32_t* base, size_t i) {
  using F = typename FieldOf<C>::F;
  constexpr int PW = F::PACKED_WORDS;
  typename C::A a;
  a.x = F::unpack(base + i * 2 * PW);
  a.y = F::unpack(base + i * 2 * PW + PW);
  return a;
}

// Q: uint4 per record.  out[q] = in[bitrev_L(rotl_L(q))], q < 2^L
template <int Q>
__global__ void __launch_bounds__(256) k_gfft_gather(const uint4* in, uint4* out, uint32_t L) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t n = (size_t)1 << L;
  if (t >= n * Q) return;
  const uint32_t q = (uint32_t)(t / Q), part = (uint32_t)(t % Q);
  const uint32_t i = ((q << 1) | (q >> (L - 1))) & (uint32_t)(n - 1);
  const uint32_t src = __brev(i) >> (32 - L);
  out[t] = in[(size_t)src * Q + part];
}

// out[l] = tw[(b0 + l) & ~mask], l < k: 8 words each
__global__ void __launch_bounds__(256) k_gfft_twiddles(const uint4* tw, uint32_t b0, uint32_t mask, uint32_t k,
                                                       uint4* out) {
  const uint32_t l = blockIdx.x * blockDim.x + threadIdx.x;
  if (l >= k) return;
  const size_t e = (b0 + l) & ~mask;
  out[2 * (size_t)l] = tw[2 * e];
  out[2 * (size_t)l + 1] = tw[2 * e + 1];
}

// (u, t) -> (u + t, u - t) for affine u, t, neither the identity: madd-2008-s of u with ZZ = ZZZ = 1
// for t and for -t, which differ in R alone.  x_t == x_u: t == u gives (2u, O), t == -u gives
// (O, 2u), by curve.cuh's dbl_affine.
// split: butterfly l of the chunk writes slot (l & 1) * k + (l >> 1) and, k / 2 further, its
// difference (the next stage's even | odd halves); otherwise l and k + l.
template <class C>
__global__ void __launch_bounds__(256) k_gfft_butterfly(const uint32_t* up, const uint32_t* tp, size_t k, int split,
                                                        typename C::P* out, uint32_t* flag) {
  using F = typename FieldOf<C>::F;
  using T = typename F::T;
  const size_t l = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (l >= k) return;
  const typename C::A u = gf_load_affine<C>(up, l);
  const typename C::A t = gf_load_affine<C>(tp, l);
  typename C::P s, d;
  const T Pd = F::template sub<C::KX>(t.x, u.x);
  const T R = F::template sub<C::KY>(t.y, u.y);
  if (F::is_zero(Pd)) {
    if (F::is_zero(R)) {
      s = C::dbl_affine(u);
      d = C::identity();
    } else {
      s = C::identity();
      d = C::dbl_affine(u);
    }
  } else {
    const T Rn = F::template sub<C::KY>(C::neg_affine(t).y, u.y);
    const T PP = F::sqr(Pd);
    const T PPP = F::mul(Pd, PP);
    const T Q = F::mul(u.x, PP);
    const T sub3 = F::add(PPP, F::add(Q, Q));
    s.X = F::template sub<C::K1>(F::sqr(R), sub3);
    s.Y = F::template mul_sub<C::KY>(R, F::template sub<C::K2>(Q, s.X), u.y, PPP);
    s.ZZ = PP;
    s.ZZZ = PPP;
    d.X = F::template sub<C::K1>(F::sqr(Rn), sub3);
    d.Y = F::template mul_sub<C::KY>(Rn, F::template sub<C::K2>(Q, d.X), u.y, PPP);
    d.ZZ = PP;
    d.ZZZ = PPP;
  }
  if (C::is_identity(s) || C::is_identity(d)) atomicOr(flag, 1u);
  const size_t lo = split ? (l & 1) * k + (l >> 1) : l;
  out[lo] = s;
  out[lo + (split ? k / 2 : k)] = d;
}

// ---- the matrix product
template <int Q>
__global__ void __launch_bounds__(256) k_gfft_gather_rows(const uint4* lag, const uint32_t* row, size_t k, uint4* out) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= k * Q) return;
  const size_t i = t / Q;
  out[t] = lag[(size_t)row[i] * Q + (t % Q)];
}

// segments k0 .. k1 of the term array: part[k - kbase] = sum of prod[t - tbase], t in seg[k] .. seg[k + 1]
template <class C>
__global__ void __launch_bounds__(256) k_gfft_seg_sum(const typename C::P* prod, const uint32_t* seg, uint32_t k0,
                                                      uint32_t k1, uint32_t tbase, uint32_t kbase,
                                                      typename C::P* part) {
  const uint32_t k = k0 + blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= k1) return;
  const uint32_t t0 = seg[k], t1 = seg[k + 1];
  typename C::P acc = C::identity();
#pragma unroll 1
  for (uint32_t t = t0; t < t1; t++) acc = C::add(acc, prod[t - tbase]);
  part[k - kbase] = acc;
}

// columns c0 .. c0 + n of the matrix whose first segment is kbase: y[j] (+)= the column's partial sums
template <class C>
__global__ void __launch_bounds__(256) k_gfft_col_sum(const uint32_t* colseg, uint32_t c0, uint32_t n, uint32_t kbase,
                                                      const typename C::P* part, int accumulate, typename C::P* y) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  const uint32_t p0 = colseg[c0 + j], p1 = colseg[c0 + j + 1];
  if (p1 - p0 > R1CS_S) return;  // k_gfft_col_long's
  typename C::P acc = accumulate ? y[j] : C::identity();
#pragma unroll 1
  for (uint32_t p = p0; p < p1; p++) acc = C::add(acc, part[p - kbase]);
  y[j] = acc;
}

// one wave per long column; those of other matrices than columns c0 .. c0 + n leave at once
template <class C>
__global__ void __launch_bounds__(64) k_gfft_col_long(const uint32_t* longcols, const uint32_t* colseg, uint32_t c0,
                                                      uint32_t n, uint32_t kbase, const typename C::P* part,
                                                      int accumulate, typename C::P* y) {
  __shared__ typename C::P sh[32];
  const uint32_t col = longcols[blockIdx.x];
  if (col < c0 || col - c0 >= n) return;
  const uint32_t p0 = colseg[col], p1 = colseg[col + 1];
  const uint32_t lane = threadIdx.x;
  typename C::P acc = C::identity();
#pragma unroll 1
  for (uint32_t p = p0 + lane; p < p1; p += 64) acc = C::add(acc, part[p - kbase]);
#pragma unroll 1
  for (uint32_t off = 32; off; off >>= 1) {
    if (lane >= off && lane < 2 * off) sh[lane - off] = acc;
    __syncthreads();
    if (lane < off) acc = C::add(acc, sh[lane]);
    __syncthreads();
  }
  if (lane == 0) y[col - c0] = accumulate ? C::add(y[col - c0], acc) : acc;
}

// f[j] = y[j] is not the identity; cnt[0] / cnt[1]: the identities among the first ni / the rest
template <class C>
__global__ void __launch_bounds__(256) k_gfft_flags(const typename C::P* y, uint32_t n, uint32_t ni, uint32_t* f,
                                                    uint32_t* cnt) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  const bool id = C::is_identity(y[j]);
  f[j] = id ? 0u : 1u;
  if (id) atomicAdd(&cnt[j < ni ? 0 : 1], 1u);
}

template <class C>
__global__ void __launch_bounds__(256) k_gfft_compact(const typename C::P* y, const uint32_t* f, const uint32_t* pos,
                                                      uint32_t n, typename C::P* out) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n || !f[j]) return;
  out[pos[j]] = y[j];
}

void group_fft_kernels(std::vector<KernInfo>& v) {
  v.push_back({"k_gfft_gather<G1>", (const void*)k_gfft_gather<6>, 256, 0});
  v.push_back({"k_gfft_gather<G2>", (const void*)k_gfft_gather<12>, 256, 0});
  v.push_back({"k_gfft_twiddles", (const void*)k_gfft_twiddles, 256, 0});
  v.push_back({"k_gfft_butterfly<G1>", (const void*)k_gfft_butterfly<G1Ops>, 256, 0});
  v.push_back({"k_gfft_butterfly<G2>", (const void*)k_gfft_butterfly<G2Ops>, 256, 0});
  v.push_back({"k_gfft_gather_rows<G1>", (const void*)k_gfft_gather_rows<6>, 256, 0});
  v.push_back({"k_gfft_gather_rows<G2>", (const void*)k_gfft_gather_rows<12>, 256, 0});
  v.push_back({"k_gfft_seg_sum<G1>", (const void*)k_gfft_seg_sum<G1Ops>, 256, 0});
  v.push_back({"k_gfft_seg_sum<G2>", (const void*)k_gfft_seg_sum<G2Ops>, 256, 0});
  v.push_back({"k_gfft_col_sum<G1>", (const void*)k_gfft_col_sum<G1Ops>, 256, 0});
  v.push_back({"k_gfft_col_sum<G2>", (const void*)k_gfft_col_sum<G2Ops>, 256, 0});
  v.push_back({"k_gfft_col_long<G1>", (const void*)k_gfft_col_long<G1Ops>, 64, 0});
  v.push_back({"k_gfft_col_long<G2>", (const void*)k_gfft_col_long<G2Ops>, 64, 0});
  v.push_back({"k_gfft_flags<G1>", (const void*)k_gfft_flags<G1Ops>, 256, 0});
  v.push_back({"k_gfft_flags<G2>", (const void*)k_gfft_flags<G2Ops>, 256, 0});
  v.push_back({"k_gfft_compact<G1>", (const void*)k_gfft_compact<G1Ops>, 256, 0});
  v.push_back({"k_gfft_compact<G2>", (const void*)k_gfft_compact<G2Ops>, 256, 0});
}

namespace {

inline unsigned nb(size_t n, unsigned bs) { return (unsigned)((n + bs - 1) / bs); }

// omega of the domain of size 2^L, or its inverse: root_of_unity^(2^(32 - L)) (domain.rs:62-66)
Fr domain_root(int L, int inverse) {
  uint64_t rou_raw[4] = {0x3829971f439f0d2bull, 0xb63683508c2280b9ull, 0xd09b681922c813b4ull, 0x16a2a19edfe81f20ull};
  Fr omega = from_int<4>(rou_raw);
  for (int i = L; i < 32; i++) omega = sqr(omega);
  return inverse ? inv(omega) : omega;
}
Fr fr_of(uint64_t v) {
  uint64_t x[4] = {v, 0, 0, 0};
  return from_int<4>(x);
}

// the workspace of the windowed multiplication (varbase_mul_chunk) for chunks of `chunk` points
template <class C>
struct MulWork {
  DevBuf xyzz, scr, table, flag;
  bh_status alloc(bh_ctx* ctx, size_t chunk) {
    BH_TRY_HIP(xyzz.alloc(8 * chunk * sizeof(typename C::P)));
    BH_TRY_HIP(scr.alloc(8 * chunk * sizeof(typename FieldOf<C>::F::T) + 64));
    BH_TRY_HIP(table.alloc(8 * chunk * (size_t)HostOf<C>::WORDS * 4));
    BH_TRY_HIP(flag.alloc(8));
    BH_TRY_HIP(hipMemsetAsync(flag.p, 0, 8, ctx->stream));
    return BH_OK;
  }
};

void srs_init(bh_ctx* ctx, int group, size_t n, bh_srs* out) {
  out->ctx = ctx;
  out->group = group;
  out->n = n;
  out->identity_idx.clear();
}

template <class C>
bh_status fft_t(bh_ctx* ctx, const bh_srs* in, size_t n, int L, int inverse, bool scale, bh_srs* out) {
  using P = typename C::P;
  constexpr int words = HostOf<C>::WORDS;
  hipStream_t st = ctx->stream;
  const size_t half = n / 2;
  const size_t chunk = std::min(half, VB_WIN_CHUNK);
  // BH_GROUP_FFT_W1 selects what the butterflies with w = 1 do (a measurement mode, like
  // BH_MPC_HOST_MILLER; results do not depend on it): unset, the first stage skips its
  // multiplications; "none": every butterfly multiplies; "prefix": every stage's prefix skips
  const char* env = getenv("BH_GROUP_FFT_W1");
  const int w1 = !env ? 1 : !strcmp(env, "none") ? 0 : !strcmp(env, "prefix") ? 2 : 1;
  // twiddles omega^(+-e), e < n / 2
  uint64_t one[4] = {1, 0, 0, 0}, root[4];
  fr_to_canonical(domain_root(L, inverse), root);
  DevBuf d_tw, d_sc, cur, nxt, tbuf, bxyzz;
  bh_status s = varbase_power_scalars(ctx, half, one, root, 0, &d_tw);
  if (s) return s;
  MulWork<C> w;
  if ((s = w.alloc(ctx, chunk))) return s;
  BH_TRY_HIP(d_sc.alloc(chunk * 32));
  BH_TRY_HIP(cur.alloc(n * words * 4));
  BH_TRY_HIP(nxt.alloc(n * words * 4));
  BH_TRY_HIP(tbuf.alloc(chunk * words * 4));
  BH_TRY_HIP(bxyzz.alloc(2 * chunk * sizeof(P)));
  uint32_t* flag = w.flag.template as<uint32_t>();
  hipLaunchKernelGGL(k_gfft_gather<words / 4>, dim3(nb(n * (words / 4), 256)), dim3(256), 0, st,
                     in->pts.as<uint4>(), cur.as<uint4>(), (uint32_t)L);
  BH_TRY_HIP(hipGetLastError());
  for (int stage = 0; stage < L; stage++) {
    const bool last = stage == L - 1;
    // the butterflies that skip the multiplication
    const size_t n1 = w1 == 2 ? (size_t)1 << (L - 1 - stage) : (w1 == 1 && stage == 0) ? half : 0;
    const uint32_t mask = (uint32_t)(((size_t)1 << (L - 1 - stage)) - 1);
    const uint32_t* x = cur.as<uint32_t>();
    uint32_t* y = nxt.as<uint32_t>();
    for (int mul = 0; mul < 2; mul++) {
      const size_t lo = mul ? n1 : 0, hi = mul ? half : n1;
      for (size_t b0 = lo; b0 < hi; b0 += chunk) {
        const size_t k = std::min(chunk, hi - b0);
        const uint32_t* v = x + (half + b0) * words;
        if (mul) {  // t = w v
          hipLaunchKernelGGL(k_gfft_twiddles, dim3(nb(k, 256)), dim3(256), 0, st, d_tw.as<uint4>(), (uint32_t)b0, mask,
                             (uint32_t)k, d_sc.as<uint4>());
          BH_TRY_HIP(hipGetLastError());
          BH_TRY_HIP(varbase_mul_chunk<C>(v, d_sc.as<uint32_t>(), 8, k, 64, 1, w.xyzz.p, w.scr.p,
                                          w.table.template as<uint32_t>(), flag, st));
          BH_TRY_HIP(normalize_batch<C>(w.xyzz.p, k, w.scr.p, tbuf.as<uint32_t>(), st));
          v = tbuf.as<uint32_t>();
        }
        hipLaunchKernelGGL(k_gfft_butterfly<C>, dim3(nb(k, 256)), dim3(256), 0, st, x + b0 * words, v, k, last ? 0 : 1,
                           bxyzz.as<P>(), flag);
        BH_TRY_HIP(hipGetLastError());
        uint32_t f = 0;
        BH_TRY_HIP(hipMemcpyAsync(&f, flag, 4, hipMemcpyDeviceToHost, st));
        BH_TRY_HIP(hipStreamSynchronize(st));
        if (f) return BH_ERR_UNEXPECTED_IDENTITY;  // before the normalisation a zero ZZ would poison
        const P* bx = bxyzz.as<P>();
        if (last) {
          BH_TRY_HIP(normalize_batch<C>(bx, k, w.scr.p, y + b0 * words, st));
          BH_TRY_HIP(normalize_batch<C>(bx + k, k, w.scr.p, y + (half + b0) * words, st));
        } else {  // (k and b0 are even: every range of a stage but the last is)
          for (int q = 0; q < 4; q++)
            BH_TRY_HIP(normalize_batch<C>(bx + q * (k / 2), k / 2, w.scr.p,
                                          y + ((q >> 1) * half + (q & 1) * (half / 2) + b0 / 2) * words, st));
        }
      }
    }
    std::swap(cur.p, nxt.p);
    std::swap(cur.bytes, nxt.bytes);
  }
  BH_TRY_HIP(hipStreamSynchronize(st));
  srs_init(ctx, in->group, n, out);
  if (inverse && scale) {  // the 1/n of ifft (domain.rs:104-121): one scalar for the vector
    bh_srs tmp;
    srs_init(ctx, in->group, n, &tmp);
    std::swap(tmp.pts.p, cur.p);
    std::swap(tmp.pts.bytes, cur.bytes);
    uint64_t ninv[4];
    fr_to_canonical(inv(fr_of(n)), ninv);
    DevBuf d_ninv;
    if ((s = varbase_upload_scalars(ctx, ninv, 1, 255, &d_ninv))) return s;
    return varbase_mul(ctx, &tmp, d_ninv.as<uint32_t>(), 0, 255, out);
  }
  std::swap(out->pts.p, cur.p);
  std::swap(out->pts.bytes, cur.bytes);
  return BH_OK;
}

// launch_fr_convert's constant that multiplies a device value by k and leaves it canonical: the raw
// 29-bit limbs of the integer k (r1cs.hip: canonical_times)
FrConst canonical_times(const Fr& k) {
  uint64_t raw[4];
  fr_to_canonical(k, raw);
  FrConst c;
  for (int i = 0; i < 9; i++) {
    const int bit = 29 * i, w = bit >> 6, sh = bit & 63;
    uint64_t lo = raw[w] >> sh;
    if (sh > 35 && w + 1 < 4) lo |= raw[w + 1] << (64 - sh);
    c.v[i] = (uint32_t)(lo & 0x1fffffffu);
  }
  return c;
}

// what the host keeps of the segment scheme to cut a matrix into chunks of whole segments
struct SegPlan {
  std::vector<uint32_t> seg;  // nseg + 1
  uint32_t first[4];          // first segment of A, B, C, and nseg
};

template <class C>
struct MatWork {
  MulWork<C> mul;
  DevBuf bases, part;
};

// y[j] (+)= sum over column j of matrix k of (coeff / m) * lag[row], j < n
template <class C>
bh_status col_product(bh_ctx* ctx, const bh_r1cs* r, const SegPlan& plan, MatWork<C>& w, int k, const bh_srs* lag,
                      const uint32_t* d_sc, int accumulate, typename C::P* y) {
  using P = typename C::P;
  constexpr int words = HostOf<C>::WORDS;
  hipStream_t st = ctx->stream;
  const size_t n = r->ni + r->na;
  const uint32_t kbase = plan.first[k], kend = plan.first[k + 1];
  uint32_t* dummy = w.mul.flag.template as<uint32_t>() + 1;  // a zero coefficient is legal: the identity
  for (uint32_t k0 = kbase; k0 < kend;) {
    // as many whole segments as fit the multiplication's chunk (a segment has at most R1CS_S terms)
    uint32_t k1 = k0;
    const uint32_t tbase = plan.seg[k0];
    while (k1 < kend && plan.seg[k1 + 1] - tbase <= VB_WIN_CHUNK) k1++;
    const size_t cnt = plan.seg[k1] - tbase;
    if (cnt) {
      hipLaunchKernelGGL(k_gfft_gather_rows<words / 4>, dim3(nb(cnt * (words / 4), 256)), dim3(256), 0, st,
                         lag->pts.as<uint4>(), r->row.as<uint32_t>() + tbase, cnt, w.bases.template as<uint4>());
      BH_TRY_HIP(hipGetLastError());
      BH_TRY_HIP(varbase_mul_chunk<C>(w.bases.template as<uint32_t>(), d_sc + (size_t)tbase * 8, 8, cnt, 64, 1,
                                      w.mul.xyzz.p, w.mul.scr.p, w.mul.table.template as<uint32_t>(), dummy, st));
    }
    hipLaunchKernelGGL(k_gfft_seg_sum<C>, dim3(nb(k1 - k0, 256)), dim3(256), 0, st, w.mul.xyzz.template as<P>(),
                       r->seg.as<uint32_t>(), k0, k1, tbase, kbase, w.part.template as<P>());
    BH_TRY_HIP(hipGetLastError());
    k0 = k1;
  }
  hipLaunchKernelGGL(k_gfft_col_sum<C>, dim3(nb(n, 256)), dim3(256), 0, st, r->colseg.as<uint32_t>(),
                     (uint32_t)(k * n), (uint32_t)n, kbase, w.part.template as<P>(), accumulate, y);
  BH_TRY_HIP(hipGetLastError());
  if (r->nlong) {
    hipLaunchKernelGGL(k_gfft_col_long<C>, dim3((unsigned)r->nlong), dim3(64), 0, st, r->longcols.as<uint32_t>(),
                       r->colseg.as<uint32_t>(), (uint32_t)(k * n), (uint32_t)n, kbase, w.part.template as<P>(),
                       accumulate, y);
    BH_TRY_HIP(hipGetLastError());
  }
  return BH_OK;
}

struct FilterWork {
  DevBuf flags, pos, scan, cnt;
};

// y (n XYZZ sums) -> the non-identity ones, in order, as packed affine (generator.rs:614-632)
template <class C>
bh_status filtered(bh_ctx* ctx, const typename C::P* y, size_t n, FilterWork& fw, DevBuf& dense, void* scr,
                   bh_srs* out) {
  using P = typename C::P;
  hipStream_t st = ctx->stream;
  uint32_t* f = fw.flags.as<uint32_t>();
  uint32_t* pos = fw.pos.as<uint32_t>();
  hipLaunchKernelGGL(k_gfft_flags<C>, dim3(nb(n, 256)), dim3(256), 0, st, y, (uint32_t)n, (uint32_t)n, f,
                     fw.cnt.as<uint32_t>());
  BH_TRY_HIP(hipGetLastError());
  exclusive_scan(f, pos, n, fw.scan.as<uint32_t>(), st);
  BH_TRY_HIP(hipGetLastError());
  hipLaunchKernelGGL(k_gfft_compact<C>, dim3(nb(n, 256)), dim3(256), 0, st, y, f, pos, (uint32_t)n, dense.as<P>());
  BH_TRY_HIP(hipGetLastError());
  uint32_t hw[2] = {0, 0};
  BH_TRY_HIP(hipMemcpyAsync(&hw[0], pos + n - 1, 4, hipMemcpyDeviceToHost, st));
  BH_TRY_HIP(hipMemcpyAsync(&hw[1], f + n - 1, 4, hipMemcpyDeviceToHost, st));
  BH_TRY_HIP(hipStreamSynchronize(st));
  const size_t cnt = (size_t)hw[0] + hw[1];
  srs_init(ctx, HostOf<C>::ID, cnt, out);
  BH_TRY_HIP(out->pts.alloc(std::max<size_t>(cnt, 1) * HostOf<C>::WORDS * 4));
  BH_TRY_HIP(normalize_batch<C>(dense.p, cnt, scr, out->pts.as<uint32_t>(), st));
  BH_TRY_HIP(hipStreamSynchronize(st));
  return BH_OK;
}

// One group's share of matrix_product.  lag: tau, alpha tau, beta tau of the group; ab[k] != null:
// the filtered sums of matrix k (A, B) against tau; kin, kout: beta A + alpha B + C
template <class C>
bh_status product_t(bh_ctx* ctx, const bh_r1cs* r, const SegPlan& plan, const uint32_t* d_sc,
                    const bh_srs* const lag[3], bh_srs* const ab[2], bh_srs* kin, bh_srs* kout) {
  using P = typename C::P;
  using T = typename FieldOf<C>::F::T;
  constexpr int words = HostOf<C>::WORDS;
  hipStream_t st = ctx->stream;
  const size_t n = r->ni + r->na, ni = r->ni, na = r->na;
  const size_t chunk = VB_WIN_CHUNK;
  uint32_t maxseg = 1;
  for (int k = 0; k < 3; k++) maxseg = std::max(maxseg, plan.first[k + 1] - plan.first[k]);
  MatWork<C> w;
  bh_status s = w.mul.alloc(ctx, std::min<size_t>(chunk, std::max<size_t>(r->terms, 1)));
  if (s) return s;
  FilterWork fw;
  DevBuf y, dense, scr;
  BH_TRY_HIP(w.bases.alloc(std::min<size_t>(chunk, std::max<size_t>(r->terms, 1)) * words * 4));
  BH_TRY_HIP(w.part.alloc((size_t)maxseg * sizeof(P)));
  BH_TRY_HIP(y.alloc(n * sizeof(P)));
  BH_TRY_HIP(dense.alloc(n * sizeof(P)));
  BH_TRY_HIP(scr.alloc(n * sizeof(T) + 64));
  BH_TRY_HIP(fw.flags.alloc(n * 4));
  BH_TRY_HIP(fw.pos.alloc(n * 4));
  BH_TRY_HIP(fw.scan.alloc(scan_scratch_words(n) * 4 + 64));
  BH_TRY_HIP(fw.cnt.alloc(8));
  for (int k = 0; k < 2; k++) {
    if (!ab[k]) continue;
    if ((s = col_product<C>(ctx, r, plan, w, k, lag[0], d_sc, 0, y.as<P>()))) return s;
    if ((s = filtered<C>(ctx, y.as<P>(), n, fw, dense, scr.p, ab[k]))) return s;
  }
  // beta A_j + alpha B_j + C_j (generator.rs:500-510 without the division, which is round two's)
  const bh_srs* kl[3] = {lag[2], lag[1], lag[0]};
  for (int k = 0; k < 3; k++)
    if ((s = col_product<C>(ctx, r, plan, w, k, kl[k], d_sc, k != 0, y.as<P>()))) return s;
  BH_TRY_HIP(hipMemsetAsync(fw.cnt.p, 0, 8, st));
  hipLaunchKernelGGL(k_gfft_flags<C>, dim3(nb(n, 256)), dim3(256), 0, st, y.as<P>(), (uint32_t)n, (uint32_t)ni,
                     fw.flags.as<uint32_t>(), fw.cnt.as<uint32_t>());
  BH_TRY_HIP(hipGetLastError());
  uint32_t cnt[2] = {0, 0};
  BH_TRY_HIP(hipMemcpyAsync(cnt, fw.cnt.p, 8, hipMemcpyDeviceToHost, st));
  BH_TRY_HIP(hipStreamSynchronize(st));
  if (cnt[1]) return BH_ERR_UNCONSTRAINED_VARIABLE;  // generator.rs:586-590
  if (cnt[0]) return BH_ERR_UNEXPECTED_IDENTITY;
  srs_init(ctx, HostOf<C>::ID, ni, kin);
  srs_init(ctx, HostOf<C>::ID, na, kout);
  BH_TRY_HIP(kin->pts.alloc(std::max<size_t>(ni, 1) * words * 4));
  BH_TRY_HIP(kout->pts.alloc(std::max<size_t>(na, 1) * words * 4));
  BH_TRY_HIP(normalize_batch<C>(y.as<P>(), ni, scr.p, kin->pts.as<uint32_t>(), st));
  BH_TRY_HIP(normalize_batch<C>(y.as<P>() + ni, na, scr.p, kout->pts.as<uint32_t>(), st));
  BH_TRY_HIP(hipStreamSynchronize(st));  // the workspace is freed on return
  return BH_OK;
}

}  // namespace

bh_status group_fft(bh_ctx* ctx, const bh_srs* in, size_t n, int inverse, bool scale, bh_srs* out) {
  if (n < 2 || n > ((size_t)1 << 28) || (n & (n - 1)) || n > in->n) return BH_ERR_INVALID_ARGUMENT;
  for (size_t i : in->identity_idx)
    if (i < n) return BH_ERR_UNEXPECTED_IDENTITY;
  int L = 0;
  while (((size_t)1 << L) < n) L++;
  return with_group(in->group, [&](auto g) {
    return fft_t<typename decltype(g)::Ops>(ctx, in, n, L, inverse ? 1 : 0, scale, out);
  });
}

bh_status matrix_product(bh_ctx* ctx, const bh_r1cs* r, const bh_srs* const lag[6], bh_srs* const out[7]) {
  hipStream_t st = ctx->stream;
  const size_t n = r->ni + r->na;
  for (int k = 0; k < 6; k++)
    if (lag[k]->n != r->m || lag[k]->group != (k & 1 ? BH_G2 : BH_G1)) return BH_ERR_INVALID_ARGUMENT;
  SegPlan plan;
  plan.seg.resize(r->nseg + 1);
  BH_TRY_HIP(hipMemcpyAsync(plan.seg.data(), r->seg.p, (r->nseg + 1) * 4, hipMemcpyDeviceToHost, st));
  for (int k = 0; k < 4; k++)
    BH_TRY_HIP(hipMemcpyAsync(&plan.first[k], r->colseg.as<uint32_t>() + (size_t)k * n, 4, hipMemcpyDeviceToHost, st));
  // the coefficients, device Montgomery -> canonical, times the 1/m the transforms left out
  DevBuf d_sc;
  BH_TRY_HIP(d_sc.alloc(std::max<size_t>(r->terms, 1) * 32));
  launch_fr_convert(r->coeff.as<uint32_t>(), d_sc.as<uint32_t>(), r->terms, canonical_times(inv(fr_of(r->m))), 1, st);
  BH_TRY_HIP(hipGetLastError());
  BH_TRY_HIP(hipStreamSynchronize(st));
  const bh_srs* l1[3] = {lag[0], lag[2], lag[4]};
  const bh_srs* l2[3] = {lag[1], lag[3], lag[5]};
  bh_srs* ab1[2] = {out[4], out[5]};
  bh_srs* ab2[2] = {nullptr, out[6]};
  bh_status s = product_t<G1Ops>(ctx, r, plan, d_sc.as<uint32_t>(), l1, ab1, out[0], out[2]);
  if (s) return s;
  return product_t<G2Ops>(ctx, r, plan, d_sc.as<uint32_t>(), l2, ab2, out[1], out[3]);
}

}  // namespace bh

extern "C" bh_status bh_srs_fft(bh_ctx* ctx, const bh_srs* in, int inverse, bh_srs** out) {
  if (!ctx || !in || !out || !in->ctx || in->ctx->device != ctx->device) return BH_ERR_INVALID_ARGUMENT;
  std::lock_guard<std::mutex> lk(ctx->mu);
  BH_TRY_HIP(hipSetDevice(ctx->device));
  bh_status s = scratch_check(ctx);
  if (s) return s;
  std::unique_ptr<bh_srs> r(new bh_srs());
  if ((s = group_fft(ctx, in, in->n, inverse, true, r.get()))) return s;
  *out = r.release();
  return BH_OK;
}
