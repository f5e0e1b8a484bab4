// The per-proof verifier's stages between Proof::read and the Miller loops (verify_each.h).
//
//   k_each_accumulate  one lane per proof: acc_j = ic_0 + sum_i x_ji ic_i (verifier.rs:33-40).  All
//                      lanes share the bases, so the sum is interleaved (Straus): per 4-bit window
//                      four doublings of the ONE accumulator and one mixed addition per input, its
//                      point read from a table of 1 ic_i .. 8 ic_i that the call builds once
//                      (varbase_multiples_table).  Signed digits as in k_varbase_mul_win: with the
//                      bias B = 0x88..8 added to a scalar by the host, digit_w = nibble_w(x + B) - 8
//                      in [-8, 7]; x < r keeps x + B below 2^256.  A zero scalar has every digit
//                      zero and costs no addition.  CurveOps::madd is complete (an accumulator that
//                      is the identity, equal or opposite to the table point), so any inputs give the
//                      group's answer, the identity included.
//   k_each_normalize   acc_j -> -acc_j as the packed affine record of pair 3 j + 1, one inversion
//                      per CHUNK points like k_normalize; an identity takes part in the prefix
//                      products as one and is stored as the all-zero record.
//   k_each_pairs       pairs 3 j and 3 j + 2 and the twist points of all three.
#include <string.h>

#include <algorithm>

#include "varbase.h"
#include "verify_each.h"

using namespace bh;

namespace bh {

namespace {

using C = G1Ops;
using F = G1F;
using T = typename F::T;
constexpr int PW = F::PACKED_WORDS;
static_assert(PW == 12 && G1Host::WORDS == 24 && G2Host::WORDS == 48, "the record layout below");

__device__ __forceinline__ typename C::A ld_affine(const uint32_t* base, size_t i) {
  typename C::A a;
  a.x = F::unpack(base + i * 2 * PW);
  a.y = F::unpack(base + i * 2 * PW + PW);
  return a;
}

struct EachAccArgs {
  const uint32_t* table;    // record d ni + i: (d + 1) ic_(i + 1), d < 8
  const uint32_t* ic0;      // one record
  const uint32_t* scalars;  // k ni biased scalars, 8 LE words each, proof-major
  size_t k, ni;
  typename C::P* out;
};

__global__ void __launch_bounds__(64) k_each_accumulate(EachAccArgs A) {
  const size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= A.k) return;
  typename C::P acc = C::identity();
#pragma unroll 1
  for (int w = 63; w >= 0; w--) {
    if (w != 63) {
#pragma unroll 1
      for (int t = 0; t < 4; t++) acc = C::dbl(acc);  // the identity stays the identity
    }
#pragma unroll 1
    for (size_t i = 0; i < A.ni; i++) {
      const uint32_t word = A.scalars[(j * A.ni + i) * 8 + (w >> 3)];
      const int d = (int)((word >> (4 * (w & 7))) & 15u) - 8;
      if (d) {
        typename C::A t = ld_affine(A.table, (size_t)((d < 0 ? -d : d) - 1) * A.ni + i);
        if (d < 0) t = C::neg_affine(t);
        acc = C::madd(acc, t);
      }
    }
  }
  A.out[j] = C::madd(acc, ld_affine(A.ic0, 0));
}

// x^(p - 2): crs.hip's fp_inv_ops (a device function cannot be shared between translation units
// built without relocatable device code)
__device__ T fp_inv(const T& x) {
  constexpr uint32_t E[12] = {0xffffaaa9u, 0xb9feffffu, 0xb153ffffu, 0x1eabfffeu, 0xf6b0f624u, 0x6730d2a0u,
                              0xf38512bfu, 0x64774b84u, 0x434bacd7u, 0x4b1ba7b6u, 0x397fe69au, 0x1a0111eau};
  T r = F::one();
#pragma unroll 1
  for (int w = 11; w >= 0; w--) {
#pragma unroll 1
    for (int b = 31; b >= 0; b--) {
      r = F::sqr(r);
      if ((E[w] >> b) & 1u) r = F::mul(r, x);
    }
  }
  return r;
}

// one thread per CHUNK consecutive points; prefix products kept in `scratch`; point i's record at
// g1 + (3 i + 1) * 24.  Bounds as k_normalize: every operand is an XYZZ coordinate (< 128p) or a
// product (< 2p).
template <int CHUNK>
__global__ void __launch_bounds__(64) k_each_normalize(const typename C::P* pts, size_t n, T* scratch, uint32_t* g1) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t i0 = t * CHUNK;
  if (i0 >= n) return;
  const size_t i1 = (i0 + CHUNK < n) ? i0 + CHUNK : n;
  T acc = F::one();
#pragma unroll 1
  for (size_t i = i0; i < i1; i++) {
    const T z = C::is_identity(pts[i]) ? F::one() : F::mul(pts[i].ZZ, pts[i].ZZZ);
    scratch[i] = acc;
    acc = F::mul(acc, z);
  }
  T inv = fp_inv(acc);
#pragma unroll 1
  for (size_t i = i1; i-- > i0;) {
    const typename C::P p = pts[i];
    const bool id = C::is_identity(p);
    const T z = id ? F::one() : F::mul(p.ZZ, p.ZZZ);
    const T zinv = F::mul(inv, scratch[i]);  // 1 / z_i
    inv = F::mul(inv, z);
    // 1/ZZ = ZZZ / z ; 1/ZZZ = ZZ / z
    T x = F::reduce(F::mul(p.X, F::mul(p.ZZZ, zinv)));
    T y = F::neg_canonical(F::reduce(F::mul(p.Y, F::mul(p.ZZ, zinv))));
    if (id) x = y = F::zero();
    uint32_t* rec = g1 + (3 * i + 1) * 24;
    F::pack(x, rec);
    F::pack(y, rec + PW);
  }
}

__global__ void __launch_bounds__(64) k_each_pairs(const uint32_t* a, const uint32_t* b, const uint32_t* c,
                                                   const uint32_t* gd, size_t k, uint32_t* g1, uint32_t* g2) {
  const size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= k) return;
  for (int w = 0; w < 24; w++) g1[3 * j * 24 + w] = a[j * 24 + w];
  for (int w = 0; w < PW; w++) g1[(3 * j + 2) * 24 + w] = c[j * 24 + w];
  // C is never the identity (Proof::read rejects it; a failed slot holds the generator)
  F::pack(F::neg_canonical(F::unpack(c + j * 24 + PW)), g1 + (3 * j + 2) * 24 + PW);
  for (int w = 0; w < 48; w++) {
    g2[3 * j * 48 + w] = b[j * 48 + w];
    g2[(3 * j + 1) * 48 + w] = gd[w];
    g2[(3 * j + 2) * 48 + w] = gd[48 + w];
  }
}

inline unsigned nb64(size_t n) { return (unsigned)((n + 63) / 64); }
constexpr int NORM_CHUNK = 32;

}  // namespace

void verify_each_kernels(std::vector<KernInfo>& v) {
  v.push_back({"k_each_accumulate", (const void*)k_each_accumulate, 64, 0});
  v.push_back({"k_each_normalize", (const void*)k_each_normalize<NORM_CHUNK>, 64, 0});
  v.push_back({"k_each_pairs", (const void*)k_each_pairs, 64, 0});
}

bh_status verify_each_pairs(bh_ctx* ctx, const bh_srs& a, const bh_srs& b, const bh_srs& c, const AffinePt<Fp>* ic,
                            size_t n_ic, const AffinePt<Fp2>& gamma, const AffinePt<Fp2>& delta, const uint64_t* inputs,
                            size_t k, DevBuf* g1, DevBuf* g2) {
  if (!n_ic || a.n != k || b.n != k || c.n != k) return BH_ERR_INVALID_ARGUMENT;
  const size_t ni = n_ic - 1;
  BH_TRY_HIP(g1->alloc(std::max<size_t>(3 * k, 1) * 24 * 4));
  BH_TRY_HIP(g2->alloc(std::max<size_t>(3 * k, 1) * 48 * 4));
  if (!k) return BH_OK;
  bh_srs d_ic, d_gd;
  bh_status s = srs_upload_affine(ctx, ic, n_ic, &d_ic);
  if (s) return s;
  const AffinePt<Fp2> gd[2] = {gamma, delta};
  if ((s = srs_upload_affine(ctx, gd, 2, &d_gd))) return s;
  // the table of the inputs' bases ic_1 ..
  DevBuf xyzz, scr, table, sc, acc;
  BH_TRY_HIP(xyzz.alloc(8 * ni * sizeof(typename C::P)));
  BH_TRY_HIP(scr.alloc(std::max(8 * ni, k) * sizeof(T) + 64));
  BH_TRY_HIP(table.alloc(8 * ni * 24 * 4));
  if (ni) BH_TRY_HIP(varbase_multiples_table<C>(d_ic.pts.as<uint32_t>() + 24, ni, xyzz.p, scr.p, table.as<uint32_t>(), ctx->stream));
  // x + B for every input
  std::vector<uint64_t> biased(std::max<size_t>(4 * k * ni, 1));
  for (size_t t = 0; t < k * ni; t++) {
    u128 carry = 0;
    for (int w = 0; w < 4; w++) {
      carry += (u128)inputs[4 * t + w] + 0x8888888888888888ull;
      biased[4 * t + w] = (uint64_t)carry;
      carry >>= 64;
    }
  }
  BH_TRY_HIP(sc.alloc(biased.size() * 8));
  BH_TRY_HIP(acc.alloc(k * sizeof(typename C::P)));
  BH_TRY_HIP(hipMemcpyAsync(sc.p, biased.data(), biased.size() * 8, hipMemcpyHostToDevice, ctx->stream));
  EachAccArgs A;
  A.table = table.as<uint32_t>();
  A.ic0 = d_ic.pts.as<uint32_t>();
  A.scalars = sc.as<uint32_t>();
  A.k = k;
  A.ni = ni;
  A.out = acc.as<typename C::P>();
  hipLaunchKernelGGL(k_each_accumulate, dim3(nb64(k)), dim3(64), 0, ctx->stream, A);
  BH_TRY_HIP(hipGetLastError());
  hipLaunchKernelGGL(k_each_normalize<NORM_CHUNK>, dim3(nb64((k + NORM_CHUNK - 1) / NORM_CHUNK)), dim3(64), 0,
                     ctx->stream, acc.as<typename C::P>(), k, scr.as<T>(), g1->as<uint32_t>());
  BH_TRY_HIP(hipGetLastError());
  hipLaunchKernelGGL(k_each_pairs, dim3(nb64(k)), dim3(64), 0, ctx->stream, a.pts.as<uint32_t>(), b.pts.as<uint32_t>(),
                     c.pts.as<uint32_t>(), d_gd.pts.as<uint32_t>(), k, g1->as<uint32_t>(), g2->as<uint32_t>());
  BH_TRY_HIP(hipGetLastError());
  BH_TRY_HIP(hipStreamSynchronize(ctx->stream));  // the workspace is freed on return
  return BH_OK;
}

}  // namespace bh
