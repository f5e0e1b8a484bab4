// Device codec for vectors of compressed points: the zcash/bls12_381 compressed encodings (G1: x,
// 48 bytes; G2: x.c1 then x.c0, 96 bytes; big-endian, the compression / infinity / sort flags in the
// top three bits of byte 0) to and from the packed device form a bh_srs holds, one lane per point.
//
//   k_points_decompress<C>  the record at raw + i * stride + offset (a device copy of the caller's
//                           bytes, read in place), decoded as verify.cpp's from_compressed and the
//                           proof kernels (proofs_dev.hip) decode one point:
//                             1. compression flag clear                          -> invalid
//                             2. infinity flag set: the sort flag clear and every other bit zero
//                                -> the identity (the all-zero device record), anything else invalid
//                             3. a coordinate >= p (G2: c1 under the flags, and c0) -> invalid
//                             4. x^3 + b not a square                            -> invalid
//                             5. the root whose lex_largest equals the sort flag
//                           and stored as k_points_to_dev (api.hip) stores the same point: fully
//                           reduced Montgomery words.  An invalid lane stores the group's generator,
//                           so that the subgroup kernel and anything later never reads garbage.  One
//                           status word per point: PT_OK, PT_INVALID or PT_IDENTITY.
//   k_points_compress<C>    a device-form point -> its record at out + i * stride + offset: canonical
//                           x written big-endian by the kernel, the compression flag, the sort flag
//                           = lex_largest(y).  The all-zero record of an identity comes out as a
//                           plain x = 0 record; the host writes the infinity encoding over the few
//                           of them (bh_srs::identity_idx) after the copy back.
//
//
// And for the uncompressed encodings (G1: x, y, 96 bytes; G2: x.c1, x.c0, y.c1, y.c0, 192 bytes; the
// flags in the top three bits of byte 0 only), whose record is exactly the size of the device record:
//
//   k_points_from_wire<C>   the record at raw + i * stride + offset, decoded as api.hip's host parser
//                           and k_points_to_dev decode it, in this order:
//                             1. compression flag or sort flag set               -> invalid
//                             2. infinity flag set: every other bit zero -> the identity (the all-zero
//                                device record), anything else invalid
//                             3. a component >= p (all 384 bits of every slot but the first are
//                                value bits)                                     -> invalid
//                             4. only when asked: y^2 != x^3 + b                 -> off the curve (a
//                                record whose components are all zero is skipped, as the parent's
//                                kernel skips it)
//                           The lane reads its whole record before it stores, so raw may be the
//                           output vector itself (a contiguous vector is decoded in place).  One
//                           status word per point: PT_OK, PT_INVALID, PT_IDENTITY or PT_OFF_CURVE; a
//                           failed lane stores the generator.
//   k_points_to_wire<C>     a device-form point -> its canonical components big-endian in wire order,
//                           flags clear.  The host writes 40 00 ... over the identities afterwards.
//
// The subgroup test of a checked decode is api.hip's k_subgroup_check on the decoded vector.  The
// host does no per-point arithmetic on any path: it scans the status words and patches identities.
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <memory>

#include "group_host.h"
#include "point_codec.cuh"
#include "point_codec.h"
#include "r1cs.h"

using namespace bh;

namespace bh {

namespace {

enum : uint32_t { PT_OK = 0, PT_INVALID = 1, PT_IDENTITY = 2, PT_OFF_CURVE = 3 };

struct DecompressArgs {
  const uint32_t* raw;       // records at raw + i * stride_w + offset_w (words)
  size_t stride_w, offset_w, n;
  uint32_t* pts;             // n packed affine records
  uint32_t* status;          // n words
  uint32_t gen[48];          // the generator's canonical coordinates (G::canonical_words)
};

// canonical packed words of one field element (12, or c0 then c1) -> fully reduced Montgomery
template <class F>
__device__ __forceinline__ typename F::T mont_from_words(const uint32_t* w) {
  if constexpr (F::PACKED_WORDS == 12) return fe_reduce_full<FpCfg>(to_mont(fe_unpack<FpCfg>(w)));
  else return F::reduce(DFp2{to_mont(fe_unpack<FpCfg>(w)), to_mont(fe_unpack<FpCfg>(w + 12))});
}

template <class C>
__global__ void __launch_bounds__(64) k_points_decompress(DecompressArgs A) {
  using F = typename FieldOf<C>::F;
  constexpr int PW = F::PACKED_WORDS;
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= A.n) return;
  const uint32_t* src = A.raw + i * A.stride_w + A.offset_w;
  uint32_t w[12];
  const uint32_t flags = ld_coordinate(src, true, w);
  uint32_t nz = 0;  // every bit of the record but the flags
#pragma unroll
  for (int l = 0; l < 12; l++) nz |= w[l];
  bool in_range;
  typename F::T x, y;
  if constexpr (PW == 12) {
    const DFp xc = fe_unpack<FpCfg>(w);
    in_range = !fe_geq_p(xc);
    x = to_mont(xc);  // a value >= p still gives a defined product (the lane has failed)
  } else {
    // wire order: c1 (with the flag bits), then c0 (all 384 bits are value bits)
    const DFp c1 = fe_unpack<FpCfg>(w);
    (void)ld_coordinate(src + 12, false, w);
#pragma unroll
    for (int l = 0; l < 12; l++) nz |= w[l];
    const DFp c0 = fe_unpack<FpCfg>(w);
    in_range = !fe_geq_p(c1) && !fe_geq_p(c0);
    x = DFp2{to_mont(c0), to_mont(c1)};
  }
  const bool compressed = (flags & 4u) != 0, infinity = (flags & 2u) != 0, sort = (flags & 1u) != 0;
  const bool identity = compressed && infinity && !sort && !nz;
  bool ok = compressed && !infinity && in_range;
  ok = field_sqrt(curve_rhs(x), &y) && ok;
  x = F::reduce(x);
  y = F::reduce(y);
  if (lex_largest(y) != sort) y = F::neg_canonical(y);
  if (!ok) {
    x = mont_from_words<F>(A.gen);
    y = mont_from_words<F>(A.gen + PW);
  }
  uint32_t* out = A.pts + i * 2 * PW;
  if (identity) {
#pragma unroll
    for (int l = 0; l < 2 * PW; l++) out[l] = 0u;
  } else {
    F::pack(x, out);
    F::pack(y, out + PW);
  }
  A.status[i] = identity ? PT_IDENTITY : ok ? PT_OK : PT_INVALID;
}

struct CompressArgs {
  const uint32_t* pts;  // n packed affine records
  size_t n;
  uint32_t* out;        // records at out + i * stride_w + offset_w (words)
  size_t stride_w, offset_w;
};

// one canonical coordinate as 48 big-endian bytes at a word-aligned address, `top` or-ed into the
// first byte's flag bits
__device__ __forceinline__ void st_coordinate(const DFp& c, uint32_t top, uint32_t* dst) {
  uint32_t w[12];
  fe_pack<FpCfg>(c, w);
  w[11] |= top;
#pragma unroll
  for (int l = 0; l < 12; l++) dst[l] = __builtin_bswap32(w[11 - l]);
}

template <class C>
__global__ void __launch_bounds__(64) k_points_compress(CompressArgs A) {
  using F = typename FieldOf<C>::F;
  constexpr int PW = F::PACKED_WORDS;
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= A.n) return;
  const uint32_t* p = A.pts + i * 2 * PW;
  const typename F::T x = F::unpack(p), y = F::unpack(p + PW);
  const uint32_t top = 0x80000000u | (lex_largest(y) ? 0x20000000u : 0u);
  uint32_t* dst = A.out + i * A.stride_w + A.offset_w;
  if constexpr (PW == 12) {
    st_coordinate(to_canonical(x), top, dst);
  } else {
    st_coordinate(to_canonical(x.c1), top, dst);
    st_coordinate(to_canonical(x.c0), 0u, dst + 12);
  }
}

struct FromWireArgs {
  const uint32_t* raw;  // records at raw + i * stride_w + offset_w (words); may alias pts
  size_t stride_w, offset_w, n;
  uint32_t* pts;        // n packed affine records
  uint32_t* status;     // n words
  int check;            // the curve equation
  uint32_t gen[48];     // the generator's canonical coordinates (G::canonical_words)
};

template <class C>
__global__ void __launch_bounds__(64) k_points_from_wire(FromWireArgs A) {
  using F = typename FieldOf<C>::F;
  constexpr int PW = F::PACKED_WORDS, NC = 2 * PW / 12;
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= A.n) return;
  const uint32_t* src = A.raw + i * A.stride_w + A.offset_w;
  uint32_t nz = 0;
  bool in_range = true;
  // wire slot k (the flags masked off slot 0) -> the component, fully reduced Montgomery.  A value >= p
  // (below 2^384 < 10p) still gives a defined product: the lane has failed.
  auto slot = [&](int k) {
    uint32_t w[12];
    (void)ld_coordinate(src + 12 * k, k == 0, w);
#pragma unroll
    for (int l = 0; l < 12; l++) nz |= w[l];
    const DFp v = fe_unpack<FpCfg>(w);
    in_range = in_range && !fe_geq_p(v);
    return fe_reduce_full<FpCfg>(to_mont(v));
  };
  const uint32_t flags = __builtin_bswap32(src[0]) >> 29;
  typename F::T x, y;  // on the wire c1 comes before c0 (host_arith.h's wire_component)
  if constexpr (NC == 2) {
    x = slot(0);
    y = slot(1);
  } else {
    x.c1 = slot(0);
    x.c0 = slot(1);
    y.c1 = slot(2);
    y.c0 = slot(3);
  }
  const bool identity = flags == 2u && !nz;
  bool ok = flags == 0u && in_range;
  bool on_curve = true;
  // the all-zero record is skipped, as k_points_to_dev (api.hip) skips it.  y^2 < 2p, x^3 + b < 6p
  // per component: the difference is < 10p, below is_zero's 128p
  if (A.check && nz) on_curve = F::is_zero(F::template sub<8>(F::sqr(y), curve_rhs(x)));
  uint32_t* out = A.pts + i * 2 * PW;  // every load of the record is above
  if (identity) {
#pragma unroll
    for (int l = 0; l < 2 * PW; l++) out[l] = 0u;
  } else if (ok && on_curve) {
    F::pack(x, out);
    F::pack(y, out + PW);
  } else {
    F::pack(mont_from_words<F>(A.gen), out);
    F::pack(mont_from_words<F>(A.gen + PW), out + PW);
  }
  A.status[i] = identity ? PT_IDENTITY : !ok ? PT_INVALID : !on_curve ? PT_OFF_CURVE : PT_OK;
}

template <class C>
__global__ void __launch_bounds__(64) k_points_to_wire(CompressArgs A) {
  using F = typename FieldOf<C>::F;
  constexpr int PW = F::PACKED_WORDS, NC = 2 * PW / 12;
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= A.n) return;
  const uint32_t* p = A.pts + i * 2 * PW;
  uint32_t* dst = A.out + i * A.stride_w + A.offset_w;
  // wire slot k holds component k (G1: x, y) or k ^ 1 (G2: c1 before c0), host_arith.h's wire_component
#pragma unroll
  for (int k = 0; k < NC; k++)
    st_coordinate(to_canonical(fe_reduce_full<FpCfg>(fe_unpack<FpCfg>(p + 12 * (NC == 2 ? k : (k ^ 1))))), 0u,
                  dst + 12 * k);
}

inline unsigned nb64(size_t n) { return (unsigned)((n + 63) / 64); }

constexpr size_t CODEC_MAX = (size_t)1 << 32;  // lanes of 64 stay within a 32-bit grid

bool word_aligned(const void* p, size_t stride, size_t offset) {
  return (uintptr_t)p % 4 == 0 && stride % 4 == 0 && offset % 4 == 0;
}

}  // namespace

void point_codec_kernels(std::vector<KernInfo>& v) {
  v.push_back({"k_points_decompress<G1>", (const void*)k_points_decompress<G1Ops>, 64, 0});
  v.push_back({"k_points_decompress<G2>", (const void*)k_points_decompress<G2Ops>, 64, 0});
  v.push_back({"k_points_compress<G1>", (const void*)k_points_compress<G1Ops>, 64, 0});
  v.push_back({"k_points_compress<G2>", (const void*)k_points_compress<G2Ops>, 64, 0});
  v.push_back({"k_points_from_wire<G1>", (const void*)k_points_from_wire<G1Ops>, 64, 0});
  v.push_back({"k_points_from_wire<G2>", (const void*)k_points_from_wire<G2Ops>, 64, 0});
  v.push_back({"k_points_to_wire<G1>", (const void*)k_points_to_wire<G1Ops>, 64, 0});
  v.push_back({"k_points_to_wire<G2>", (const void*)k_points_to_wire<G2Ops>, 64, 0});
}

bh_status points_decompress_device(bh_ctx* ctx, int group, const uint8_t* d_raw, size_t stride, size_t offset,
                                   size_t n, int checked, bool reject_identity, bh_srs* out) {
  if (n > CODEC_MAX || !word_aligned(d_raw, stride, offset)) return BH_ERR_INVALID_ARGUMENT;
  return with_group(group, [&](auto g) -> bh_status {
    using G = decltype(g);
    out->ctx = ctx;
    out->group = group;
    out->n = n;
    out->identity_idx.clear();
    BH_TRY_HIP(out->pts.alloc(std::max<size_t>(n, 1) * G::WORDS * 4));
    if (!n) return BH_OK;
    DevBuf st;  // n status words, then the subgroup kernel's word
    BH_TRY_HIP(st.alloc((n + 1) * 4));
    BH_TRY_HIP(hipMemsetAsync(st.as<uint32_t>() + n, 0, 4, ctx->stream));
    DecompressArgs A;
    A.raw = reinterpret_cast<const uint32_t*>(d_raw);
    A.stride_w = stride / 4;
    A.offset_w = offset / 4;
    A.n = n;
    A.pts = out->pts.as<uint32_t>();
    A.status = st.as<uint32_t>();
    memset(A.gen, 0, sizeof A.gen);
    if constexpr (G::ID == BH_G1) G::canonical_words(jac_to_affine(crs_g1_gen()), A.gen);
    else G::canonical_words(jac_to_affine(crs_g2_gen()), A.gen);
    hipLaunchKernelGGL(k_points_decompress<typename G::Ops>, dim3(nb64(n)), dim3(64), 0, ctx->stream, A);
    BH_TRY_HIP(hipGetLastError());
    if (checked)
      if (bh_status s = subgroup_check_enqueue(ctx, group, A.pts, n, A.status + n)) return s;
    std::vector<uint32_t> h(n + 1);
    BH_TRY_HIP(hipMemcpyAsync(h.data(), st.p, (n + 1) * 4, hipMemcpyDeviceToHost, ctx->stream));
    BH_TRY_HIP(hipStreamSynchronize(ctx->stream));  // st is freed on return
    for (size_t i = 0; i < n; i++) {
      if (h[i] == PT_INVALID || (h[i] == PT_IDENTITY && reject_identity)) return BH_ERR_INVALID_ENCODING;
      if (h[i] == PT_IDENTITY) out->identity_idx.push_back(i);
    }
    return h[n] ? BH_ERR_NOT_IN_SUBGROUP : BH_OK;
  });
}

bh_status srs_from_compressed(bh_ctx* ctx, int group, const uint8_t* bytes, size_t n, int checked,
                              bool reject_identity, bh_srs* out) {
  if (n > CODEC_MAX) return BH_ERR_INVALID_ARGUMENT;
  const size_t rec = compressed_bytes(group);
  DevBuf raw;
  BH_TRY_HIP(raw.alloc(std::max<size_t>(n, 1) * rec));
  if (n) BH_TRY_HIP(hipMemcpyAsync(raw.p, bytes, n * rec, hipMemcpyHostToDevice, ctx->stream));
  // returns synchronised: raw is freed on return
  return points_decompress_device(ctx, group, raw.as<uint8_t>(), rec, 0, n, checked, reject_identity, out);
}

bh_status points_compress_device(bh_ctx* ctx, const bh_srs* s, size_t first, size_t n, uint8_t* d_out, size_t stride,
                                 size_t offset) {
  if (first > s->n || n > s->n - first || n > CODEC_MAX || !word_aligned(d_out, stride, offset))
    return BH_ERR_INVALID_ARGUMENT;
  if (!n) return BH_OK;
  return with_group(s->group, [&](auto g) -> bh_status {
    using G = decltype(g);
    CompressArgs A;
    A.pts = s->pts.as<uint32_t>() + first * G::WORDS;
    A.n = n;
    A.out = reinterpret_cast<uint32_t*>(d_out);
    A.stride_w = stride / 4;
    A.offset_w = offset / 4;
    hipLaunchKernelGGL(k_points_compress<typename G::Ops>, dim3(nb64(n)), dim3(64), 0, ctx->stream, A);
    BH_TRY_HIP(hipGetLastError());
    return BH_OK;
  });
}

void points_compress_patch(const bh_srs* s, size_t first, size_t n, uint8_t* h_out, size_t stride, size_t offset) {
  const size_t rec = compressed_bytes(s->group);
  for (size_t i : s->identity_idx)
    if (i >= first && i - first < n) {
      uint8_t* b = h_out + (i - first) * stride + offset;
      memset(b, 0, rec);
      b[0] = 0xC0;
    }
}

bh_status srs_to_compressed(bh_ctx* ctx, const bh_srs* s, size_t first, size_t n, uint8_t* out) {
  if (!n) return BH_OK;
  const size_t rec = compressed_bytes(s->group);
  DevBuf d;
  BH_TRY_HIP(d.alloc(n * rec));
  if (bh_status st = points_compress_device(ctx, s, first, n, d.as<uint8_t>(), rec, 0)) return st;
  BH_TRY_HIP(hipMemcpyAsync(out, d.p, n * rec, hipMemcpyDeviceToHost, ctx->stream));
  BH_TRY_HIP(hipStreamSynchronize(ctx->stream));  // d is freed on return
  points_compress_patch(s, first, n, out, rec, 0);
  return BH_OK;
}

// ---------------------------------------------------------------- the uncompressed encodings
namespace {
thread_local int g_codec_device = 0;
}

bool point_codec_host() {
  const char* env = getenv("BH_POINT_CODEC_HOST");
  return env && env[0] == '1';
}
void point_codec_note(bool device) { g_codec_device = device ? 1 : 0; }

bh_status points_from_wire_device(bh_ctx* ctx, int group, const uint8_t* d_raw, size_t stride, size_t offset, size_t n,
                                  int checked, bool reject_identity, bh_srs* out) {
  if (n > CODEC_MAX || !word_aligned(d_raw, stride, offset)) return BH_ERR_INVALID_ARGUMENT;
  return with_group(group, [&](auto g) -> bh_status {
    using G = decltype(g);
    out->ctx = ctx;
    out->group = group;
    out->n = n;
    out->identity_idx.clear();
    if (d_raw != out->pts.p) BH_TRY_HIP(out->pts.alloc(std::max<size_t>(n, 1) * G::WORDS * 4));
    if (!n) return BH_OK;
    DevBuf st;  // n status words, then the subgroup kernel's word
    BH_TRY_HIP(st.alloc((n + 1) * 4));
    BH_TRY_HIP(hipMemsetAsync(st.as<uint32_t>() + n, 0, 4, ctx->stream));
    FromWireArgs A;
    A.raw = reinterpret_cast<const uint32_t*>(d_raw);
    A.stride_w = stride / 4;
    A.offset_w = offset / 4;
    A.n = n;
    A.pts = out->pts.as<uint32_t>();
    A.status = st.as<uint32_t>();
    A.check = checked ? 1 : 0;
    memset(A.gen, 0, sizeof A.gen);
    if constexpr (G::ID == BH_G1) G::canonical_words(jac_to_affine(crs_g1_gen()), A.gen);
    else G::canonical_words(jac_to_affine(crs_g2_gen()), A.gen);
    hipLaunchKernelGGL(k_points_from_wire<typename G::Ops>, dim3(nb64(n)), dim3(64), 0, ctx->stream, A);
    BH_TRY_HIP(hipGetLastError());
    if (checked)
      if (bh_status s = subgroup_check_enqueue(ctx, group, A.pts, n, A.status + n)) return s;
    std::vector<uint32_t> h(n + 1);
    BH_TRY_HIP(hipMemcpyAsync(h.data(), st.p, (n + 1) * 4, hipMemcpyDeviceToHost, ctx->stream));
    BH_TRY_HIP(hipStreamSynchronize(ctx->stream));  // st is freed on return
    bool off_curve = false;
    for (size_t i = 0; i < n; i++) {
      if (h[i] == PT_INVALID || (h[i] == PT_IDENTITY && reject_identity)) return BH_ERR_INVALID_ENCODING;
      if (h[i] == PT_IDENTITY) out->identity_idx.push_back(i);
      off_curve = off_curve || h[i] == PT_OFF_CURVE;
    }
    if (off_curve) return BH_ERR_NOT_ON_CURVE;
    return h[n] ? BH_ERR_NOT_IN_SUBGROUP : BH_OK;
  });
}

bh_status srs_from_wire(bh_ctx* ctx, int group, const uint8_t* bytes, size_t n, int checked, bool reject_identity,
                        bh_srs* out) {
  if (n > CODEC_MAX) return BH_ERR_INVALID_ARGUMENT;
  const size_t rec = 2 * compressed_bytes(group);
  // the wire record is the size of the device record: the bytes land in the vector and are decoded there
  BH_TRY_HIP(out->pts.alloc(std::max<size_t>(n, 1) * rec));
  if (n) BH_TRY_HIP(hipMemcpyAsync(out->pts.p, bytes, n * rec, hipMemcpyHostToDevice, ctx->stream));
  return points_from_wire_device(ctx, group, out->pts.as<uint8_t>(), rec, 0, n, checked, reject_identity, out);
}

bh_status points_to_wire_device(bh_ctx* ctx, const bh_srs* s, size_t first, size_t n, uint8_t* d_out, size_t stride,
                                size_t offset) {
  if (first > s->n || n > s->n - first || n > CODEC_MAX || !word_aligned(d_out, stride, offset))
    return BH_ERR_INVALID_ARGUMENT;
  if (!n) return BH_OK;
  return with_group(s->group, [&](auto g) -> bh_status {
    using G = decltype(g);
    CompressArgs A;
    A.pts = s->pts.as<uint32_t>() + first * G::WORDS;
    A.n = n;
    A.out = reinterpret_cast<uint32_t*>(d_out);
    A.stride_w = stride / 4;
    A.offset_w = offset / 4;
    hipLaunchKernelGGL(k_points_to_wire<typename G::Ops>, dim3(nb64(n)), dim3(64), 0, ctx->stream, A);
    BH_TRY_HIP(hipGetLastError());
    return BH_OK;
  });
}

void points_wire_patch(const bh_srs* s, size_t first, size_t n, uint8_t* h_out, size_t stride, size_t offset) {
  const size_t rec = 2 * compressed_bytes(s->group);
  for (size_t i : s->identity_idx)
    if (i >= first && i - first < n) {
      uint8_t* b = h_out + (i - first) * stride + offset;
      memset(b, 0, rec);
      b[0] = 0x40;
    }
}

bh_status srs_to_wire(bh_ctx* ctx, const bh_srs* s, size_t first, size_t n, uint8_t* out) {
  if (!n) return BH_OK;
  const size_t rec = 2 * compressed_bytes(s->group);
  DevBuf d;
  BH_TRY_HIP(d.alloc(n * rec));
  if (bh_status st = points_to_wire_device(ctx, s, first, n, d.as<uint8_t>(), rec, 0)) return st;
  BH_TRY_HIP(hipMemcpyAsync(out, d.p, n * rec, hipMemcpyDeviceToHost, ctx->stream));
  BH_TRY_HIP(hipStreamSynchronize(ctx->stream));  // d is freed on return
  points_wire_patch(s, first, n, out, rec, 0);
  return BH_OK;
}

}  // namespace bh

extern "C" {

bh_status bh_srs_upload_compressed(bh_ctx* ctx, int group, const uint8_t* bytes, size_t n, int checked, bh_srs** out) {
  if (!ctx || !out || (group != BH_G1 && group != BH_G2) || (n && !bytes)) return BH_ERR_INVALID_ARGUMENT;
  std::lock_guard<std::mutex> lk(ctx->mu);
  BH_TRY_HIP(hipSetDevice(ctx->device));
  if (bh_status sc = scratch_check(ctx)) return sc;
  std::unique_ptr<bh_srs> s(new bh_srs());
  if (bh_status st = srs_from_compressed(ctx, group, bytes, n, checked, false, s.get())) return st;
  *out = s.release();
  return BH_OK;
}

bh_status bh_srs_read_compressed(const bh_srs* srs, size_t first, size_t n, uint8_t* out) {
  if (!srs || !srs->ctx || (n && !out) || first > srs->n || n > srs->n - first) return BH_ERR_INVALID_ARGUMENT;
  if (!n) return BH_OK;
  bh_ctx* ctx = srs->ctx;
  std::lock_guard<std::mutex> lk(ctx->mu);
  BH_TRY_HIP(hipSetDevice(ctx->device));
  return srs_to_compressed(ctx, srs, first, n, out);
}

int bh_srs_last_codec_device(void) { return g_codec_device; }

}  // extern "C"
