// Device Proof::read: k compressed Groth16 proofs (A 48 bytes, B 96, C 48; groth16/mod.rs:50-103)
// decoded as verify.cpp's from_compressed decodes one point, one lane per point:
//
//   k_proof_sqrt_g1   2k lanes, A and C together: flags, x < p, y = (x^3 + 4)^((p+1)/4), y^2 checked,
//                     the sign flag against lex_largest(y); stores (x, y) in the packed device form
//   k_proof_sqrt_g2   k lanes: the same over Fp2 (wire order c1 then c0, the flag bits on c1 only),
//                     the square root of x^3 + 4(1 + u) by the p = 3 mod 4 method below
//   k_proof_subgroup  [r]P == O per point (api.hip's k_subgroup_check with a status word per point),
//                     a kernel of its own so that the square-root kernels are not sized by the
//                     point formulas' registers; G1 (2k lanes) and G2 (k lanes) in separate launches
//
// Each point has a status word: 0, BH_ERR_INVALID_ENCODING (compression flag clear, infinity flag
// set, a coordinate >= p, x^3 + b not a square -- in that order, as the host) or, from the last
// kernel, BH_ERR_NOT_IN_SUBGROUP.  A lane whose point fails in a square-root kernel stores the
// group's generator, so the subgroup kernel (which skips it) and anything later never reads garbage.
//
// The square roots, the range and sign rules and the coordinate load are point_codec.cuh's, shared
// with the point-vector codec (point_codec.hip).
#include <string.h>

#include <algorithm>
#include <memory>

#include "group_host.h"
#include "point_codec.cuh"
#include "proofs_dev.h"
#include "r1cs.h"

using namespace bh;

namespace bh {

namespace {

// ---------------------------------------------------------------- decode kernels
constexpr uint32_t ST_ENCODING = BH_ERR_INVALID_ENCODING, ST_SUBGROUP = BH_ERR_NOT_IN_SUBGROUP;
constexpr size_t PROOF_WORDS = 48;  // 192 bytes

// the generators' canonical coordinates (G1Host / G2Host::canonical_words)
struct GenWords {
  uint32_t g1[24], g2[48];
};

struct DecodeArgs {
  const uint32_t* proofs;  // k records of PROOF_WORDS words
  size_t k;
  uint32_t *a, *b, *c;              // k packed affine records each (24, 48, 24 words)
  uint32_t *st_a, *st_b, *st_c;     // k status words each
  GenWords gen;
};

// lanes [0, k): A of proof lane; [k, 2k): C of proof lane - k
__global__ void __launch_bounds__(64) k_proof_sqrt_g1(DecodeArgs A) {
  const size_t lane = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (lane >= 2 * A.k) return;
  const bool is_c = lane >= A.k;
  const size_t j = is_c ? lane - A.k : lane;
  uint32_t w[12];
  const uint32_t flags = ld_coordinate(A.proofs + j * PROOF_WORDS + (is_c ? 36 : 0), true, w);
  const DFp xc = fe_unpack<FpCfg>(w);
  bool ok = (flags & 4u) && !(flags & 2u) && !fe_geq_p(xc);
  DFp x = to_mont(xc), y;  // a value >= p still gives a defined product (the lane has failed)
  ok = field_sqrt(curve_rhs(x), &y) && ok;
  x = fe_reduce_full<FpCfg>(x);
  y = fe_reduce_full<FpCfg>(y);
  if (lex_largest(y) != ((flags & 1u) != 0)) y = FpOps::neg_canonical(y);
  if (!ok) {
    x = fe_reduce_full<FpCfg>(to_mont(fe_unpack<FpCfg>(A.gen.g1)));
    y = fe_reduce_full<FpCfg>(to_mont(fe_unpack<FpCfg>(A.gen.g1 + 12)));
  }
  uint32_t* out = (is_c ? A.c : A.a) + j * 24;
  fe_pack<FpCfg>(x, out);
  fe_pack<FpCfg>(y, out + 12);
  (is_c ? A.st_c : A.st_a)[j] = ok ? 0u : ST_ENCODING;
}

__global__ void __launch_bounds__(64) k_proof_sqrt_g2(DecodeArgs A) {
  const size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= A.k) return;
  uint32_t w[12];
  // wire order: c1 (with the flag bits), then c0 (all 384 bits are value bits)
  const uint32_t flags = ld_coordinate(A.proofs + j * PROOF_WORDS + 12, true, w);
  const DFp c1 = fe_unpack<FpCfg>(w);
  (void)ld_coordinate(A.proofs + j * PROOF_WORDS + 24, false, w);
  const DFp c0 = fe_unpack<FpCfg>(w);
  bool ok = (flags & 4u) && !(flags & 2u) && !fe_geq_p(c1) && !fe_geq_p(c0);
  DFp2 x{to_mont(c0), to_mont(c1)}, y;
  ok = field_sqrt(curve_rhs(x), &y) && ok;
  x = F2::reduce(x);
  y = F2::reduce(y);
  if (lex_largest(y) != ((flags & 1u) != 0)) y = F2::neg_canonical(y);
  if (!ok) {
    x = F2::reduce(DFp2{to_mont(fe_unpack<FpCfg>(A.gen.g2)), to_mont(fe_unpack<FpCfg>(A.gen.g2 + 12))});
    y = F2::reduce(DFp2{to_mont(fe_unpack<FpCfg>(A.gen.g2 + 24)), to_mont(fe_unpack<FpCfg>(A.gen.g2 + 36))});
  }
  uint32_t* out = A.b + j * 48;
  F2::pack(x, out);
  F2::pack(y, out + 24);
  A.st_b[j] = ok ? 0u : ST_ENCODING;
}

// [r]P == O for the n0 points of pts0 and then the n1 points of pts1 (device form, no identity
// among them), one status word each: a point whose word is already non-zero is skipped, one outside
// the subgroup gets BH_ERR_NOT_IN_SUBGROUP.  The double-and-add of k_subgroup_check (api.hip).
template <class C>
__global__ void __launch_bounds__(64) k_proof_subgroup(const uint32_t* pts0, uint32_t* st0, size_t n0,
                                                       const uint32_t* pts1, uint32_t* st1, size_t n1) {
  using F = typename FieldOf<C>::F;
  constexpr int PW = F::PACKED_WORDS;
  const size_t lane = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (lane >= n0 + n1) return;
  const bool second = lane >= n0;
  const size_t i = second ? lane - n0 : lane;
  uint32_t* st = (second ? st1 : st0) + i;
  if (*st) return;
  const uint32_t* p = (second ? pts1 : pts0) + i * 2 * PW;
  typename C::A a;
  a.x = F::unpack(p);
  a.y = F::unpack(p + PW);
  // r = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001, LE words
  constexpr uint32_t R[8] = {0x00000001u, 0xffffffffu, 0xfffe5bfeu, 0x53bda402u,
                             0x09a1d805u, 0x3339d808u, 0x299d7d48u, 0x73eda753u};
  typename C::P acc = C::from_affine(a);
#pragma unroll 1
  for (int bit = 253; bit >= 0; bit--) {  // bit 254 is the leading one
    acc = C::dbl(acc);
    if ((R[bit >> 5] >> (bit & 31)) & 1u) acc = C::madd(acc, a);
  }
  if (!C::is_identity(acc)) *st = ST_SUBGROUP;
}

// ---------------------------------------------------------------- self-test kernel
// in: n canonical values (12 words, or c0 then c1); out per value: the is-square flag, then the
// canonical root field_sqrt left
template <class F>
__global__ void __launch_bounds__(64) k_selftest_field_sqrt(const uint32_t* in, uint32_t* out, size_t n) {
  constexpr int PW = F::PACKED_WORDS;
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  typename F::T a, root;
  if constexpr (PW == 12) a = to_mont(fe_unpack<FpCfg>(in + t * PW));
  else a = DFp2{to_mont(fe_unpack<FpCfg>(in + t * PW)), to_mont(fe_unpack<FpCfg>(in + t * PW + 12))};
  const bool sq = field_sqrt(a, &root);
  root = F::reduce(root);
  uint32_t* o = out + t * (PW + 1);
  o[0] = sq ? 1u : 0u;
  if constexpr (PW == 12) fe_pack<FpCfg>(to_canonical(root), o + 1);
  else F::pack(DFp2{to_canonical(root.c0), to_canonical(root.c1)}, o + 1);
}

inline unsigned nb64(size_t n) { return (unsigned)((n + 63) / 64); }

void init_vector(bh_ctx* ctx, int group, size_t n, bh_srs* v) {
  v->ctx = ctx;
  v->group = group;
  v->n = n;
  v->identity_idx.clear();
}

constexpr size_t PROOFS_MAX = (size_t)1 << 30;  // 2k lanes of 64 stay within a 32-bit grid

}  // namespace

void proofs_kernels(std::vector<KernInfo>& v) {
  v.push_back({"k_proof_sqrt_g1", (const void*)k_proof_sqrt_g1, 64, 0});
  v.push_back({"k_proof_sqrt_g2", (const void*)k_proof_sqrt_g2, 64, 0});
  v.push_back({"k_proof_subgroup<G1>", (const void*)k_proof_subgroup<G1Ops>, 64, 0});
  v.push_back({"k_proof_subgroup<G2>", (const void*)k_proof_subgroup<G2Ops>, 64, 0});
}

bh_status proofs_decode_device(bh_ctx* ctx, const uint8_t* proofs, size_t k, std::vector<uint32_t>* status, bh_srs* a,
                               bh_srs* b, bh_srs* c) {
  if (k > PROOFS_MAX) return BH_ERR_INVALID_ARGUMENT;
  init_vector(ctx, BH_G1, k, a);
  init_vector(ctx, BH_G2, k, b);
  init_vector(ctx, BH_G1, k, c);
  BH_TRY_HIP(a->pts.alloc(std::max<size_t>(k, 1) * G1Host::WORDS * 4));
  BH_TRY_HIP(b->pts.alloc(std::max<size_t>(k, 1) * G2Host::WORDS * 4));
  BH_TRY_HIP(c->pts.alloc(std::max<size_t>(k, 1) * G1Host::WORDS * 4));
  status->assign(k, 0);
  if (!k) return BH_OK;
  DevBuf raw, st;
  BH_TRY_HIP(raw.alloc(k * PROOF_WORDS * 4));
  BH_TRY_HIP(st.alloc(3 * k * 4));
  DecodeArgs A;
  A.proofs = raw.as<uint32_t>();
  A.k = k;
  A.a = a->pts.as<uint32_t>();
  A.b = b->pts.as<uint32_t>();
  A.c = c->pts.as<uint32_t>();
  A.st_a = st.as<uint32_t>();
  A.st_b = A.st_a + k;
  A.st_c = A.st_b + k;
  G1Host::canonical_words(jac_to_affine(crs_g1_gen()), A.gen.g1);
  G2Host::canonical_words(jac_to_affine(crs_g2_gen()), A.gen.g2);
  BH_TRY_HIP(hipMemcpyAsync(raw.p, proofs, k * PROOF_WORDS * 4, hipMemcpyHostToDevice, ctx->stream));
  hipLaunchKernelGGL(k_proof_sqrt_g1, dim3(nb64(2 * k)), dim3(64), 0, ctx->stream, A);
  BH_TRY_HIP(hipGetLastError());
  hipLaunchKernelGGL(k_proof_sqrt_g2, dim3(nb64(k)), dim3(64), 0, ctx->stream, A);
  BH_TRY_HIP(hipGetLastError());
  hipLaunchKernelGGL(k_proof_subgroup<G1Ops>, dim3(nb64(2 * k)), dim3(64), 0, ctx->stream, A.a, A.st_a, k, A.c, A.st_c,
                     k);
  BH_TRY_HIP(hipGetLastError());
  hipLaunchKernelGGL(k_proof_subgroup<G2Ops>, dim3(nb64(k)), dim3(64), 0, ctx->stream, A.b, A.st_b, k,
                     (const uint32_t*)nullptr, (uint32_t*)nullptr, (size_t)0);
  BH_TRY_HIP(hipGetLastError());
  std::vector<uint32_t> h(3 * k);
  BH_TRY_HIP(hipMemcpyAsync(h.data(), st.p, 3 * k * 4, hipMemcpyDeviceToHost, ctx->stream));
  BH_TRY_HIP(hipStreamSynchronize(ctx->stream));  // raw and st are freed on return
  for (size_t j = 0; j < k; j++) (*status)[j] = h[j] ? h[j] : h[k + j] ? h[k + j] : h[2 * k + j];
  return BH_OK;
}

}  // namespace bh

extern "C" {

bh_status bh_proofs_decode(bh_ctx* ctx, const uint8_t* proofs, size_t k, uint32_t* status, bh_srs** a, bh_srs** b,
                           bh_srs** c) {
  if (!ctx || !a || !b || !c || (k && !proofs)) return BH_ERR_INVALID_ARGUMENT;
  *a = *b = *c = nullptr;
  std::lock_guard<std::mutex> lk(ctx->mu);
  BH_TRY_HIP(hipSetDevice(ctx->device));
  bh_status s = scratch_check(ctx);
  if (s) return s;
  std::unique_ptr<bh_srs> va(new bh_srs()), vb(new bh_srs()), vc(new bh_srs());
  std::vector<uint32_t> st;
  if ((s = proofs_decode_device(ctx, proofs, k, &st, va.get(), vb.get(), vc.get()))) return s;
  if (status)
    for (size_t j = 0; j < k; j++) status[j] = st[j];
  for (size_t j = 0; j < k; j++)
    if (st[j]) return (bh_status)st[j];  // the lowest failing proof; no vector is handed out
  *a = va.release();
  *b = vb.release();
  *c = vc.release();
  return BH_OK;
}

bh_status bh_selftest_field_sqrt(int device, int field, const uint32_t* in, size_t n, uint32_t* out) {
  if ((field != 1 && field != 2) || (n && (!in || !out)) || n > (1u << 20)) return BH_ERR_INVALID_ARGUMENT;
  if (!n) return BH_OK;
  for (size_t i = 0; i < n * (size_t)field; i++) {  // canonical values only
    uint64_t raw[6];
    memcpy(raw, in + 12 * i, 48);
    if (geq_p<6>(raw)) return BH_ERR_INVALID_ARGUMENT;
  }
  BH_TRY_HIP(hipSetDevice(device));
  const size_t pw = 12 * (size_t)field, in_b = n * pw * 4, out_b = n * (pw + 1) * 4;
  DevBuf din, dout;
  BH_TRY_HIP(din.alloc(in_b));
  BH_TRY_HIP(dout.alloc(out_b));
  BH_TRY_HIP(hipMemcpy(din.p, in, in_b, hipMemcpyHostToDevice));
  if (field == 1)
    hipLaunchKernelGGL(k_selftest_field_sqrt<FpOps>, dim3(nb64(n)), dim3(64), 0, nullptr, din.as<uint32_t>(),
                       dout.as<uint32_t>(), n);
  else
    hipLaunchKernelGGL(k_selftest_field_sqrt<Fp2Ops>, dim3(nb64(n)), dim3(64), 0, nullptr, din.as<uint32_t>(),
                       dout.as<uint32_t>(), n);
  BH_TRY_HIP(hipGetLastError());
  BH_TRY_HIP(hipMemcpy(out, dout.p, out_b, hipMemcpyDeviceToHost));
  return BH_OK;
}

}  // extern "C"
