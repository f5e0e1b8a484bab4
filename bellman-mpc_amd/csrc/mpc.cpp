// The two parameter rounds of the fork's multi-party trusted setup (reference groth16/mpc.rs) for
// any length and any Fr scalar, on device-resident vectors.
//
//   round one, "common"    CommonParamterInStorage / CommonParamter           mpc.rs:362-414
//     initial_common_paramters, mpc_common_paramters_generator, verify_common_paramter
//                                                                              mpc.rs:708-862
//     the matrixed_h part of CommonParamterInStorage::matrix                   mpc.rs:631-635
//   round two, "uncommon"  UnCommonParamterInStorage / UnCommonParamter        mpc.rs:891-1131
//
// Both rounds have one shape: a storage holds two (G1, G2) point pairs and three (G1, G2) vector
// pairs; a contribution holds a ParameterPair (g1_result, g2_result, g1_mine, g2_mine) for each
// point pair and a TauParameterPair (a list of ParameterPairs) for each vector pair.  The player's
// side is varbase.hip's per-element multiplication for the results and crs.hip's fixed-base path
// for the "mine" lists; the verifier batches the reference's per-element pairing checks with the
// caller's random z_i over verify.cpp's Miller loop.  The structure check
// (bh_mpc_common_check, bh_mpc_common_verify_structure) is not in the
// reference: it shows that a round-one storage is a power sequence, with the multiexp, the
// power-scalar kernel and the host pairing that are already here.  bh_params_check (DESIGN.md
// section 19) closes the chain the same way: Parameters against a circuit and such a storage.
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <memory>

#include "group_fft.h"
#include "pairing.h"
#include "pairing_dev.h"
#include "params_check.h"
#include "point_codec.h"
#include "r1cs.h"
#include "varbase.h"

using namespace bh;

namespace {

struct MpcStorage {
  bh_ctx* ctx = nullptr;
  // common: alpha, beta; uncommon: gamma, delta
  AffinePt<Fp> p1[2];
  AffinePt<Fp2> p2[2];
  // common: tau, alpha_mul_tau, beta_mul_tau; uncommon: kin, kout, h -- (g1, g2) each
  std::unique_ptr<bh_srs> v[6];
};

struct HostPair {  // ParameterPair, mpc.rs:16-29
  AffinePt<Fp> r1, m1;
  AffinePt<Fp2> r2, m2;
};

struct MpcContrib {
  bh_ctx* ctx = nullptr;
  HostPair pp[2];
  std::unique_ptr<bh_srs> res[6], mine[6];
};

}  // namespace

struct bh_mpc_common : MpcStorage {};
struct bh_mpc_uncommon : MpcStorage {};
struct bh_mpc_common_contrib : MpcContrib {};
struct bh_mpc_uncommon_contrib : MpcContrib {};
// CommonParamterMatrix (mpc.rs:597-645) of one circuit: BH_MPC_KIN_G1 .. BH_MPC_MATRIX_B_G2
struct bh_mpc_matrix {
  bh_ctx* ctx = nullptr;
  size_t m = 0, ni = 0, na = 0;
  std::unique_ptr<bh_srs> v[9];
};

namespace {

AffinePt<Fp> g1_gen() { return jac_to_affine(crs_g1_gen()); }
AffinePt<Fp2> g2_gen() { return jac_to_affine(crs_g2_gen()); }
// device vector -> host affine points (caller holds ctx->mu; the stream is idle)
template <class T>
bh_status download(const bh_srs* s, std::vector<AffinePt<T>>* out) {
  return download_points<HostOfField<T>>(*s, s->n, out);
}
template <class T>
AffinePt<T> pt_mul(const AffinePt<T>& p, const uint64_t k[4]) {
  return jac_to_affine(jac_mul(jac_from_affine(p), k, 4));
}
template <class T>
AffinePt<T> pt_neg(AffinePt<T> p) {
  if (!p.infinity) p.y = neg(p.y);
  return p;
}
bh_status clone_srs(bh_ctx* ctx, const bh_srs* in, std::unique_ptr<bh_srs>* out) {
  std::unique_ptr<bh_srs> r(new bh_srs());
  r->ctx = ctx;
  r->group = in->group;
  r->n = in->n;
  r->identity_idx = in->identity_idx;
  const size_t bytes = in->n * with_group(in->group, [](auto g) { return decltype(g)::WORDS * (size_t)4; });
  BH_TRY_HIP(r->pts.alloc(std::max<size_t>(bytes, 16)));
  if (bytes) {
    BH_TRY_HIP(hipMemcpyAsync(r->pts.p, in->pts.p, bytes, hipMemcpyDeviceToDevice, ctx->stream));
    BH_TRY_HIP(hipStreamSynchronize(ctx->stream));
  }
  *out = std::move(r);
  return BH_OK;
}

bool same_device(const bh_ctx* ctx, const bh_srs* s) { return s && s->ctx && s->ctx->device == ctx->device; }

// ---------------------------------------------------------------- the player's side
struct Tables {
  bh_srs t1, t2;
  bh_status upload(bh_ctx* ctx) {
    const auto a = crs_table_g1();
    const auto b = crs_table_g2();
    bh_status s = srs_upload_affine(ctx, a.data(), a.size(), &t1);
    if (s) return s;
    return srs_upload_affine(ctx, b.data(), b.size(), &t2);
  }
};

// make_new_paramter (mpc.rs:647-675) with inverse == false
HostPair new_pair(const AffinePt<Fp>& o1, const AffinePt<Fp2>& o2, const uint64_t k[4]) {
  return HostPair{pt_mul(o1, k), pt_mul(g1_gen(), k), pt_mul(o2, k), pt_mul(g2_gen(), k)};
}

// make_new_tau_paramter (mpc.rs:677-706) on vector pair j: scalars (a x^i)^(+-1)
bh_status new_tau_pair(bh_ctx* ctx, const Tables& tab, const MpcStorage* st, int j, const uint64_t a[4],
                       const uint64_t x[4], int invert, MpcContrib* c) {
  const bh_srs* g1 = st->v[2 * j].get();
  const bh_srs* g2 = st->v[2 * j + 1].get();
  DevBuf d_sc;
  bh_status s = varbase_power_scalars(ctx, g1->n, a, x, invert, &d_sc);
  if (s) return s;
  const uint64_t one[4] = {1, 0, 0, 0};
  const int stride = memcmp(x, one, 32) ? 8 : 0;  // x = 1: one scalar for the whole vector
  for (int k = 0; k < 2; k++) {
    c->res[2 * j + k].reset(new bh_srs());
    c->mine[2 * j + k].reset(new bh_srs());
  }
  if ((s = varbase_mul(ctx, g1, d_sc.as<uint32_t>(), stride, 255, c->res[2 * j].get()))) return s;
  if ((s = varbase_mul(ctx, g2, d_sc.as<uint32_t>(), stride, 255, c->res[2 * j + 1].get()))) return s;
  if ((s = fixed_base_device<G1Ops>(ctx, tab.t1, d_sc.as<uint32_t>(), g1->n, c->mine[2 * j].get()))) return s;
  return fixed_base_device<G2Ops>(ctx, tab.t2, d_sc.as<uint32_t>(), g1->n, c->mine[2 * j + 1].get());
}

// to_storage_format (mpc.rs:381-394, 910-923)
template <class S>
bh_status to_storage(bh_ctx* ctx, const MpcContrib* c, S** out) {
  std::unique_ptr<S> n(new S());
  n->ctx = ctx;
  for (int k = 0; k < 2; k++) {
    n->p1[k] = c->pp[k].r1;
    n->p2[k] = c->pp[k].r2;
  }
  for (int k = 0; k < 6; k++) {
    bh_status s = clone_srs(ctx, c->res[k].get(), &n->v[k]);
    if (s) return s;
  }
  *out = n.release();
  return BH_OK;
}

// ---------------------------------------------------------------- the verifier's side
// verify_new_paramter (mpc.rs:787-804): e(R1, G2) == e(O1, M2) and e(R1, G2) == e(G1, R2)
bool verify_pair(const HostPair& p, const AffinePt<Fp>& o1) {
  const AffinePt<Fp2> ng2 = pt_neg(g2_gen());
  return pairing_product_is_one({{p.r1, ng2}, {o1, p.m2}}) && pairing_product_is_one({{p.r1, ng2}, {g1_gen(), p.r2}});
}

template <class T>
bh_status msm(bh_ctx* ctx, const bh_srs* b, const uint32_t* d_z, AffinePt<T>* out) {
  Jac<T> r;
  bh_status s = msm_device<HostOfField<T>>(ctx, b, 0, d_z, b->n, nullptr, &r, nullptr);
  if (!s) *out = jac_to_affine(r);
  return s;
}

// prod_i f(p_i, q_i): the Miller loops shared over the context's host pool, the partial Fp12
// products multiplied
Fp12 pooled_miller(bh_ctx* ctx, const std::vector<AffinePt<Fp>>& p, const std::vector<AffinePt<Fp2>>& q) {
  HostPool& pool = ctx_pool(ctx);
  const size_t n = p.size();
  const int parts = (int)std::min<size_t>(n, (size_t)pool.size());
  std::vector<Fp12> part((size_t)std::max(parts, 1), f12_one());
  if (parts)
    pool.parallel_for(parts, [&](int t) {
      const size_t lo = n * (size_t)t / parts, hi = n * (size_t)(t + 1) / parts;
      std::vector<Pair> ps;
      ps.reserve(hi - lo);
      for (size_t i = lo; i < hi; i++) ps.push_back({p[i], q[i]});
      part[t] = multi_miller_loop(ps);
    });
  Fp12 f = f12_one();
  for (const Fp12& x : part) f = f12_mul(f, x);
  return f;
}

// One vector pair of verify_common_paramter (mpc.rs:842-854), batched with z:
//   (1) e(S1, -G2) prod_i e(z_i O1_i, M2_i) == 1,  (2) e(S1, G2) == e(G1, S2),
// S1 = sum z_i R1_i, S2 = sum z_i R2_i.  The len Miller loops of (1) run on the device
// (pairing_dev.hip) over the device vectors z_i O1_i and M2; on the host's pool threads instead
// when BH_MPC_HOST_MILLER=1 is set (a diagnostic mode, like BH_PROVER_SERIAL) and when the device
// product reports a zero denominator, which only an M2 element outside the subgroup can cause: such
// a contribution gets the host loop's verdict, whatever that is.  miller_ms: wall time of the len
// Miller loops on whichever path ran; on_device: counts the pairs whose loops ran on the device.
bh_status verify_tau_pair(bh_ctx* ctx, const MpcStorage* st, const MpcContrib* c, int j, const uint32_t* d_z,
                          int nbits, bool* ok, double* miller_ms, int* on_device) {
  AffinePt<Fp> s1;
  AffinePt<Fp2> s2;
  bh_status s = msm(ctx, c->res[2 * j].get(), d_z, &s1);
  if (s) return s;
  if ((s = msm(ctx, c->res[2 * j + 1].get(), d_z, &s2))) return s;
  bh_srs q;
  if ((s = varbase_mul(ctx, st->v[2 * j].get(), d_z, 8, nbits, &q))) return s;
  const bh_srs* mine2 = c->mine[2 * j + 1].get();
  const AffinePt<Fp2> g2 = g2_gen(), ng2 = pt_neg(g2);
  const char* env = getenv("BH_MPC_HOST_MILLER");
  bool host = env && env[0] == '1';
  Fp12 f;
  auto t0 = std::chrono::steady_clock::now();
  auto add_ms = [&] {
    if (miller_ms) *miller_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  };
  if (!host) {
    s = miller_product_device(ctx, &q, 0, mine2, 0, q.n, 0, &f);
    add_ms();
    if (s == BH_ERR_PAIRING_DEGENERATE) host = true;
    else if (s) return s;
    else if (on_device) ++*on_device;
  }
  if (host) {
    std::vector<AffinePt<Fp>> qh;
    std::vector<AffinePt<Fp2>> m2;
    if ((s = download(&q, &qh))) return s;
    if ((s = download(mine2, &m2))) return s;
    t0 = std::chrono::steady_clock::now();
    f = pooled_miller(ctx, qh, m2);
    add_ms();
  }
  f = f12_mul(f, multi_miller_loop({{s1, ng2}}));
  *ok = f12_is_one(final_exponentiation(f)) && pairing_product_is_one({{s1, ng2}, {g1_gen(), s2}});
  return BH_OK;
}

bh_status upload_z(bh_ctx* ctx, const uint64_t* z, size_t n, DevBuf* d_z, int* nbits) {
  int nb = 1;
  for (size_t i = 0; i < n; i++) {
    if (!scalar_below_r(z + 4 * i) || scalar_is_zero(z + 4 * i)) return BH_ERR_INVALID_ARGUMENT;
    nb = std::max(nb, scalar_bits(z + 4 * i));
  }
  *nbits = nb;
  return varbase_upload_scalars(ctx, z, n, nb, d_z);
}

// ---------------------------------------------------------------- bytes
void put_u32(std::vector<uint8_t>& v, size_t n) {
  v.push_back((uint8_t)(n >> 24));
  v.push_back((uint8_t)(n >> 16));
  v.push_back((uint8_t)(n >> 8));
  v.push_back((uint8_t)n);
}
// Every writer and reader below takes one `compressed` switch: the layouts are the same, each
// point 48 / 96 bytes instead of 96 / 192.  Single points go through the host's to_compressed /
// point_from_compressed, vectors through the device codec (point_codec.hip).
size_t wire_bytes(int group, bool compressed) {
  return compressed ? compressed_bytes(group) : with_group(group, [](auto g) { return decltype(g)::WIRE; });
}
template <class T>
void put(std::vector<uint8_t>& v, const AffinePt<T>& p, bool compressed) {
  uint8_t b[HostOfField<T>::WIRE];
  if (compressed) to_compressed(p, b);
  else to_uncompressed(p, b);
  v.insert(v.end(), b, b + wire_bytes(HostOfField<T>::ID, compressed));
}
bh_status put_vec(std::vector<uint8_t>& v, bh_ctx* ctx, const bh_srs* s, bool compressed) {
  const size_t at = v.size();
  v.resize(at + s->n * wire_bytes(s->group, compressed));
  if (compressed) return srs_to_compressed(ctx, s, 0, s->n, v.data() + at);
  return srs_read_bytes(ctx, s, 0, s->n, v.data() + at);  // the codec, or the host loop under its knob
}

struct Reader {
  const uint8_t* in;
  size_t len, o = 0;
  int checked;
  bool compressed;
  bh_status u32(size_t* n) {
    if (len - o < 4) return BH_ERR_UNEXPECTED_EOF;
    *n = ((size_t)in[o] << 24) | ((size_t)in[o + 1] << 16) | ((size_t)in[o + 2] << 8) | in[o + 3];
    o += 4;
    return BH_OK;
  }
  template <class T>
  bh_status point(AffinePt<T>* p) {
    const size_t pb = wire_bytes(HostOfField<T>::ID, compressed);
    if (len - o < pb) return BH_ERR_UNEXPECTED_EOF;
    o += pb;
    if (compressed) return point_from_compressed(in + o - pb, p, checked != 0);  // refuses the identity
    const int r = from_uncompressed(in + o - pb, p, checked != 0, checked != 0);
    if (r == -3) return BH_ERR_NOT_IN_SUBGROUP;
    if (r == -2) return BH_ERR_NOT_ON_CURVE;
    return (r || p->infinity) ? BH_ERR_INVALID_ENCODING : BH_OK;
  }
  // n consecutive points of one group -> device vector (the checks of bh_params_load)
  bh_status vec(bh_ctx* ctx, int group, size_t n, std::unique_ptr<bh_srs>* out) {
    const size_t pb = wire_bytes(group, compressed);
    if (n > (len - o) / pb) return BH_ERR_UNEXPECTED_EOF;
    out->reset(new bh_srs());
    const bh_status s = compressed ? srs_from_compressed(ctx, group, in + o, n, checked, true, out->get())
                                   : srs_from_bytes(ctx, group, in + o, n, checked, true, out->get());
    o += n * pb;
    return s;
  }
  // n ParameterPairs (g1_result, g2_result, g1_mine, g2_mine per element) -> their four vectors
  bh_status pairs(bh_ctx* ctx, size_t n, std::unique_ptr<bh_srs>* const dst[4]) {
    size_t w[4], pair = 0;
    for (int k = 0; k < 4; k++) pair += w[k] = wire_bytes(k & 1 ? BH_G2 : BH_G1, compressed);
    if (n > (len - o) / pair) return BH_ERR_UNEXPECTED_EOF;
    const uint8_t* list = in + o;
    o += n * pair;
    for (int k = 0; k < 4; k++) dst[k]->reset(new bh_srs());
    bh_status s;
    if (compressed || !point_codec_host()) {
      // the interleaved list goes to the device as it is; the codec reads it strided
      if (!compressed) point_codec_note(true);
      DevBuf raw;
      BH_TRY_HIP(raw.alloc(std::max<size_t>(n * pair, 16)));
      if (n) BH_TRY_HIP(hipMemcpyAsync(raw.p, list, n * pair, hipMemcpyHostToDevice, ctx->stream));
      size_t off = 0;
      for (int k = 0; k < 4; k++) {
        // each call returns synchronised, so raw outlives every read of it
        const int group = k & 1 ? BH_G2 : BH_G1;
        s = compressed ? points_decompress_device(ctx, group, raw.as<uint8_t>(), pair, off, n, checked, true, dst[k]->get())
                       : points_from_wire_device(ctx, group, raw.as<uint8_t>(), pair, off, n, checked, true, dst[k]->get());
        if (s) return s;
        off += w[k];
      }
      return BH_OK;
    }
    // BH_POINT_CODEC_HOST=1: de-interleave the list into its four vectors on the host
    std::vector<uint8_t> col[4];
    for (int k = 0; k < 4; k++) col[k].resize(n * w[k]);
    for (size_t i = 0; i < n; i++) {
      const uint8_t* b = list + i * pair;
      size_t off = 0;
      for (int k = 0; k < 4; k++) {
        memcpy(&col[k][i * w[k]], b + off, w[k]);
        off += w[k];
      }
    }
    for (int k = 0; k < 4; k++)
      if ((s = srs_from_bytes(ctx, k & 1 ? BH_G2 : BH_G1, col[k].data(), n, checked, true, dst[k]->get()))) return s;
    return BH_OK;
  }
};

// storage bytes.  common: u32-BE len, the four points, the six vectors; uncommon (vector pairs
// of different lengths): the four points, then every vector behind its own u32-BE length
bh_status storage_write(const MpcStorage* st, bool common, bool compressed, std::vector<uint8_t>& v) {
  if (common) put_u32(v, st->v[0]->n);
  for (int k = 0; k < 2; k++) {
    put(v, st->p1[k], compressed);
    put(v, st->p2[k], compressed);
  }
  for (int k = 0; k < 6; k++) {
    if (!common) put_u32(v, st->v[k]->n);
    bh_status s = put_vec(v, st->ctx, st->v[k].get(), compressed);
    if (s) return s;
  }
  return BH_OK;
}

template <class S>
bh_status storage_read(bh_ctx* ctx, const uint8_t* bytes, size_t len, int checked, bool common, bool compressed,
                       S** out) {
  Reader r{bytes, len, 0, checked, compressed};
  std::unique_ptr<S> st(new S());
  st->ctx = ctx;
  bh_status s;
  size_t n = 0;
  if (common && (s = r.u32(&n))) return s;
  for (int k = 0; k < 2; k++) {
    if ((s = r.point(&st->p1[k])) || (s = r.point(&st->p2[k]))) return s;
  }
  for (int k = 0; k < 6; k++) {
    if (!common) {
      size_t nk;
      if ((s = r.u32(&nk))) return s;
      if (k & 1) {
        if (nk != n) return BH_ERR_INVALID_ENCODING;  // a pair's vectors have one length
      } else {
        n = nk;
      }
    }
    if ((s = r.vec(ctx, k & 1 ? BH_G2 : BH_G1, n, &st->v[k]))) return s;
  }
  if (r.o != len) return BH_ERR_INVALID_ENCODING;
  *out = st.release();
  return BH_OK;
}

// contribution bytes: the ParameterPairs in declaration order (common: alpha, beta; uncommon:
// delta, gamma), each g1_result, g2_result, g1_mine, g2_mine; then the three TauParameterPairs,
// each a u32-BE length and that many ParameterPairs
bh_status contrib_write(const MpcContrib* c, bool common, bool compressed, std::vector<uint8_t>& v) {
  for (int k = 0; k < 2; k++) {
    const HostPair& p = c->pp[common ? k : 1 - k];
    put(v, p.r1, compressed);
    put(v, p.r2, compressed);
    put(v, p.m1, compressed);
    put(v, p.m2, compressed);
  }
  for (int j = 0; j < 3; j++) {
    if (compressed || !point_codec_host()) {  // the four vectors coded into one interleaved device list, one copy back
      if (!compressed) point_codec_note(true);
      const bh_srs* col[4] = {c->res[2 * j].get(), c->res[2 * j + 1].get(), c->mine[2 * j].get(),
                              c->mine[2 * j + 1].get()};
      const size_t n = col[0]->n, pair = 2 * (wire_bytes(BH_G1, compressed) + wire_bytes(BH_G2, compressed));
      put_u32(v, n);
      const size_t at = v.size();
      v.resize(at + n * pair);
      if (!n) continue;
      DevBuf d;
      BH_TRY_HIP(d.alloc(n * pair));
      size_t off = 0;
      for (int k = 0; k < 4; k++) {
        if (col[k]->n != n) return BH_ERR_INVALID_ARGUMENT;
        if (bh_status s = compressed ? points_compress_device(c->ctx, col[k], 0, n, d.as<uint8_t>(), pair, off)
                                     : points_to_wire_device(c->ctx, col[k], 0, n, d.as<uint8_t>(), pair, off))
          return s;
        off += wire_bytes(col[k]->group, compressed);
      }
      BH_TRY_HIP(hipMemcpyAsync(v.data() + at, d.p, n * pair, hipMemcpyDeviceToHost, c->ctx->stream));
      BH_TRY_HIP(hipStreamSynchronize(c->ctx->stream));  // d is freed at the end of the round
      off = 0;
      for (int k = 0; k < 4; k++) {
        if (compressed) points_compress_patch(col[k], 0, n, v.data() + at, pair, off);
        else points_wire_patch(col[k], 0, n, v.data() + at, pair, off);
        off += wire_bytes(col[k]->group, compressed);
      }
      continue;
    }
    point_codec_note(false);
    std::vector<AffinePt<Fp>> r1, m1;
    std::vector<AffinePt<Fp2>> r2, m2;
    bh_status s;
    if ((s = download(c->res[2 * j].get(), &r1)) || (s = download(c->res[2 * j + 1].get(), &r2)) ||
        (s = download(c->mine[2 * j].get(), &m1)) || (s = download(c->mine[2 * j + 1].get(), &m2)))
      return s;
    put_u32(v, r1.size());
    for (size_t i = 0; i < r1.size(); i++) {
      put(v, r1[i], false);
      put(v, r2[i], false);
      put(v, m1[i], false);
      put(v, m2[i], false);
    }
  }
  return BH_OK;
}

template <class Cn>
bh_status contrib_read(bh_ctx* ctx, const uint8_t* bytes, size_t len, int checked, bool common, bool compressed,
                       Cn** out) {
  Reader r{bytes, len, 0, checked, compressed};
  std::unique_ptr<Cn> c(new Cn());
  c->ctx = ctx;
  bh_status s;
  for (int k = 0; k < 2; k++) {
    HostPair& p = c->pp[common ? k : 1 - k];
    if ((s = r.point(&p.r1)) || (s = r.point(&p.r2)) || (s = r.point(&p.m1)) || (s = r.point(&p.m2))) return s;
  }
  for (int j = 0; j < 3; j++) {
    size_t n;
    if ((s = r.u32(&n))) return s;
    std::unique_ptr<bh_srs>* const dst[4] = {&c->res[2 * j], &c->res[2 * j + 1], &c->mine[2 * j], &c->mine[2 * j + 1]};
    if ((s = r.pairs(ctx, n, dst))) return s;
  }
  if (r.o != len) return BH_ERR_INVALID_ENCODING;
  *out = c.release();
  return BH_OK;
}

bh_status emit(const std::vector<uint8_t>& v, uint8_t* out, size_t cap, size_t* written) {
  *written = v.size();
  if (!out) return BH_OK;  // size query
  if (cap < v.size()) return BH_ERR_INVALID_ARGUMENT;
  memcpy(out, v.data(), v.size());
  return BH_OK;
}

bh_status storage_point(const MpcStorage* st, int which, uint8_t* out) {
  if (!st || !out || which < 0 || which > 3) return BH_ERR_INVALID_ARGUMENT;
  if (which & 1)
    to_uncompressed(st->p2[which >> 1], out);
  else
    to_uncompressed(st->p1[which >> 1], out);
  return BH_OK;
}
bh_status contrib_point(const MpcContrib* c, int which, uint8_t* out) {
  if (!c || !out || which < 0 || which > 7) return BH_ERR_INVALID_ARGUMENT;
  const HostPair& p = c->pp[which >> 2];
  switch (which & 3) {
    case 0: to_uncompressed(p.r1, out); break;
    case 1: to_uncompressed(p.r2, out); break;
    case 2: to_uncompressed(p.m1, out); break;
    default: to_uncompressed(p.m2, out); break;
  }
  return BH_OK;
}
bh_status contrib_vector(const MpcContrib* c, int which, int mine, const bh_srs** out) {
  if (!c || !out || which < 0 || which > 5) return BH_ERR_INVALID_ARGUMENT;
  *out = (mine ? c->mine : c->res)[which].get();
  return BH_OK;
}

bh_status check_scalars(std::initializer_list<const uint64_t*> ws) {
  for (const uint64_t* w : ws)
    if (!w || !scalar_below_r(w)) return BH_ERR_INVALID_ARGUMENT;
  for (const uint64_t* w : ws)
    if (scalar_is_zero(w)) return BH_ERR_UNEXPECTED_IDENTITY;
  return BH_OK;
}

struct CtxLock {
  std::lock_guard<std::mutex> lk;
  explicit CtxLock(bh_ctx* ctx) : lk(ctx->mu) {}
};
#define MPC_ENTER(ctx)                      \
  CtxLock _lock(ctx);                       \
  BH_TRY_HIP(hipSetDevice((ctx)->device)); \
  if (bh_status _s = scratch_check(ctx)) return _s

// the entry points' shared halves: a handle's bytes under its context's lock, and the checks in
// front of a read
template <class H, class Write>
bh_status handle_bytes(const H* h, Write&& write, uint8_t* out, size_t cap, size_t* written) {
  if (!h || !written) return BH_ERR_INVALID_ARGUMENT;
  std::vector<uint8_t> v;
  {
    CtxLock lk(h->ctx);
    BH_TRY_HIP(hipSetDevice(h->ctx->device));
    if (bh_status s = write(v)) return s;
  }
  return emit(v, out, cap, written);
}
bh_status storage_bytes(const MpcStorage* st, bool common, bool compressed, uint8_t* out, size_t cap, size_t* written) {
  return handle_bytes(st, [&](std::vector<uint8_t>& v) { return storage_write(st, common, compressed, v); }, out, cap,
                      written);
}
bh_status contrib_bytes(const MpcContrib* c, bool common, bool compressed, uint8_t* out, size_t cap, size_t* written) {
  return handle_bytes(c, [&](std::vector<uint8_t>& v) { return contrib_write(c, common, compressed, v); }, out, cap,
                      written);
}
template <class S>
bh_status storage_parse(bh_ctx* ctx, const uint8_t* bytes, size_t len, int checked, bool common, bool compressed,
                        S** out) {
  if (!ctx || !bytes || !out) return BH_ERR_INVALID_ARGUMENT;
  MPC_ENTER(ctx);
  return storage_read(ctx, bytes, len, checked, common, compressed, out);
}
template <class Cn>
bh_status contrib_parse(bh_ctx* ctx, const uint8_t* bytes, size_t len, int checked, bool common, bool compressed,
                        Cn** out) {
  if (!ctx || !bytes || !out) return BH_ERR_INVALID_ARGUMENT;
  MPC_ENTER(ctx);
  return contrib_read(ctx, bytes, len, checked, common, compressed, out);
}

thread_local double g_miller_ms = 0;
thread_local int g_miller_device = 0;
thread_local double g_matrix_ms[3] = {0, 0, 0};
thread_local double g_check_ms[2] = {0, 0};
thread_local double g_pcheck_ms[3] = {0, 0, 0};

double ms_since(std::chrono::steady_clock::time_point t0) {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

// ---------------------------------------------------------------- the structure check
// What bh_mpc_common_check looks at: a storage's own fields, or a contribution's results (its
// to_storage_format(), mpc.rs:381-394) before they are cloned.
struct CheckView {
  AffinePt<Fp> p1[2];
  AffinePt<Fp2> p2[2];
  const bh_srs* v[6];
};
CheckView view_of(const MpcStorage* st) {
  CheckView w;
  for (int k = 0; k < 2; k++) {
    w.p1[k] = st->p1[k];
    w.p2[k] = st->p2[k];
  }
  for (int k = 0; k < 6; k++) w.v[k] = st->v[k].get();
  return w;
}
CheckView view_of(const MpcContrib* c) {
  CheckView w;
  for (int k = 0; k < 2; k++) {
    w.p1[k] = c->pp[k].r1;
    w.p2[k] = c->pp[k].r2;
  }
  for (int k = 0; k < 6; k++) w.v[k] = c->res[k].get();
  return w;
}

struct Equation {  // `bit` (a BH_MPC_CHECK_* constant) is set unless the product of the pairs is one
  uint32_t bit;
  std::vector<Pair> pairs;
};

template <class T>
bool same_bytes(const AffinePt<T>& a, const AffinePt<T>& b) {
  uint8_t x[HostOfField<T>::WIRE], y[HostOfField<T>::WIRE];
  to_uncompressed(a, x);
  to_uncompressed(b, y);
  return a.infinity == b.infinity && !memcmp(x, y, sizeof x);
}

// Equations 0-8 of bh_mpc_common_check on w, whose six vectors have one
// length, with the weights rho^i; `more` joins the nine pairing equations on the pool.  The sums
// are msm_device's over the weights varbase_power_scalars writes; the shifted sum R is the tau
// vector from element 1 under the weights from index 0.  ms[0]: weights and multiexps, ms[1]:
// pairings.
bh_status structure_mask(bh_ctx* ctx, const CheckView& w, const uint64_t rho[4], std::vector<Equation> more,
                         uint32_t* mask, double ms[2]) {
  const size_t len = w.v[0]->n;
  const AffinePt<Fp> g1 = g1_gen();
  const AffinePt<Fp2> g2 = g2_gen(), ng2 = pt_neg(g2);
  uint32_t m = 0;
  std::vector<Equation> eq = std::move(more);
  eq.push_back({BH_MPC_CHECK_ALPHA, {{w.p1[0], ng2}, {g1, w.p2[0]}}});
  eq.push_back({BH_MPC_CHECK_BETA, {{w.p1[1], ng2}, {g1, w.p2[1]}}});
  auto t0 = std::chrono::steady_clock::now();
  if (len) {
    std::vector<AffinePt<Fp>> t1;
    std::vector<AffinePt<Fp2>> t2;
    bh_status s;
    if ((s = download_points<G1Host>(*w.v[0], 1, &t1))) return s;
    if ((s = download_points<G2Host>(*w.v[1], std::min<size_t>(len, 2), &t2))) return s;
    if (!same_bytes(t1[0], g1) || !same_bytes(t2[0], g2)) m |= BH_MPC_CHECK_FIRST;
    DevBuf d_w;
    const uint64_t one[4] = {1, 0, 0, 0};
    if ((s = varbase_power_scalars(ctx, len, one, rho, 0, &d_w))) return s;
    AffinePt<Fp> s1[3];
    AffinePt<Fp2> s2[3];
    for (int j = 0; j < 3; j++) {
      if ((s = msm(ctx, w.v[2 * j], d_w.as<uint32_t>(), &s1[j]))) return s;
      if ((s = msm(ctx, w.v[2 * j + 1], d_w.as<uint32_t>(), &s2[j]))) return s;
    }
    if (len >= 2) {
      Jac<Fp> l, r;
      if ((s = msm_device<G1Host>(ctx, w.v[0], 0, d_w.as<uint32_t>(), len - 1, nullptr, &l, nullptr))) return s;
      if ((s = msm_device<G1Host>(ctx, w.v[0], 1, d_w.as<uint32_t>(), len - 1, nullptr, &r, nullptr))) return s;
      eq.push_back({BH_MPC_CHECK_POWERS, {{jac_to_affine(r), ng2}, {jac_to_affine(l), t2[1]}}});
    }
    eq.push_back({BH_MPC_CHECK_TAU_G2, {{s1[0], ng2}, {g1, s2[0]}}});
    const uint32_t by_scalar[3] = {0, BH_MPC_CHECK_ALPHA_TAU, BH_MPC_CHECK_BETA_TAU};
    const uint32_t in_g2[3] = {0, BH_MPC_CHECK_ALPHA_TAU_G2, BH_MPC_CHECK_BETA_TAU_G2};
    for (int j = 1; j < 3; j++) {
      eq.push_back({by_scalar[j], {{s1[j], ng2}, {s1[0], w.p2[j - 1]}}});
      eq.push_back({in_g2[j], {{s1[j], ng2}, {g1, s2[j]}}});
    }
  }
  ms[0] = ms_since(t0);
  t0 = std::chrono::steady_clock::now();
  std::vector<char> bad(eq.size(), 0);  // every equation is evaluated: the mask is complete
  ctx_pool(ctx).parallel_for((int)eq.size(), [&](int k) { bad[k] = !pairing_product_is_one(eq[k].pairs); });
  for (size_t k = 0; k < eq.size(); k++)
    if (bad[k]) m |= eq[k].bit;
  ms[1] = ms_since(t0);
  *mask = m;
  return BH_OK;
}

bool check_weight(const uint64_t* rho) { return rho && scalar_below_r(rho) && !scalar_is_zero(rho); }

}  // namespace

extern "C" {

// ================================================================ round one
bh_status bh_mpc_common_initial(bh_ctx* ctx, size_t len, bh_mpc_common** out) {
  if (!ctx || !out || len > 0x7fffffffull) return BH_ERR_INVALID_ARGUMENT;
  MPC_ENTER(ctx);
  std::unique_ptr<bh_mpc_common> st(new bh_mpc_common());
  st->ctx = ctx;
  for (int k = 0; k < 2; k++) {
    st->p1[k] = g1_gen();
    st->p2[k] = g2_gen();
  }
  const std::vector<AffinePt<Fp>> v1(len, g1_gen());
  const std::vector<AffinePt<Fp2>> v2(len, g2_gen());
  bh_status s;
  st->v[0].reset(new bh_srs());
  st->v[1].reset(new bh_srs());
  if ((s = srs_upload_affine(ctx, v1.data(), len, st->v[0].get()))) return s;
  if ((s = srs_upload_affine(ctx, v2.data(), len, st->v[1].get()))) return s;
  for (int k = 2; k < 6; k++)
    if ((s = clone_srs(ctx, st->v[k & 1].get(), &st->v[k]))) return s;
  *out = st.release();
  return BH_OK;
}

bh_status bh_mpc_common_contribute(bh_ctx* ctx, const bh_mpc_common* st, const uint64_t alpha[4],
                                   const uint64_t beta[4], const uint64_t tau[4], bh_mpc_common_contrib** out) {
  if (!ctx || !st || !out || st->ctx->device != ctx->device) return BH_ERR_INVALID_ARGUMENT;
  if (bh_status s = check_scalars({alpha, beta, tau})) return s;
  MPC_ENTER(ctx);
  std::unique_ptr<bh_mpc_common_contrib> c(new bh_mpc_common_contrib());
  c->ctx = ctx;
  c->pp[0] = new_pair(st->p1[0], st->p2[0], alpha);
  c->pp[1] = new_pair(st->p1[1], st->p2[1], beta);
  Tables tab;
  bh_status s = tab.upload(ctx);
  if (s) return s;
  const uint64_t one[4] = {1, 0, 0, 0};
  const uint64_t* a[3] = {one, alpha, beta};  // mpc.rs:756-776
  for (int j = 0; j < 3; j++)
    if ((s = new_tau_pair(ctx, tab, st, j, a[j], tau, 0, c.get()))) return s;
  *out = c.release();
  return BH_OK;
}

bh_status bh_mpc_common_verify(bh_ctx* ctx, const bh_mpc_common* st, const bh_mpc_common_contrib* c,
                               const uint64_t* z, int* valid, bh_mpc_common** next) {
  if (!ctx || !st || !c || !valid || !next) return BH_ERR_INVALID_ARGUMENT;
  if (st->ctx->device != ctx->device || c->ctx->device != ctx->device) return BH_ERR_INVALID_ARGUMENT;
  *valid = 0;
  *next = nullptr;
  const size_t len = st->v[0]->n;
  if (len && !z) return BH_ERR_INVALID_ARGUMENT;
  MPC_ENTER(ctx);
  g_miller_ms = 0;
  g_miller_device = 0;
  DevBuf d_z;
  int nbits = 1;
  bh_status s = upload_z(ctx, z, len, &d_z, &nbits);
  if (s) return s;
  // the reference's length check (mpc.rs:815-817), against the storage too: its loops index
  // the storage's vectors with the contribution's length
  for (int k = 0; k < 6; k++)
    if (c->res[k]->n != len || c->mine[k]->n != len) return BH_OK;
  bool ok = verify_pair(c->pp[0], st->p1[0]) && verify_pair(c->pp[1], st->p1[1]);
  // alpha_mul_tau and beta_mul_tau (mpc.rs:842-854); the reference's check of the tau list
  // itself is commented out (mpc.rs:831-840) and result_tau stays true
  for (int j = 1; j < 3 && ok; j++)
    if ((s = verify_tau_pair(ctx, st, c, j, d_z.as<uint32_t>(), nbits, &ok, &g_miller_ms, &g_miller_device)))
      return s;
  if (!ok) return BH_OK;
  if ((s = to_storage(ctx, c, next))) return s;
  *valid = 1;
  return BH_OK;
}

// The storage is a power sequence: DESIGN.md section 16
bh_status bh_mpc_common_check(bh_ctx* ctx, const bh_mpc_common* st, const uint64_t rho[4], int* valid,
                              uint32_t* failed) {
  if (!ctx || !st || !valid || !check_weight(rho) || st->ctx->device != ctx->device) return BH_ERR_INVALID_ARGUMENT;
  *valid = 0;
  if (failed) *failed = 0;
  MPC_ENTER(ctx);
  uint32_t mask = 0;
  g_check_ms[0] = g_check_ms[1] = 0;
  if (bh_status s = structure_mask(ctx, view_of(st), rho, {}, &mask, g_check_ms)) return s;
  if (failed) *failed = mask;
  *valid = mask == 0;
  return BH_OK;
}

// A contribution to a well-formed storage: three single-element ratio proofs (the first equation
// of verify_new_paramter, mpc.rs:787-804) and the structure check of the result
bh_status bh_mpc_common_verify_structure(bh_ctx* ctx, const bh_mpc_common* st, const bh_mpc_common_contrib* c,
                                         const uint64_t rho[4], int* valid, uint32_t* failed,
                                         bh_mpc_common** next) {
  if (!ctx || !st || !c || !valid || !next || !check_weight(rho)) return BH_ERR_INVALID_ARGUMENT;
  if (st->ctx->device != ctx->device || c->ctx->device != ctx->device) return BH_ERR_INVALID_ARGUMENT;
  *valid = 0;
  *next = nullptr;
  if (failed) *failed = 0;
  MPC_ENTER(ctx);
  g_check_ms[0] = g_check_ms[1] = 0;
  const size_t len = st->v[0]->n;
  for (int k = 0; k < 6; k++)
    if (c->res[k]->n != len || c->mine[k]->n != len) {
      if (failed) *failed = BH_MPC_CHECK_LENGTHS;
      return BH_OK;
    }
  const AffinePt<Fp2> ng2 = pt_neg(g2_gen());
  std::vector<Equation> ratio;
  ratio.push_back({BH_MPC_CHECK_ALPHA_RATIO, {{c->pp[0].r1, ng2}, {st->p1[0], c->pp[0].m2}}});
  ratio.push_back({BH_MPC_CHECK_BETA_RATIO, {{c->pp[1].r1, ng2}, {st->p1[1], c->pp[1].m2}}});
  bh_status s;
  if (len >= 2) {
    std::vector<AffinePt<Fp>> o1, r1;
    std::vector<AffinePt<Fp2>> m2;
    if ((s = download_points<G1Host>(*st->v[0], 2, &o1)) || (s = download_points<G1Host>(*c->res[0], 2, &r1)) ||
        (s = download_points<G2Host>(*c->mine[1], 2, &m2)))
      return s;
    ratio.push_back({BH_MPC_CHECK_TAU_RATIO, {{r1[1], ng2}, {o1[1], m2[1]}}});
  }
  uint32_t mask = 0;
  if ((s = structure_mask(ctx, view_of(c), rho, std::move(ratio), &mask, g_check_ms))) return s;
  if (failed) *failed = mask;
  if (mask) return BH_OK;
  if ((s = to_storage(ctx, c, next))) return s;
  *valid = 1;
  return BH_OK;
}

bh_status bh_mpc_common_h_basis(bh_ctx* ctx, const bh_mpc_common* st, size_t n, bh_srs** h_g1, bh_srs** h_g2) {
  if (!ctx || !st || !h_g1 || !h_g2 || st->ctx->device != ctx->device) return BH_ERR_INVALID_ARGUMENT;
  const size_t len = st->v[0]->n;
  if (n > len / 2) return BH_ERR_INVALID_ARGUMENT;
  MPC_ENTER(ctx);
  std::unique_ptr<bh_srs> a(new bh_srs()), b(new bh_srs());
  bh_status s;
  if ((s = varbase_sub(ctx, st->v[0].get(), 0, n, n, a.get()))) return s;
  if ((s = varbase_sub(ctx, st->v[1].get(), 0, n, n, b.get()))) return s;
  *h_g1 = a.release();
  *h_g2 = b.release();
  return BH_OK;
}

size_t bh_mpc_common_len(const bh_mpc_common* st) { return st ? st->v[0]->n : 0; }
bh_status bh_mpc_common_free(bh_mpc_common* st) {
  delete st;
  return BH_OK;
}
bh_status bh_mpc_common_contrib_free(bh_mpc_common_contrib* c) {
  delete c;
  return BH_OK;
}
bh_status bh_mpc_common_vector(const bh_mpc_common* st, int which, const bh_srs** out) {
  if (!st || !out || which < 0 || which > 5) return BH_ERR_INVALID_ARGUMENT;
  *out = st->v[which].get();
  return BH_OK;
}
bh_status bh_mpc_common_point(const bh_mpc_common* st, int which, uint8_t* out) { return storage_point(st, which, out); }
bh_status bh_mpc_common_contrib_vector(const bh_mpc_common_contrib* c, int which, int mine, const bh_srs** out) {
  return contrib_vector(c, which, mine, out);
}
bh_status bh_mpc_common_contrib_point(const bh_mpc_common_contrib* c, int which, uint8_t* out) {
  return contrib_point(c, which, out);
}

bh_status bh_mpc_common_write(const bh_mpc_common* st, uint8_t* out, size_t cap, size_t* written) {
  return storage_bytes(st, true, false, out, cap, written);
}
bh_status bh_mpc_common_write_compressed(const bh_mpc_common* st, uint8_t* out, size_t cap, size_t* written) {
  return storage_bytes(st, true, true, out, cap, written);
}
bh_status bh_mpc_common_read(bh_ctx* ctx, const uint8_t* bytes, size_t len, int checked, bh_mpc_common** out) {
  return storage_parse(ctx, bytes, len, checked, true, false, out);
}
bh_status bh_mpc_common_read_compressed(bh_ctx* ctx, const uint8_t* bytes, size_t len, int checked,
                                        bh_mpc_common** out) {
  return storage_parse(ctx, bytes, len, checked, true, true, out);
}
bh_status bh_mpc_common_contrib_write(const bh_mpc_common_contrib* c, uint8_t* out, size_t cap, size_t* written) {
  return contrib_bytes(c, true, false, out, cap, written);
}
bh_status bh_mpc_common_contrib_write_compressed(const bh_mpc_common_contrib* c, uint8_t* out, size_t cap,
                                                 size_t* written) {
  return contrib_bytes(c, true, true, out, cap, written);
}
bh_status bh_mpc_common_contrib_read(bh_ctx* ctx, const uint8_t* bytes, size_t len, int checked,
                                     bh_mpc_common_contrib** out) {
  return contrib_parse(ctx, bytes, len, checked, true, false, out);
}
bh_status bh_mpc_common_contrib_read_compressed(bh_ctx* ctx, const uint8_t* bytes, size_t len, int checked,
                                                bh_mpc_common_contrib** out) {
  return contrib_parse(ctx, bytes, len, checked, true, true, out);
}

// ================================================================ round two
bh_status bh_mpc_uncommon_initial(bh_ctx* ctx, const bh_srs* front_g1, const bh_srs* front_g2, const bh_srs* back_g1,
                                  const bh_srs* back_g2, const bh_srs* h_g1, const bh_srs* h_g2,
                                  bh_mpc_uncommon** out) {
  if (!ctx || !out) return BH_ERR_INVALID_ARGUMENT;
  const bh_srs* v[6] = {front_g1, front_g2, back_g1, back_g2, h_g1, h_g2};
  for (int k = 0; k < 6; k++)
    if (!same_device(ctx, v[k]) || v[k]->group != (k & 1 ? BH_G2 : BH_G1)) return BH_ERR_INVALID_ARGUMENT;
  for (int j = 0; j < 3; j++)
    if (v[2 * j]->n != v[2 * j + 1]->n) return BH_ERR_INVALID_ARGUMENT;
  MPC_ENTER(ctx);
  std::unique_ptr<bh_mpc_uncommon> st(new bh_mpc_uncommon());
  st->ctx = ctx;
  for (int k = 0; k < 2; k++) {
    st->p1[k] = g1_gen();
    st->p2[k] = g2_gen();
  }
  for (int k = 0; k < 6; k++)
    if (bh_status s = clone_srs(ctx, v[k], &st->v[k])) return s;
  *out = st.release();
  return BH_OK;
}

bh_status bh_mpc_uncommon_contribute(bh_ctx* ctx, const bh_mpc_uncommon* st, const uint64_t gamma[4],
                                     const uint64_t delta[4], bh_mpc_uncommon_contrib** out) {
  if (!ctx || !st || !out || st->ctx->device != ctx->device) return BH_ERR_INVALID_ARGUMENT;
  if (bh_status s = check_scalars({gamma, delta})) return s;
  MPC_ENTER(ctx);
  std::unique_ptr<bh_mpc_uncommon_contrib> c(new bh_mpc_uncommon_contrib());
  c->ctx = ctx;
  c->pp[0] = new_pair(st->p1[0], st->p2[0], gamma);
  c->pp[1] = new_pair(st->p1[1], st->p2[1], delta);
  Tables tab;
  bh_status s = tab.upload(ctx);
  if (s) return s;
  const uint64_t one[4] = {1, 0, 0, 0};
  const uint64_t* a[3] = {gamma, delta, delta};  // kin, kout, h: mpc.rs:1049-1054, inverted
  for (int j = 0; j < 3; j++)
    if ((s = new_tau_pair(ctx, tab, st, j, a[j], one, 1, c.get()))) return s;
  *out = c.release();
  return BH_OK;
}

bh_status bh_mpc_uncommon_verify(bh_ctx* ctx, const bh_mpc_uncommon* matrix, const bh_mpc_uncommon* st,
                                 const bh_mpc_uncommon_contrib* c, const uint64_t* z, size_t z_len, int* valid,
                                 bh_mpc_uncommon** next) {
  if (!ctx || !matrix || !st || !c || !valid || !next) return BH_ERR_INVALID_ARGUMENT;
  if (matrix->ctx->device != ctx->device || st->ctx->device != ctx->device || c->ctx->device != ctx->device)
    return BH_ERR_INVALID_ARGUMENT;
  *valid = 0;
  *next = nullptr;
  size_t maxlen = 0;
  for (int j = 0; j < 3; j++) maxlen = std::max(maxlen, st->v[2 * j]->n);
  if (z_len < maxlen || (maxlen && !z)) return BH_ERR_INVALID_ARGUMENT;
  MPC_ENTER(ctx);
  DevBuf d_z;
  int nbits = 1;
  bh_status s = upload_z(ctx, z, maxlen, &d_z, &nbits);
  if (s) return s;
  // the reference indexes the contribution's and the matrix' lists with the storage's lengths
  // (mpc.rs:1089-1123)
  for (int k = 0; k < 6; k++)
    if (c->res[k]->n != st->v[k]->n || c->mine[k]->n != st->v[k]->n || matrix->v[k]->n != st->v[k]->n) return BH_OK;
  bool ok = verify_pair(c->pp[1], st->p1[1]) && verify_pair(c->pp[0], st->p1[0]);  // delta, gamma: mpc.rs:1082-1086
  const AffinePt<Fp2> ng2 = pt_neg(g2_gen());
  for (int j = 0; j < 3 && ok; j++) {
    // e(sum z_i new_i, gamma_or_delta_g2) == e(sum z_i matrix_i, G2)
    AffinePt<Fp> sn, sm;
    if ((s = msm(ctx, c->res[2 * j].get(), d_z.as<uint32_t>(), &sn))) return s;
    if ((s = msm(ctx, matrix->v[2 * j].get(), d_z.as<uint32_t>(), &sm))) return s;
    ok = pairing_product_is_one({{sn, c->pp[j == 0 ? 0 : 1].r2}, {sm, ng2}});
  }
  if (!ok) return BH_OK;
  if ((s = to_storage(ctx, c, next))) return s;
  *valid = 1;
  return BH_OK;
}

bh_status bh_mpc_uncommon_free(bh_mpc_uncommon* st) {
  delete st;
  return BH_OK;
}
bh_status bh_mpc_uncommon_contrib_free(bh_mpc_uncommon_contrib* c) {
  delete c;
  return BH_OK;
}
bh_status bh_mpc_uncommon_vector(const bh_mpc_uncommon* st, int which, const bh_srs** out) {
  if (!st || !out || which < 0 || which > 5) return BH_ERR_INVALID_ARGUMENT;
  *out = st->v[which].get();
  return BH_OK;
}
bh_status bh_mpc_uncommon_point(const bh_mpc_uncommon* st, int which, uint8_t* out) {
  return storage_point(st, which, out);
}
bh_status bh_mpc_uncommon_contrib_vector(const bh_mpc_uncommon_contrib* c, int which, int mine, const bh_srs** out) {
  return contrib_vector(c, which, mine, out);
}
bh_status bh_mpc_uncommon_contrib_point(const bh_mpc_uncommon_contrib* c, int which, uint8_t* out) {
  return contrib_point(c, which, out);
}
bh_status bh_mpc_uncommon_write(const bh_mpc_uncommon* st, uint8_t* out, size_t cap, size_t* written) {
  return storage_bytes(st, false, false, out, cap, written);
}
bh_status bh_mpc_uncommon_write_compressed(const bh_mpc_uncommon* st, uint8_t* out, size_t cap, size_t* written) {
  return storage_bytes(st, false, true, out, cap, written);
}
bh_status bh_mpc_uncommon_read(bh_ctx* ctx, const uint8_t* bytes, size_t len, int checked, bh_mpc_uncommon** out) {
  return storage_parse(ctx, bytes, len, checked, false, false, out);
}
bh_status bh_mpc_uncommon_read_compressed(bh_ctx* ctx, const uint8_t* bytes, size_t len, int checked,
                                          bh_mpc_uncommon** out) {
  return storage_parse(ctx, bytes, len, checked, false, true, out);
}
bh_status bh_mpc_uncommon_contrib_write(const bh_mpc_uncommon_contrib* c, uint8_t* out, size_t cap, size_t* written) {
  return contrib_bytes(c, false, false, out, cap, written);
}
bh_status bh_mpc_uncommon_contrib_write_compressed(const bh_mpc_uncommon_contrib* c, uint8_t* out, size_t cap,
                                                   size_t* written) {
  return contrib_bytes(c, false, true, out, cap, written);
}
bh_status bh_mpc_uncommon_contrib_read(bh_ctx* ctx, const uint8_t* bytes, size_t len, int checked,
                                       bh_mpc_uncommon_contrib** out) {
  return contrib_parse(ctx, bytes, len, checked, false, false, out);
}
bh_status bh_mpc_uncommon_contrib_read_compressed(bh_ctx* ctx, const uint8_t* bytes, size_t len, int checked,
                                                  bh_mpc_uncommon_contrib** out) {
  return contrib_parse(ctx, bytes, len, checked, false, true, out);
}

// ================================================================ between the rounds
// CommonParamterInStorage::matrix (mpc.rs:597-645) for any circuit: the Lagrange basis from the
// inverse transforms of the six vectors' first m elements, the circuit's matrices applied to it
// (group_fft.hip), and matrixed_h.  The transforms leave the 1/m to the product's coefficients.
bh_status bh_mpc_common_matrix(bh_ctx* ctx, const bh_mpc_common* st, const bh_r1cs* r, bh_mpc_matrix** out) {
  if (!ctx || !st || !r || !out || st->ctx->device != ctx->device || r->device != ctx->device)
    return BH_ERR_INVALID_ARGUMENT;
  const size_t m = r->m;
  if (m < 2 || st->v[0]->n / 2 < m) return BH_ERR_INVALID_ARGUMENT;
  MPC_ENTER(ctx);
  std::vector<AffinePt<Fp>> first;
  bh_status s = download_points<G1Host>(*st->v[0], 1, &first);
  if (s) return s;
  uint8_t got[G1Host::WIRE], want[G1Host::WIRE];
  to_uncompressed(first[0], got);
  to_uncompressed(g1_gen(), want);
  if (first[0].infinity || memcmp(got, want, sizeof got)) return BH_ERR_INVALID_ARGUMENT;  // mpc.rs:632
  std::unique_ptr<bh_mpc_matrix> mx(new bh_mpc_matrix());
  mx->ctx = ctx;
  mx->m = m;
  mx->ni = r->ni;
  mx->na = r->na;
  for (auto& v : mx->v) v.reset(new bh_srs());
  bh_srs lag[6];
  const bh_srs* lagp[6];
  for (double& x : g_matrix_ms) x = 0;
  auto t0 = std::chrono::steady_clock::now();
  for (int k = 0; k < 6; k++) {
    if ((s = group_fft(ctx, st->v[k].get(), m, 1, false, &lag[k]))) return s;
    lagp[k] = &lag[k];
  }
  bh_srs* prod[7] = {mx->v[BH_MPC_KIN_G1].get(),  mx->v[BH_MPC_KIN_G2].get(),   mx->v[BH_MPC_KOUT_G1].get(),
                     mx->v[BH_MPC_KOUT_G2].get(), mx->v[BH_MPC_MATRIX_A].get(), mx->v[BH_MPC_MATRIX_B_G1].get(),
                     mx->v[BH_MPC_MATRIX_B_G2].get()};
  g_matrix_ms[0] = ms_since(t0);
  t0 = std::chrono::steady_clock::now();
  if ((s = matrix_product(ctx, r, lagp, prod))) return s;
  g_matrix_ms[1] = ms_since(t0);
  t0 = std::chrono::steady_clock::now();
  if ((s = varbase_sub(ctx, st->v[0].get(), 0, m, m, mx->v[BH_MPC_H_G1].get()))) return s;
  if ((s = varbase_sub(ctx, st->v[1].get(), 0, m, m, mx->v[BH_MPC_H_G2].get()))) return s;
  g_matrix_ms[2] = ms_since(t0);
  *out = mx.release();
  return BH_OK;
}

bh_status bh_mpc_matrix_vector(const bh_mpc_matrix* mx, int which, const bh_srs** out) {
  if (!mx || !out || which < 0 || which > 8) return BH_ERR_INVALID_ARGUMENT;
  *out = mx->v[which].get();
  return BH_OK;
}
bh_status bh_mpc_matrix_free(bh_mpc_matrix* mx) {
  delete mx;
  return BH_OK;
}

// generate_parameters_mpc (generator.rs:207-236) with the queries filled in
bh_status bh_mpc_parameters(bh_ctx* ctx, const bh_mpc_common* round1, const bh_mpc_matrix* mx,
                            const bh_mpc_uncommon* round2, bh_params** out) {
  if (!ctx || !round1 || !mx || !round2 || !out) return BH_ERR_INVALID_ARGUMENT;
  if (round1->ctx->device != ctx->device || mx->ctx->device != ctx->device || round2->ctx->device != ctx->device)
    return BH_ERR_INVALID_ARGUMENT;
  const size_t want[3] = {mx->ni, mx->na, mx->m};
  for (int j = 0; j < 3; j++)
    if (round2->v[2 * j]->n != want[j] || round2->v[2 * j + 1]->n != want[j]) return BH_ERR_INVALID_ARGUMENT;
  MPC_ENTER(ctx);
  std::unique_ptr<bh_params> p(new bh_params());
  p->ctx = ctx;
  p->alpha_g1 = round1->p1[0];
  p->beta_g1 = round1->p1[1];
  p->beta_g2 = round1->p2[1];
  p->gamma_g2 = round2->p2[0];
  p->delta_g1 = round2->p1[1];
  p->delta_g2 = round2->p2[1];
  bh_status s = download(round2->v[BH_MPC_KIN_G1].get(), &p->ic);
  if (s) return s;
  const struct { const bh_srs* src; size_t n; bh_srs* dst; } q[5] = {
      {round2->v[BH_MPC_H_G1].get(), mx->m - 1, &p->h},
      {round2->v[BH_MPC_KOUT_G1].get(), mx->na, &p->l},
      {mx->v[BH_MPC_MATRIX_A].get(), mx->v[BH_MPC_MATRIX_A]->n, &p->a},
      {mx->v[BH_MPC_MATRIX_B_G1].get(), mx->v[BH_MPC_MATRIX_B_G1]->n, &p->b_g1},
      {mx->v[BH_MPC_MATRIX_B_G2].get(), mx->v[BH_MPC_MATRIX_B_G2]->n, &p->b_g2}};
  for (const auto& x : q) {
    const size_t bytes = x.n * with_group(x.src->group, [](auto g) { return decltype(g)::WORDS * (size_t)4; });
    x.dst->ctx = ctx;
    x.dst->group = x.src->group;
    x.dst->n = x.n;
    BH_TRY_HIP(x.dst->pts.alloc(std::max<size_t>(bytes, 16)));
    if (bytes) BH_TRY_HIP(hipMemcpyAsync(x.dst->pts.p, x.src->pts.p, bytes, hipMemcpyDeviceToDevice, ctx->stream));
  }
  BH_TRY_HIP(hipStreamSynchronize(ctx->stream));
  *out = p.release();
  return BH_OK;
}

// ================================================================ Parameters against circuit and storage
// DESIGN.md section 19.  The scalars are params_check.hip's, resident; the multiexps msm_device's
// on them, one after another on the context's stream; the pairings the host pool's, as in
// structure_mask.  generator.rs:520-572 (the queries), 614-633 (the identity filter)
bh_status bh_params_check(bh_ctx* ctx, const bh_params* p, const bh_r1cs* r, const bh_mpc_common* st,
                          const uint64_t rho[4], const uint64_t sigma[4], int* valid, uint32_t* failed) {
  if (!ctx || !p || !r || !st || !valid || !check_weight(rho) || !check_weight(sigma)) return BH_ERR_INVALID_ARGUMENT;
  if (!p->ctx || p->ctx->device != ctx->device || r->device != ctx->device || st->ctx->device != ctx->device)
    return BH_ERR_INVALID_ARGUMENT;
  const size_t m = r->m, ni = r->ni, na = r->na;
  if (m < 2 || st->v[0]->n < 2 * m) return BH_ERR_INVALID_ARGUMENT;
  *valid = 0;
  if (failed) *failed = 0;
  MPC_ENTER(ctx);
  for (double& x : g_pcheck_ms) x = 0;
  uint32_t mask = 0;
  auto done = [&] {
    if (failed) *failed = mask;
    *valid = mask == 0;
    return BH_OK;
  };
  if (p->ic.size() != ni || p->l.n != na || p->h.n != m - 1 || p->b_g1.n != p->b_g2.n) {
    mask = BH_PARAMS_CHECK_SIZES;
    return done();
  }
  auto t0 = std::chrono::steady_clock::now();
  ParamsCheckScalars sc;
  bh_status s = params_check_scalars(ctx, r, fr_from_canonical(rho), fr_from_canonical(sigma), &sc);
  if (s) return s;
  g_pcheck_ms[0] = ms_since(t0);
  if (p->a.n != sc.n_a || p->b_g1.n != sc.n_b) {
    mask = BH_PARAMS_CHECK_SIZES;
    return done();
  }
  // ---- the multiexps: 13 in G1 (14 with ic's), 2 in G2
  t0 = std::chrono::steady_clock::now();
  const bh_srs *T = st->v[0].get(), *T2 = st->v[1].get(), *AT = st->v[2].get(), *BT = st->v[4].get();
  auto g1 = [&](const bh_srs* b, const uint32_t* d, size_t len, Jac<Fp>* o) {
    return msm_device<G1Host>(ctx, b, 0, d, len, nullptr, o, nullptr);
  };
  auto g2 = [&](const bh_srs* b, const uint32_t* d, size_t len, Jac<Fp2>* o) {
    return msm_device<G2Host>(ctx, b, 0, d, len, nullptr, o, nullptr);
  };
  const uint32_t* w = sc.w.as<uint32_t>();
  const uint32_t* hw = sc.hw.as<uint32_t>();
  Jac<Fp> a_l, a_r, b1_l, b1_r, l_l, ic_l, h_l, h_r, k[2];
  Jac<Fp2> b2_l, b2_r;
  // the left-hand sides, over the Parameters
  if ((s = g1(&p->a, sc.wa.as<uint32_t>(), sc.n_a, &a_l))) return s;
  if ((s = g1(&p->b_g1, sc.wb.as<uint32_t>(), sc.n_b, &b1_l))) return s;
  if ((s = g2(&p->b_g2, sc.wb.as<uint32_t>(), sc.n_b, &b2_l))) return s;
  if ((s = g1(&p->l, w + ni * 8, na, &l_l))) return s;
  if ((s = g1(&p->h, hw + m * 8, m - 1, &h_l))) return s;
  {
    // ic lives on the host.  An identity among it (a zero ic scalar, which the generator writes as
    // one) has no device record: the generator stands in for it and its share is taken off again
    std::vector<AffinePt<Fp>> ic = p->ic;
    Jac<Fp> off = jac_identity<Fp>();
    const Fr rho_fr = fr_from_canonical(rho);
    for (size_t j = 0; j < ni; j++) {
      if (!ic[j].infinity) continue;
      ic[j] = g1_gen();
      const uint64_t e = j;
      uint64_t wj[4];
      fr_to_canonical(pow_vartime(rho_fr, &e, 1), wj);
      off = jac_add(off, jac_mul(jac_from_affine(pt_neg(g1_gen())), wj, 4));
    }
    bh_srs d_ic;
    if ((s = srs_upload_affine(ctx, ic.data(), ni, &d_ic))) return s;
    if ((s = g1(&d_ic, w, ni, &ic_l))) return s;
    ic_l = jac_add(ic_l, off);
  }
  // the right-hand sides, over the storage
  const uint32_t* cw = sc.coef[0].as<uint32_t>();
  if ((s = g1(T, cw, m, &a_r))) return s;
  if ((s = g1(T, cw + m * 8, m, &b1_r))) return s;
  if ((s = g2(T2, cw + m * 8, m, &b2_r))) return s;
  if ((s = g1(T, hw, 2 * m, &h_r))) return s;
  for (int z = 0; z < 2; z++) {  // K(w), K(w_in) = <BT, c_A> + <AT, c_B> + <T, c_C>
    const uint32_t* c = sc.coef[z].as<uint32_t>();
    const bh_srs* base[3] = {BT, AT, T};
    k[z] = jac_identity<Fp>();
    for (int v = 0; v < 3; v++) {
      Jac<Fp> part;
      if ((s = g1(base[v], c + (size_t)v * m * 8, m, &part))) return s;
      k[z] = jac_add(k[z], part);
    }
  }
  const AffinePt<Fp> k_in = jac_to_affine(k[1]);
  const AffinePt<Fp> k_aux = jac_to_affine(jac_add(k[0], jac_from_affine(pt_neg(k_in))));
  g_pcheck_ms[1] = ms_since(t0);
  // ---- bytes, point equalities, pairings
  t0 = std::chrono::steady_clock::now();
  if (!same_bytes(p->alpha_g1, st->p1[0])) mask |= BH_PARAMS_CHECK_ALPHA;
  if (!same_bytes(p->beta_g1, st->p1[1]) || !same_bytes(p->beta_g2, st->p2[1])) mask |= BH_PARAMS_CHECK_BETA;
  if (p->gamma_g2.infinity || p->delta_g2.infinity) mask |= BH_PARAMS_CHECK_DELTA;
  if (!same_bytes(jac_to_affine(a_l), jac_to_affine(a_r))) mask |= BH_PARAMS_CHECK_A;
  if (!same_bytes(jac_to_affine(b1_l), jac_to_affine(b1_r))) mask |= BH_PARAMS_CHECK_B_G1;
  if (!same_bytes(jac_to_affine(b2_l), jac_to_affine(b2_r))) mask |= BH_PARAMS_CHECK_B_G2;
  const AffinePt<Fp2> ng2 = pt_neg(g2_gen());
  const std::vector<Equation> eq = {
      {BH_PARAMS_CHECK_DELTA, {{p->delta_g1, ng2}, {g1_gen(), p->delta_g2}}},
      {BH_PARAMS_CHECK_L, {{jac_to_affine(l_l), p->delta_g2}, {k_aux, ng2}}},
      {BH_PARAMS_CHECK_IC, {{jac_to_affine(ic_l), p->gamma_g2}, {k_in, ng2}}},
      {BH_PARAMS_CHECK_H, {{jac_to_affine(h_l), p->delta_g2}, {jac_to_affine(h_r), ng2}}}};
  std::vector<char> bad(eq.size(), 0);  // every equation is evaluated: the mask is complete
  ctx_pool(ctx).parallel_for((int)eq.size(), [&](int i) { bad[i] = !pairing_product_is_one(eq[i].pairs); });
  for (size_t i = 0; i < eq.size(); i++)
    if (bad[i]) mask |= eq[i].bit;
  g_pcheck_ms[2] = ms_since(t0);
  return done();
}

// wall time (ms) of this thread's last bh_params_check: the scalar side, the multiexps, the pairings
void bh_params_last_check_ms(double out[3]) {
  for (int i = 0; i < 3; i++) out[i] = g_pcheck_ms[i];
}

// wall time (ms) of the per-element Miller loops of this thread's last bh_mpc_common_verify, and
// how many of its vector pairs ran them on the device
void bh_mpc_last_matrix_ms(double out[3]) {
  for (int k = 0; k < 3; k++) out[k] = g_matrix_ms[k];
}
// wall time (ms) of this thread's last structure check: the weights and multiexps, the pairings
void bh_mpc_last_check_ms(double out[2]) {
  for (int k = 0; k < 2; k++) out[k] = g_check_ms[k];
}
double bh_mpc_last_miller_ms(void) { return g_miller_ms; }
int bh_mpc_last_miller_device(void) { return g_miller_device; }

}  // extern "C"
