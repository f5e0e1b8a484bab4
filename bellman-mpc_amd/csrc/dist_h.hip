// Distributed H pipeline: see dist_h.h for the data distribution.  Restates, split over N
// ranks, the H block of create_proof (reference src/groth16/prover.rs:210-231):
//   a, b, c: ifft, coset_fft (domain.rs:81-99, 101-125); a*b - c; divide_by_z_on_coset
//   (domain.rs:139-151); icoset_fft.
// As on one device (run_h_vector, api.hip), c takes only its ifft: with K = 1/Z(g),
//   h = icoset_fft(A o B K) - ifft(c) K,
// so c leaves the pipeline after the first exchange: k_dist_mid keeps c' = ifft(c) K for this
// rank's q chunk (the index set k_dist_final writes h for), the second exchange carries a and b
// only (2*M*32 bytes per rank instead of 3*M*32), and k_dist_final subtracts c'.
//
// Index algebra (m = N*M, omega of order m, n = N*j + r, k = M*t + q):
//   inverse  X[M t + q] = sum_r w_N^(-r t) * w^(-r q) * Y_r[q],  Y_r = iNTT_M(x[N j + r])
//   forward  V[N j + r] = NTT_M over q of  w^(q r) * sum_t w_N^(t r) * v[M t + q]
// so each transform is a local M-point NTT (existing LDS passes), an all-to-all of C = M/N
// element chunks and, per q, an N-point DFT with the w^(+-q r) twiddles, done in registers.
//
// Operand contract: every packed value k_dist_mid and k_dist_final load (the exchanged chunks and
// cprime) is below 2r, which the local NTT's stores guarantee; every packed value they store (work's
// a and b rows, cprime) is below 2r again, and hbuf holds canonical scalars (below r).  The N-point
// DFT keeps that bound by one conditional subtraction of 2r per butterfly output, and geometric()
// passes x[0] through as loaded.  bh_selftest_dist_h (the whole pipeline with N virtual ranks on one
// stream) and bh_selftest_dist_stage (one rank's one kernel on chosen packed words) at the end of
// this file let tests/test_gpu_dist_h.py hold the kernels to it against tests/dist_h_model.py.
#include "dist_h.h"
#include "ntt_common.cuh"

namespace bh {

struct DistArgs {
  uint32_t M, C, rank, m_minus_1;
  const uint32_t* tw_fwd;  // omega^j, j < m/2 (domain of size m, unpacked)
  const uint32_t* tw_inv;
  const uint32_t* sc_lo;   // power table over the global index k (g^k m^-1 or g^-k m^-1): split, or
  const uint32_t* sc_hi;   // full in sc_hi (sc_bits = POW_FULL_TABLE, pow_factor)
  int sc_bits;
  const uint32_t* ck;      // m^-1 / Z(g) (9 limbs): c's ifft scale (k_dist_mid)
  uint32_t* cprime;        // c' = ifft(c) / Z(g) at [t*C + u] for k = t*M + q (hbuf's layout), M elements
  uint32_t wN[16][9], wNinv[16][9];  // w_N^k, w_N^-k (device Montgomery limbs)
};

template <int N>
__device__ __forceinline__ DFr wconst(const uint32_t (&w)[16][9], int k) {
  DFr r;
#pragma unroll
  for (int l = 0; l < 9; l++) r.v[l] = w[k][l];
  return r;
}

// X[k] = sum_j x[j] w^(j k), natural order in and out (radix-2 DIT, fully unrolled)
template <int N>
__device__ __forceinline__ void small_dft(DFr (&x)[N], const uint32_t (&w)[16][9]) {
  constexpr int LOG = N == 2 ? 1 : N == 4 ? 2 : N == 8 ? 3 : 4;
#pragma unroll
  for (int i = 0; i < N; i++) {
    const int j = (int)(__builtin_bitreverse32((uint32_t)i) >> (32 - LOG));
    if (i < j) {
      DFr t = x[i];
      x[i] = x[j];
      x[j] = t;
    }
  }
#pragma unroll
  for (int h = 1; h < N; h <<= 1) {
    const int step = N / (2 * h);
#pragma unroll
    for (int s = 0; s < N; s += 2 * h) {
#pragma unroll
      for (int jj = 0; jj < h; jj++) {
        const DFr t = jj == 0 ? x[s + jj + h] : fe_mul<FrCfg>(x[s + jj + h], wconst<N>(w, jj * step));
        const DFr u = x[s + jj];
        x[s + jj] = fe_csub<FrCfg, 2>(fe_add<FrCfg>(u, t));
        x[s + jj + h] = fe_csub<FrCfg, 2>(fe_sub<FrCfg, 2>(u, t));
      }
    }
  }
}

// x[r] *= s^r for r < N
template <int N>
__device__ __forceinline__ void geometric(DFr (&x)[N], const DFr& s) {
  DFr p = s;
#pragma unroll
  for (int r = 1; r < N; r++) {
    x[r] = fe_mul<FrCfg>(x[r], p);
    if (r + 1 < N) p = fe_mul<FrCfg>(p, s);
  }
}

// out[vec*M + brev(j)] = full[vec*m + N*j + r]: this rank's residue class, bit-reversed for DIT
__global__ void __launch_bounds__(256) k_gather_class(const uint32_t* full, uint32_t* out, uint32_t M, int Lm,
                                                      uint32_t N, uint32_t r, uint32_t nvec, size_t m) {
  const size_t gid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= (size_t)nvec * M) return;
  const uint32_t vec = (uint32_t)(gid / M), j = (uint32_t)(gid % M);
  const uint4* src = reinterpret_cast<const uint4*>(full + ((size_t)vec * m + (size_t)N * j + r) * 8);
  uint4* dst = reinterpret_cast<uint4*>(out + ((size_t)vec * M + brev(j, Lm)) * 8);
  dst[0] = src[0];
  dst[1] = src[1];
}

// after exchange 1: received Y_r[q] (r = source rank) for q in this rank's chunk.
// inverse N-DFT over r (with w^(-r q)), scale g^k m^-1 (ifft + distribute_powers), forward
// N-DFT over t (with w^(q r')) -> out[vec*M + r'*C + u], row r' bound for rank r'.
// vec 2 (c) ends after the inverse DFT: scaled by the constant m^-1 / Z(g) into cprime, nothing sent.
template <int N>
__global__ void __launch_bounds__(256) k_dist_mid(const uint32_t* recv, uint32_t* out, DistArgs a, uint32_t nvec) {
  const uint32_t gid = blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= nvec * a.C) return;
  const uint32_t vec = gid / a.C, u = gid % a.C;
  const uint32_t q = a.rank * a.C + u;
  const size_t base = (size_t)vec * a.M + u;
  DFr x[N];
#pragma unroll
  for (int r = 0; r < N; r++) x[r] = ld_packed(recv, base + (size_t)r * a.C);
  geometric<N>(x, ld_limbs(a.tw_inv, q));
  small_dft<N>(x, a.wNinv);
  if (vec == 2) {
    const DFr ck = ld_limbs(a.ck, 0);
#pragma unroll
    for (int t = 0; t < N; t++) st_packed(a.cprime, (size_t)t * a.C + u, fe_mul<FrCfg>(x[t], ck));
    return;
  }
#pragma unroll
  for (int t = 0; t < N; t++) x[t] = fe_mul<FrCfg>(x[t], pow_factor(a.sc_lo, a.sc_hi, a.sc_bits, t * a.M + q));
  small_dft<N>(x, a.wN);
  geometric<N>(x, ld_limbs(a.tw_fwd, q));
#pragma unroll
  for (int r = 0; r < N; r++) st_packed(out, base + (size_t)r * a.C, x[r]);
}

// after exchange 3: inverse N-DFT over r, scale g^-k m^-1 (icoset), minus c', canonical scalars of
// h[M t + q] at hbuf[t*C + u], their global index (-1 for k = m-1: truncation, prover.rs:227)
template <int N>
__global__ void __launch_bounds__(256) k_dist_final(const uint32_t* recv, uint32_t* hbuf, int32_t* hidx,
                                                    DistArgs a) {
  const uint32_t u = blockIdx.x * blockDim.x + threadIdx.x;
  if (u >= a.C) return;
  const uint32_t q = a.rank * a.C + u;
  DFr x[N];
#pragma unroll
  for (int r = 0; r < N; r++) x[r] = ld_packed(recv, u + (size_t)r * a.C);
  geometric<N>(x, ld_limbs(a.tw_inv, q));
  small_dft<N>(x, a.wNinv);
#pragma unroll
  for (int t = 0; t < N; t++) {
    const uint32_t k = t * a.M + q;
    DFr v = fe_mul<FrCfg>(x[t], pow_factor(a.sc_lo, a.sc_hi, a.sc_bits, k));
    v = fe_sub<FrCfg, 2>(v, ld_packed(a.cprime, (size_t)t * a.C + u));  // v < 2r, c' < 2r: < 4r
    v = fe_csub<FrCfg, 1>(fe_from_mont<FrCfg>(v));  // v < 2^261, so v * 2^-261 <= r: one subtraction
    uint32_t w[8];
    fe_pack<FrCfg>(v, w);
    uint4* p = reinterpret_cast<uint4*>(hbuf + ((size_t)t * a.C + u) * 8);
    p[0] = make_uint4(w[0], w[1], w[2], w[3]);
    p[1] = make_uint4(w[4], w[5], w[6], w[7]);
    hidx[(size_t)t * a.C + u] = k == a.m_minus_1 ? -1 : (int32_t)k;
  }
}

// ------------------------------------------------------------------ host side
static int log2i(int n) {
  int l = 0;
  while ((1 << l) < n) l++;
  return l;
}

bool dist_h_eligible(int N, int L) {
  if (N < 2 || N > 16 || (N & (N - 1))) return false;
  return L >= 2 * log2i(N) + 1;
}

bh_status dist_h_init(bh_ctx* ctx, DistH& d, int N, int rank, int L) {
  if (!dist_h_eligible(N, L) || rank < 0 || rank >= N) return BH_ERR_INVALID_ARGUMENT;
  d.N = N;
  d.rank = rank;
  d.L = L;
  d.Lm = L - log2i(N);
  d.M = (size_t)1 << d.Lm;
  d.C = d.M / N;
  BH_TRY_HIP(d.work.alloc(3 * d.M * 32));
  BH_TRY_HIP(d.recv.alloc(3 * d.M * 32));
  BH_TRY_HIP(d.hbuf.alloc(d.M * 32));
  BH_TRY_HIP(d.cprime.alloc(d.M * 32));
  BH_TRY_HIP(d.hidx.alloc(d.M * 4));
  Domain *D, *Dm;
  bh_status s;
  if ((s = ctx_domain(ctx, L, &D)) || (s = ctx_domain(ctx, d.Lm, &Dm))) return s;
  return BH_OK;
}

static bh_status make_args(bh_ctx* ctx, const DistH& d, bool icoset, DistArgs* a) {
  Domain* D;
  bh_status s = ctx_domain(ctx, d.L, &D);
  if (s) return s;
  a->M = (uint32_t)d.M;
  a->C = (uint32_t)d.C;
  a->rank = (uint32_t)d.rank;
  a->m_minus_1 = (uint32_t)(((size_t)1 << d.L) - 1);
  a->tw_fwd = D->tw_fwd.as<uint32_t>();
  a->tw_inv = D->tw_inv.as<uint32_t>();
  // the factors g^(+-k) m^-1 over the global index k: the domain's full tables (one load per element)
  a->sc_lo = nullptr;
  a->sc_hi = icoset ? D->icoset_full.as<uint32_t>() : D->coset_full.as<uint32_t>();
  a->sc_bits = POW_FULL_TABLE;
  a->ck = D->consts.as<uint32_t>() + 27;
  a->cprime = d.cprime.as<uint32_t>();
  // w_N = root_of_unity^(2^(32 - log N))  (the same root as domain.rs:62-66, of order N)
  uint64_t rou_raw[4] = {0x3829971f439f0d2bull, 0xb63683508c2280b9ull, 0xd09b681922c813b4ull, 0x16a2a19edfe81f20ull};
  Fr w = from_int<4>(rou_raw);
  for (int i = log2i(d.N); i < 32; i++) w = sqr(w);
  const Fr winv = inv(w);
  Fr p = Fr::one(), pi = Fr::one();
  for (int k = 0; k < 16; k++) {
    fr_to_dev_limbs(p, a->wN[k]);
    fr_to_dev_limbs(pi, a->wNinv[k]);
    p = mul(p, w);
    pi = mul(pi, winv);
  }
  return BH_OK;
}

static inline unsigned blocks(size_t n, unsigned bs) { return (unsigned)((n + bs - 1) / bs); }

bh_status dist_h_phase1(bh_ctx* ctx, DistH& d, const uint32_t* abc_full, hipStream_t st) {
  Domain* Dm;
  bh_status s = ctx_domain(ctx, d.Lm, &Dm);
  if (s) return s;
  const size_t m = (size_t)1 << d.L;
  hipLaunchKernelGGL(k_gather_class, dim3(blocks(3 * d.M, 256)), dim3(256), 0, st, abc_full, d.work.as<uint32_t>(),
                     (uint32_t)d.M, d.Lm, (uint32_t)d.N, (uint32_t)d.rank, 3u, m);
  // Y_r = iNTT_M of the residue class: DIT (bit-reversed in, natural out), omega_M^-1
  for (int v = 0; v < 3; v++)
    launch_ntt(d.work.as<uint32_t>() + v * d.M * 8, d.Lm, false, Dm->lv_inv.as<uint32_t>(), nullptr, nullptr, 0, st);
  BH_TRY_HIP(hipGetLastError());
  return BH_OK;
}

template <int N>
static void launch_mid(const DistH& d, const DistArgs& a, hipStream_t st) {
  hipLaunchKernelGGL(k_dist_mid<N>, dim3(blocks(3 * d.C, 256)), dim3(256), 0, st, d.recv.as<uint32_t>(),
                     d.work.as<uint32_t>(), a, 3u);
}
template <int N>
static void launch_final(const DistH& d, const DistArgs& a, hipStream_t st) {
  hipLaunchKernelGGL(k_dist_final<N>, dim3(blocks(d.C, 256)), dim3(256), 0, st, d.work.as<uint32_t>(),
                     d.hbuf.as<uint32_t>(), d.hidx.as<int32_t>(), a);
}

bh_status dist_h_phase2(bh_ctx* ctx, DistH& d, hipStream_t st) {
  DistArgs a;
  bh_status s = make_args(ctx, d, false, &a);
  if (s) return s;
  switch (d.N) {
    case 2: launch_mid<2>(d, a, st); break;
    case 4: launch_mid<4>(d, a, st); break;
    case 8: launch_mid<8>(d, a, st); break;
    case 16: launch_mid<16>(d, a, st); break;
    default: return BH_ERR_INVALID_ARGUMENT;
  }
  BH_TRY_HIP(hipGetLastError());
  return BH_OK;
}

bh_status dist_h_phase3(bh_ctx* ctx, DistH& d, hipStream_t st) {
  Domain *D, *Dm;
  bh_status s;
  if ((s = ctx_domain(ctx, d.L, &D)) || (s = ctx_domain(ctx, d.Lm, &Dm))) return s;
  uint32_t* a = d.recv.as<uint32_t>();
  uint32_t* b = a + d.M * 8;
  // coset_fft's local M-point NTTs: DIF (natural q in, bit-reversed j out), omega_M
  for (uint32_t* x : {a, b}) launch_ntt(x, d.Lm, true, Dm->lv_fwd.as<uint32_t>(), nullptr, nullptr, 0, st);
  // a*b, divide_by_z_on_coset (order-agnostic: the two vectors share the layout)
  launch_pointwise(a, b, nullptr, d.M, 3, D->consts.as<uint32_t>() + 9, st);
  // icoset_fft's local iNTT_M: DIT (bit-reversed j in, natural q out), omega_M^-1
  launch_ntt(a, d.Lm, false, Dm->lv_inv.as<uint32_t>(), nullptr, nullptr, 0, st);
  BH_TRY_HIP(hipGetLastError());
  return BH_OK;
}

bh_status dist_h_final(bh_ctx* ctx, DistH& d, hipStream_t st) {
  DistArgs a;
  bh_status s = make_args(ctx, d, true, &a);
  if (s) return s;
  switch (d.N) {
    case 2: launch_final<2>(d, a, st); break;
    case 4: launch_final<4>(d, a, st); break;
    case 8: launch_final<8>(d, a, st); break;
    case 16: launch_final<16>(d, a, st); break;
    default: return BH_ERR_INVALID_ARGUMENT;
  }
  BH_TRY_HIP(hipGetLastError());
  return BH_OK;
}

bh_status dist_h_run(bh_ctx* ctx, DistH& d, const uint32_t* abc_full, const HExchange& ex, hipStream_t st) {
  bh_status s;
  if ((s = dist_h_phase1(ctx, d, abc_full, st))) return s;
  if ((s = ex(d.work.as<uint32_t>(), d.recv.as<uint32_t>(), 3, st))) return s;
  if ((s = dist_h_phase2(ctx, d, st))) return s;
  if ((s = ex(d.work.as<uint32_t>(), d.recv.as<uint32_t>(), 2, st))) return s;  // a and b: c ended in phase 2
  if ((s = dist_h_phase3(ctx, d, st))) return s;
  if ((s = ex(d.recv.as<uint32_t>(), d.work.as<uint32_t>(), 1, st))) return s;
  return dist_h_final(ctx, d, st);
}

void dist_kernels(std::vector<KernInfo>& v) {
  v.push_back({"k_dist_mid<2>", (const void*)k_dist_mid<2>, 256, 0});
  v.push_back({"k_dist_mid<4>", (const void*)k_dist_mid<4>, 256, 0});
  v.push_back({"k_dist_mid<8>", (const void*)k_dist_mid<8>, 256, 0});
  v.push_back({"k_dist_mid<16>", (const void*)k_dist_mid<16>, 256, 0});
  v.push_back({"k_dist_final<2>", (const void*)k_dist_final<2>, 256, 0});
  v.push_back({"k_dist_final<4>", (const void*)k_dist_final<4>, 256, 0});
  v.push_back({"k_dist_final<8>", (const void*)k_dist_final<8>, 256, 0});
  v.push_back({"k_dist_final<16>", (const void*)k_dist_final<16>, 256, 0});
}

// ------------------------------------------------------------------ self-tests (api_internal.h)
namespace {

// LocalExchanger's rule (prover.hip) between the virtual ranks of one stream: chunk r of rank p's
// send buffer -> chunk p of rank r's receive buffer, for nvec vectors of stride M
bh_status selftest_exchange(std::vector<DistH>& d, bool work_to_recv, int nvec, hipStream_t st) {
  const size_t N = d.size(), M = d[0].M, C = d[0].C;
  for (size_t r = 0; r < N; r++)
    for (size_t p = 0; p < N; p++)
      for (int v = 0; v < nvec; v++) {
        const uint32_t* send = (work_to_recv ? d[p].work : d[p].recv).as<uint32_t>();
        uint32_t* recv = (work_to_recv ? d[r].recv : d[r].work).as<uint32_t>();
        BH_TRY_HIP(hipMemcpyAsync(recv + ((size_t)v * M + p * C) * 8, send + ((size_t)v * M + r * C) * 8, C * 32,
                                  hipMemcpyDeviceToDevice, st));
      }
  return BH_OK;
}

bh_status selftest_pipeline(bh_ctx* ctx, const uint64_t* a, const uint64_t* b, const uint64_t* c, size_t m, int N,
                            int L, uint32_t* h_out, int32_t* idx_out) {
  hipStream_t st = ctx->stream;
  DevBuf abc;
  BH_TRY_HIP(abc.alloc(3 * m * 32));
  std::vector<DistH> d(N);
  bh_status s;
  for (int r = 0; r < N; r++)
    if ((s = dist_h_init(ctx, d[r], N, r, L))) return s;
  uint32_t* full = abc.as<uint32_t>();
  if ((s = upload_fr(ctx, a, m, m, full)) || (s = upload_fr(ctx, b, m, m, full + m * 8)) ||
      (s = upload_fr(ctx, c, m, m, full + 2 * m * 8)))
    return s;
  for (int r = 0; r < N; r++)
    if ((s = dist_h_phase1(ctx, d[r], full, st))) return s;
  if ((s = selftest_exchange(d, true, 3, st))) return s;
  for (int r = 0; r < N; r++)
    if ((s = dist_h_phase2(ctx, d[r], st))) return s;
  if ((s = selftest_exchange(d, true, 2, st))) return s;
  for (int r = 0; r < N; r++)
    if ((s = dist_h_phase3(ctx, d[r], st))) return s;
  if ((s = selftest_exchange(d, false, 1, st))) return s;
  for (int r = 0; r < N; r++)
    if ((s = dist_h_final(ctx, d[r], st))) return s;
  const size_t M = d[0].M;
  for (int r = 0; r < N; r++) {
    BH_TRY_HIP(hipMemcpyAsync(h_out + (size_t)r * M * 8, d[r].hbuf.p, M * 32, hipMemcpyDeviceToHost, st));
    BH_TRY_HIP(hipMemcpyAsync(idx_out + (size_t)r * M, d[r].hidx.p, M * 4, hipMemcpyDeviceToHost, st));
  }
  BH_TRY_HIP(hipStreamSynchronize(st));
  return BH_OK;
}

bh_status selftest_stage(bh_ctx* ctx, int L, int N, int rank, int stage, const uint32_t* recv, const uint32_t* cprime,
                         uint32_t* out, uint32_t* out2) {
  hipStream_t st = ctx->stream;
  DistH d;
  bh_status s = dist_h_init(ctx, d, N, rank, L);
  if (s) return s;
  const size_t M = d.M;
  // what the kernel is to write starts as all ones: a slot it left alone is not below 2r
  BH_TRY_HIP(hipMemsetAsync(d.cprime.p, 0xFF, M * 32, st));
  if (stage == 0) {
    BH_TRY_HIP(hipMemcpyAsync(d.recv.p, recv, 3 * M * 32, hipMemcpyHostToDevice, st));
    BH_TRY_HIP(hipMemsetAsync(d.work.p, 0xFF, 3 * M * 32, st));
    if ((s = dist_h_phase2(ctx, d, st))) return s;
    BH_TRY_HIP(hipMemcpyAsync(out, d.work.p, 2 * M * 32, hipMemcpyDeviceToHost, st));
    BH_TRY_HIP(hipMemcpyAsync(out2, d.cprime.p, M * 32, hipMemcpyDeviceToHost, st));
  } else {
    BH_TRY_HIP(hipMemcpyAsync(d.work.p, recv, M * 32, hipMemcpyHostToDevice, st));  // where k_dist_final reads
    BH_TRY_HIP(hipMemcpyAsync(d.cprime.p, cprime, M * 32, hipMemcpyHostToDevice, st));
    BH_TRY_HIP(hipMemsetAsync(d.hbuf.p, 0xFF, M * 32, st));
    BH_TRY_HIP(hipMemsetAsync(d.hidx.p, 0xFF, M * 4, st));
    if ((s = dist_h_final(ctx, d, st))) return s;
    BH_TRY_HIP(hipMemcpyAsync(out, d.hbuf.p, M * 32, hipMemcpyDeviceToHost, st));
    BH_TRY_HIP(hipMemcpyAsync(out2, d.hidx.p, M * 4, hipMemcpyDeviceToHost, st));
  }
  BH_TRY_HIP(hipStreamSynchronize(st));
  return BH_OK;
}

}  // namespace
}  // namespace bh

extern "C" {

bh_status bh_selftest_dist_h(bh_ctx* ctx, const uint64_t* a, const uint64_t* b, const uint64_t* c, size_t m, int nranks,
                             uint32_t* h_out, int32_t* idx_out) {
  using namespace bh;
  if (!ctx || !a || !b || !c || !h_out || !idx_out) return BH_ERR_INVALID_ARGUMENT;
  if (m == 0 || (m & (m - 1)) || m > ((size_t)1 << 30)) return BH_ERR_INVALID_ARGUMENT;
  const int L = log2i((int)m);
  if (!dist_h_eligible(nranks, L)) return BH_ERR_INVALID_ARGUMENT;
  std::lock_guard<std::mutex> lk(ctx->mu);
  BH_TRY_HIP(hipSetDevice(ctx->device));
  bh_status s = scratch_check(ctx);
  if (s) return s;
  s = selftest_pipeline(ctx, a, b, c, m, nranks, L, h_out, idx_out);
  if (s) (void)hipStreamSynchronize(ctx->stream);  // nothing in flight when the ranks' buffers go
  return s;
}

bh_status bh_selftest_dist_stage(bh_ctx* ctx, int log_m, int nranks, int rank, int stage, const uint32_t* recv,
                                 const uint32_t* cprime, uint32_t* out, uint32_t* out2) {
  using namespace bh;
  if (!ctx || !recv || !out || !out2 || (stage == 1 && !cprime)) return BH_ERR_INVALID_ARGUMENT;
  if (stage != 0 && stage != 1) return BH_ERR_INVALID_ARGUMENT;
  if (log_m < 0 || log_m > 30 || !dist_h_eligible(nranks, log_m) || rank < 0 || rank >= nranks)
    return BH_ERR_INVALID_ARGUMENT;
  std::lock_guard<std::mutex> lk(ctx->mu);
  BH_TRY_HIP(hipSetDevice(ctx->device));
  bh_status s = scratch_check(ctx);
  if (s) return s;
  s = selftest_stage(ctx, log_m, nranks, rank, stage, recv, cprime, out, out2);
  if (s) (void)hipStreamSynchronize(ctx->stream);
  return s;
}

}  // extern "C"
