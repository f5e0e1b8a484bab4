// The scalar side of bh_params_check: Parameters are audited against a
// circuit and a round-one storage with random linear combinations, and every combination's
// scalars are made here, on the device, from the two scalars rho and sigma.
//
// What is reused as it is (deliberately: these are the library's, not copies of them):
//   k_r1cs_powers                  rho^j and sigma^i                      (r1cs_powers_device)
//   k_r1cs_segments / _columns / _long   u, v, w at x_i = sigma^i         (r1cs_eval_device)
//   k_r1cs_row_segments + pass 2   A z | B z | C z                        (r1cs_rows_device)
//   the resident ifft              c_M(z), size m, with the 1/m           (device_ifft)
//   k_fr_convert                   device Montgomery -> canonical         (launch_fr_convert)
//   the tiled scan                 positions of the present columns       (exclusive_scan)
// New here, one lane per element, in the style of k_gfft_flags / k_gfft_compact:
//   k_pcheck_flags      fu[j] = u_j != 0, fv[j] = v_j != 0: column j of A / B is present
//   k_pcheck_compact    the canonical w_j of the present columns, order kept
//   k_pcheck_split      z_in = w on the inputs and zero on the aux variables (device Montgomery, the
//                       row product's operand) and w itself as canonical scalars, whose halves
//                       [0, ni) and [ni, n) are the multiexps' w_in and w_aux
//   k_pcheck_h_weights  the signed weights of H's right-hand side: -rho^i | rho^i, i < m - 1
// Nothing here is atomic and no value depends on the order of anything.
#include <algorithm>

#include "ntt_common.cuh"
#include "params_check.h"

using namespace bh;

namespace bh {

// device Montgomery (< 2r) -> the canonical value (x * 2^-261 <= r, as k_scalars_prepare)
__device__ __forceinline__ DFr pc_canonical(const DFr& x) {
  return fe_csub<FrCfg, 1>(fe_from_mont<FrCfg>(x));
}

// y: u | v | w, n each (packed device Montgomery, < 2r).  The same exact test as the generator's
// k_r1cs_ext (ntt_common.cuh: fr_is_zero_below_2r), so both call the same columns present
__global__ void __launch_bounds__(256) k_pcheck_flags(const uint32_t* y, uint32_t n, uint32_t* fu, uint32_t* fv) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  fu[j] = fr_is_zero_below_2r(ld_packed(y, j)) ? 0u : 1u;
  fv[j] = fr_is_zero_below_2r(ld_packed(y, (size_t)n + j)) ? 0u : 1u;
}

// pos: the exclusive scan of flag, so pos[j] < the number of set flags <= n
__global__ void __launch_bounds__(256) k_pcheck_compact(const uint32_t* pw, const uint32_t* flag, const uint32_t* pos,
                                                        uint32_t n, uint32_t* out) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n || !flag[j]) return;
  st_packed(out, pos[j], pc_canonical(ld_packed(pw, j)));
}

__global__ void __launch_bounds__(256) k_pcheck_split(const uint32_t* pw, uint32_t n, uint32_t ni, uint32_t* z_in,
                                                      uint32_t* w) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  const DFr p = ld_packed(pw, j);
  st_packed(z_in, j, j < ni ? p : fe_zero<FrCfg>());
  st_packed(w, j, pc_canonical(p));
}

// hw: 2 m scalars.  r - c for a canonical c is in (0, r]: one conditional subtraction maps r to 0
__global__ void __launch_bounds__(256) k_pcheck_h_weights(const uint32_t* pw, uint32_t m, uint32_t* hw) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m) return;
  DFr c = fe_zero<FrCfg>(), neg = fe_zero<FrCfg>();
  if (i < m - 1) {
    c = pc_canonical(ld_packed(pw, i));
    neg = fe_csub<FrCfg, 1>(fe_sub<FrCfg, 1>(fe_zero<FrCfg>(), c));
  }
  st_packed(hw, i, neg);
  st_packed(hw, (size_t)m + i, c);
}

void params_check_kernels(std::vector<KernInfo>& v) {
  v.push_back({"k_pcheck_flags", (const void*)k_pcheck_flags, 256, 0});
  v.push_back({"k_pcheck_compact", (const void*)k_pcheck_compact, 256, 0});
  v.push_back({"k_pcheck_split", (const void*)k_pcheck_split, 256, 0});
  v.push_back({"k_pcheck_h_weights", (const void*)k_pcheck_h_weights, 256, 0});
}

namespace {

inline unsigned nb(size_t n, unsigned bs) { return (unsigned)((n + bs - 1) / bs); }

// launch_fr_convert's constant that leaves a device value canonical: the raw limbs of the integer 1
// (r1cs.hip: canonical_times)
FrConst canonical_const() {
  FrConst c = {};
  c.v[0] = 1;
  return c;
}

}  // namespace

bh_status params_check_scalars(bh_ctx* ctx, const bh_r1cs* r, const Fr& rho, const Fr& sigma,
                               ParamsCheckScalars* out) {
  const size_t m = r->m, ni = r->ni, n = r->ni + r->na;
  hipStream_t st = ctx->stream;
  Domain* D;
  bh_status s = ctx_domain(ctx, (int)r->L, &D);
  if (s) return s;
  // presence: u and v at x_i = sigma^i
  DevBuf d_x, d_part, d_y, d_flags, d_pos, d_scan, d_pw;
  BH_TRY_HIP(d_x.alloc(m * 32));
  BH_TRY_HIP(d_part.alloc(std::max<size_t>(r->nseg, 1) * 32));
  BH_TRY_HIP(d_y.alloc(r->ncol * 32));
  BH_TRY_HIP(d_flags.alloc(2 * n * 4));
  BH_TRY_HIP(d_pos.alloc(2 * n * 4));
  BH_TRY_HIP(d_scan.alloc(scan_scratch_words(n) * 4 + 64));
  BH_TRY_HIP(d_pw.alloc(std::max(n, m) * 32));
  BH_TRY_HIP(out->w.alloc(n * 32));
  BH_TRY_HIP(out->wa.alloc(n * 32));
  BH_TRY_HIP(out->wb.alloc(n * 32));
  BH_TRY_HIP(out->hw.alloc(2 * m * 32));
  if ((s = r1cs_powers_device(ctx, sigma, m, d_x.as<uint32_t>()))) return s;
  BH_TRY_HIP(r1cs_eval_device(r, d_x.as<uint32_t>(), d_part.as<uint32_t>(), d_y.as<uint32_t>(), st));
  uint32_t* fu = d_flags.as<uint32_t>();
  uint32_t* fv = fu + n;
  uint32_t* pu = d_pos.as<uint32_t>();
  uint32_t* pv = pu + n;
  hipLaunchKernelGGL(k_pcheck_flags, dim3(nb(n, 256)), dim3(256), 0, st, d_y.as<uint32_t>(), (uint32_t)n, fu, fv);
  BH_TRY_HIP(hipGetLastError());
  // the weights rho^j, j < max(n, m), and what is cut from them
  if ((s = r1cs_powers_device(ctx, rho, std::max(n, m), d_pw.as<uint32_t>()))) return s;
  const uint32_t* pw = d_pw.as<uint32_t>();
  exclusive_scan(fu, pu, n, d_scan.as<uint32_t>(), st);
  BH_TRY_HIP(hipGetLastError());
  hipLaunchKernelGGL(k_pcheck_compact, dim3(nb(n, 256)), dim3(256), 0, st, pw, fu, pu, (uint32_t)n,
                     out->wa.as<uint32_t>());
  BH_TRY_HIP(hipGetLastError());
  exclusive_scan(fv, pv, n, d_scan.as<uint32_t>(), st);
  BH_TRY_HIP(hipGetLastError());
  hipLaunchKernelGGL(k_pcheck_compact, dim3(nb(n, 256)), dim3(256), 0, st, pw, fv, pv, (uint32_t)n,
                     out->wb.as<uint32_t>());
  BH_TRY_HIP(hipGetLastError());
  uint32_t hw[4] = {0, 0, 0, 0};  // the counts are all that crosses back
  BH_TRY_HIP(hipMemcpyAsync(&hw[0], pu + n - 1, 4, hipMemcpyDeviceToHost, st));
  BH_TRY_HIP(hipMemcpyAsync(&hw[1], fu + n - 1, 4, hipMemcpyDeviceToHost, st));
  BH_TRY_HIP(hipMemcpyAsync(&hw[2], pv + n - 1, 4, hipMemcpyDeviceToHost, st));
  BH_TRY_HIP(hipMemcpyAsync(&hw[3], fv + n - 1, 4, hipMemcpyDeviceToHost, st));
  DevBuf d_zin;
  BH_TRY_HIP(d_zin.alloc(n * 32));
  hipLaunchKernelGGL(k_pcheck_split, dim3(nb(n, 256)), dim3(256), 0, st, pw, (uint32_t)n, (uint32_t)ni,
                     d_zin.as<uint32_t>(), out->w.as<uint32_t>());
  BH_TRY_HIP(hipGetLastError());
  hipLaunchKernelGGL(k_pcheck_h_weights, dim3(nb(m, 256)), dim3(256), 0, st, pw, (uint32_t)m, out->hw.as<uint32_t>());
  BH_TRY_HIP(hipGetLastError());
  // c_A | c_B | c_C of w and of w_in
  DevBuf d_abc, d_tmp, d_rows;
  BH_TRY_HIP(d_abc.alloc(3 * m * 32));
  BH_TRY_HIP(d_tmp.alloc(m * 32));
  const uint32_t* z[2] = {pw, d_zin.as<uint32_t>()};
  for (int k = 0; k < 2; k++) {
    BH_TRY_HIP(out->coef[k].alloc(3 * m * 32));
    if ((s = r1cs_rows_device(r, z[k], &d_rows, d_abc.as<uint32_t>(), st))) return s;
    for (int v = 0; v < 3; v++)
      if ((s = device_ifft(ctx, D, d_abc.as<uint32_t>() + (size_t)v * m * 8, d_tmp.as<uint32_t>()))) return s;
    launch_fr_convert(d_abc.as<uint32_t>(), out->coef[k].as<uint32_t>(), 3 * m, canonical_const(), 1, st);
    BH_TRY_HIP(hipGetLastError());
  }
  BH_TRY_HIP(hipStreamSynchronize(st));  // the scratch is freed on return
  out->n_a = (size_t)hw[0] + hw[1];
  out->n_b = (size_t)hw[2] + hw[3];
  return BH_OK;
}

}  // namespace bh
