// Host interface of the scalar side of bh_params_check (params_check.hip):
// every scalar vector the check's multiexps read, written on the device and left there.  The
// function enqueues on ctx->stream and returns synchronised; the caller holds ctx->mu and has set
// the device.
#pragma once
#include <vector>

#include "api_internal.h"
#include "kinfo.h"
#include "r1cs.h"

namespace bh {

void params_check_kernels(std::vector<KernInfo>& v);  // scratch budget (scratch.cpp)

// With n = ni + na variables in the order [inputs, aux], w_j = rho^j and x_i = sigma^i, i < m:
struct ParamsCheckScalars {
  size_t n_a = 0, n_b = 0;  // present columns of A and of B: u_j != 0, v_j != 0 at x
  DevBuf w;                 // n canonical scalars w_j: w_in is [0, ni), w_aux is [ni, n)
  DevBuf wa, wb;            // w compacted to the present columns of A / of B, order kept
  // c_A | c_B | c_C (3 m canonical scalars): the inverse transforms of the rows A z | B z | C z,
  // coef[0] for z = w, coef[1] for z = w_in (w on the inputs, zero on the aux variables)
  DevBuf coef[2];
  // 2 m canonical scalars, the signed weights of H: -rho^i at i and rho^i at m + i for i < m - 1,
  // zero at m - 1 and 2 m - 1; the m - 1 scalars from m on are the weights of h itself
  DevBuf hw;
};

// m = r->m >= 2; rho, sigma nonzero
bh_status params_check_scalars(bh_ctx* ctx, const bh_r1cs* r, const Fr& rho, const Fr& sigma, ParamsCheckScalars* out);

}  // namespace bh
