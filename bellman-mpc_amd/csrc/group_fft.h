// Host interface of the group-valued FFT and of the sparse matrix product over point vectors
// (group_fft.hip): what turns a finished round one of the ceremony into the vectors round two
// starts from (mpc.cpp).  Every function enqueues on ctx->stream and returns synchronised; the
// caller holds ctx->mu and has set the device.
#pragma once
#include <vector>

#include "api_internal.h"
#include "kinfo.h"
#include "r1cs.h"

namespace bh {

void group_fft_kernels(std::vector<KernInfo>& v);  // scratch budget (scratch.cpp)

// EvaluationDomain<Point<G>>::fft / ifft (domain.rs:81-99) of the first n = 2^L points of `in`
// (2 <= n <= 2^28, n <= in->n), natural order in and out.  inverse: omega^-1, and the 1/n when
// `scale` (a consumer that multiplies the result by scalars anyway folds it into those instead).
// BH_ERR_UNEXPECTED_IDENTITY: an identity in `in` or among the butterfly outputs of any stage.
bh_status group_fft(bh_ctx* ctx, const bh_srs* in, size_t n, int inverse, bool scale, bh_srs* out);

// The circuit-specific vectors of CommonParamterMatrix from the UNSCALED inverse transforms
// lag[0..6) (m points each, the order of BH_MPC_TAU_G1 .. BH_MPC_BETA_TAU_G2) of a storage's six
// vectors: the 1/m goes into the coefficients.
//   out[0..4)  kin_g1, kin_g2, kout_g1, kout_g2: beta A_j + alpha B_j + C_j of the inputs / the aux
//   out[4..7)  A_j(tau) G1, B_j(tau) G1, B_j(tau) G2 over [inputs, aux], identities filtered out
// BH_ERR_UNEXPECTED_IDENTITY: an identity among kin; BH_ERR_UNCONSTRAINED_VARIABLE: among kout.
bh_status matrix_product(bh_ctx* ctx, const bh_r1cs* r, const bh_srs* const lag[6], bh_srs* const out[7]);

}  // namespace bh
