// Host interface of the device multi-Miller loop (pairing_dev.hip): the product of the Miller
// values of n (G1, G2) pairs held in two device vectors, in the conventions of verify.cpp.
#pragma once
#include <vector>

#include "api_internal.h"
#include "kinfo.h"
#include "pairing.h"

namespace bh {

void pairing_kernels(std::vector<KernInfo>& v);  // scratch budget (scratch.cpp)

constexpr int MILLER_MAX_K = 16;  // pairs per lane

// *out = prod_{i < n} f(g1[off1 + i], g2[off2 + i]) before the final exponentiation, equal
// coefficient for coefficient to multi_miller_loop of the same pairs (a pair with an all-zero
// record, the identity, on either side contributes one).  K: pairs per lane, 1..MILLER_MAX_K, or 0
// for the library's choice.  Enqueues on ctx->stream and returns synchronised; the caller holds
// ctx->mu, has set the device and has checked the ranges.
// BH_ERR_PAIRING_DEGENERATE: a step met a zero denominator (a twist point outside the order-r
// subgroup); *out is then not written.
bh_status miller_product_device(bh_ctx* ctx, const bh_srs* g1, size_t off1, const bh_srs* g2, size_t off2, size_t n,
                                int K, Fp12* out);

// verdict[l] = 1 iff scale * prod_{k < K} f(g1[l K + k], g2[l K + k]) has final exponentiation one,
// else 0, for l < lanes: K pairs per lane of packed affine records in two device arrays (an
// all-zero record, the identity, makes its pair count as one), the Miller loops, the product by
// the host's value `scale`, the final exponentiation and the comparison all on the device, at most
// MILLER_CHUNK lanes per pass.  Returns synchronised; the caller holds ctx->mu and has set the
// device.  BH_ERR_PAIRING_DEGENERATE as above; verdict is then unspecified.
bh_status pairing_each_is_one(bh_ctx* ctx, const uint32_t* g1, const uint32_t* g2, size_t lanes, int K,
                              const Fp12& scale, uint32_t* verdict);

}  // namespace bh
