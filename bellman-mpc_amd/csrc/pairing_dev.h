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

}  // namespace bh
