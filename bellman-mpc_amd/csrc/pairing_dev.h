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

// ---- the pieces the target group's unit (gt.hip) builds on; the caller holds ctx->mu and has set
// the device.
// pairs per call of the loop (the workspace: 752 B per pair at K = 16, plus 1.7 KB per lane)
constexpr size_t MILLER_CHUNK = (size_t)1 << 20;

// The loop's device state of one call.  f: fslots >= 2 Fp12 buffers of 144 * stride words each, the
// first two the loop's double buffer; miller_lanes leaves every lane's value in the first.
struct MillerWork {
  DevBuf f, T, S, mask, flag;
  size_t lanes = 0, stride = 0;
};
// lane l's value prod_{k < K} f(g1[l K + k], g2[l K + k]) for the lanes of n pairs, left on the
// device in w->f; returns synchronised.  BH_ERR_PAIRING_DEGENERATE: a step met a zero denominator.
bh_status miller_lanes(bh_ctx* ctx, const uint32_t* g1, const uint32_t* g2, size_t n, int K, int fslots,
                       MillerWork* w);

// The final exponentiation's chain in place on slot 0 of ws (FE_SLOTS * 144 * stride words),
// enqueued on ctx->stream; the tables must outlive the enqueued work (the caller synchronises
// before dropping them).
struct FexpTables {
  DevBuf prog, consts;
  std::vector<std::pair<int, int>> launches;
};
bh_status fexp_tables(bh_ctx* ctx, FexpTables* t);
bh_status fexp_enqueue(bh_ctx* ctx, const FexpTables& t, uint32_t* ws, size_t n, size_t stride);

// The product of the m values at lanes 0 .. m-1 of f, which the levels overwrite; ping and pong: one
// Fp12 buffer each of the same stride.  Returns synchronised.
bh_status f12_lanes_product(bh_ctx* ctx, uint32_t* f, uint32_t* ping, uint32_t* pong, size_t stride, size_t m,
                            Fp12* out);

// host Montgomery (R = 2^384) <-> the device's packed words (12 per Fp; a value's 144 in the
// order c[0].c0, c[0].c1, ..., c[5].c1)
void fp_to_dev_words(const Fp& x, uint32_t* w);
Fp12 f12_from_dev_words(const uint32_t* w);

}  // namespace bh
