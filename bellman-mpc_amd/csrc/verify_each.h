// Host interface of the per-proof verifier's device stages between Proof::read (proofs_dev.hip) and
// the Miller loops (pairing_dev.hip): the accumulated inputs of every proof and the pairs of every
// lane, for bh_verify_each_device (verify.cpp).
#pragma once
#include <vector>

#include "api_internal.h"
#include "kinfo.h"

namespace bh {

void verify_each_kernels(std::vector<KernInfo>& v);  // scratch budget (scratch.cpp)

// The 3 k Miller pairs of k proofs, lane-interleaved: pair 3 j is (A_j, B_j), pair 3 j + 1 is
// (-acc_j, gamma) with acc_j = ic[0] + sum_i x_ji ic[i + 1] (verifier.rs:33-40), pair 3 j + 2 is
// (-C_j, delta); g1 and g2 become 3 k packed affine records each.  a, b, c: the decoded proofs
// (proofs_decode_device).  ic: n_ic >= 1 points of the order-r subgroup, none the identity.
// inputs: k (n_ic - 1) canonical scalars below r, 4 LE u64 each.  An acc_j that is the identity is
// stored as the all-zero record, which the Miller loop counts as a pair of value one; so is an
// identity gamma or delta.  Enqueues on ctx->stream and returns synchronised; the caller holds
// ctx->mu and has set the device.
bh_status verify_each_pairs(bh_ctx* ctx, const bh_srs& a, const bh_srs& b, const bh_srs& c, const AffinePt<Fp>* ic,
                            size_t n_ic, const AffinePt<Fp2>& gamma, const AffinePt<Fp2>& delta, const uint64_t* inputs,
                            size_t k, DevBuf* g1, DevBuf* g2);

}  // namespace bh
