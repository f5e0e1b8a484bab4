// Host interface of the device Proof::read (proofs_dev.hip): k compressed Groth16 proofs decoded,
// sign-selected and subgroup-checked on the device, left as three device vectors.
#pragma once
#include <vector>

#include "api_internal.h"
#include "kinfo.h"

namespace bh {

void proofs_kernels(std::vector<KernInfo>& v);  // scratch budget (scratch.cpp)

// Proof::read (groth16/mod.rs:50-103) of k proofs of 192 bytes each, with verify.cpp's
// from_compressed semantics per point.  a, b, c: empty bh_srs that become the k points A (G1),
// B (G2, as encoded: not negated) and C (G1) in the packed affine device form; a point that failed
// holds the group's generator instead.  status: k words, BH_OK or the error of proof j's first
// failing point in the order A, B, C.  Enqueues on ctx->stream and returns synchronised; the caller
// holds ctx->mu and has set the device.  The return value reports the run (BH_ERR_HIP,
// BH_ERR_OUT_OF_MEMORY), not the proofs.
bh_status proofs_decode_device(bh_ctx* ctx, const uint8_t* proofs, size_t k, std::vector<uint32_t>* status, bh_srs* a,
                               bh_srs* b, bh_srs* c);

}  // namespace bh
