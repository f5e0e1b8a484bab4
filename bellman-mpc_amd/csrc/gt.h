// Host interface of the target group's unit (gt.hip): a vector of Gt values resident on a
// context's device, behind the bh_gt_* entry points of include/bellman_hip.h.
#pragma once
#include <vector>

#include "api_internal.h"
#include "kinfo.h"

namespace bh {

void gt_kernels(std::vector<KernInfo>& v);  // scratch budget (scratch.cpp)

}  // namespace bh

// n values in the crate's convention (conj(e0)^3 of the library's own), on the flat basis
// sum_k c_k w^k, fully reduced device Montgomery words in the word-major lane layout of the pairing
// workspace: word w (of 144) of element l at w * stride + l, stride = n rounded up to 64 lanes.
struct bh_gt {
  bh_ctx* ctx = nullptr;
  size_t n = 0, stride = 0;
  bh::DevBuf v;
};
