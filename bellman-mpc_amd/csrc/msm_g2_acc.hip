// G2Ops instantiation of the device MSM, part 1: workspace, digit sort and the bucket
// accumulation kernels (see msm_impl.cuh).  The accumulation's Fp2 products use the column-wise
// Karatsuba form (field.cuh); every kernel of this unit is emitted here only.
// This unit keeps the split (two chains and a merge per column) products: its kernels sit at the
// register limit, and carry-seeded columns cost k_accumulate_pf<G2> one more AGPR (12 -> 13) and
// k_accumulate_g2d 4 more bytes of scratch for 1.2 % fewer static VALU.
#define BH_COLUMN_CHAIN 0
#define BH_FP2_KARATSUBA 1
#include "msm_impl.cuh"

namespace bh {
template struct MsmWorkspace<G2Ops>;
template void fit_segments<G2Ops>(MsmShape&, size_t);
template void fit_segments_E<G2Ops>(MsmShape&, size_t);
template hipError_t msm_sort<G2Ops>(MsmWorkspace<G2Ops>&, hipStream_t, const uint32_t*, size_t, const int32_t*,
                                     uint32_t, const MsmShape&);
template hipError_t msm_accumulate<G2Ops>(MsmWorkspace<G2Ops>&, hipStream_t, const uint32_t*, size_t, const MsmShape&,
                                           MsmTiming*);
template hipError_t msm_selftest_accumulate<G2Ops>(int, const uint32_t*, size_t, uint32_t, const uint32_t*, size_t,
                                                    const uint32_t*, size_t, uint32_t, uint32_t, uint32_t, uint32_t*,
                                                    uint32_t*, uint32_t*);
template void msm_acc_kernels<G2Ops>(std::vector<KernInfo>&);
}  // namespace bh
