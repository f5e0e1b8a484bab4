// G1Ops instantiation of the device MSM, part 2: continuation fix-up, bucket reduction
// and window sums (see msm_impl.cuh).
#include "msm_impl.cuh"

namespace bh {
// instantiated in msm_g1_acc.hip (the accumulation kernels compile there, in parallel)
extern template struct MsmWorkspace<G1Ops>;
extern template void fit_segments<G1Ops>(MsmShape&, size_t);
extern template void fit_segments_E<G1Ops>(MsmShape&, size_t);
extern template hipError_t msm_sort<G1Ops>(MsmWorkspace<G1Ops>&, hipStream_t, const uint32_t*, size_t, const int32_t*,
                                            uint32_t, const MsmShape&);
extern template hipError_t msm_accumulate<G1Ops>(MsmWorkspace<G1Ops>&, hipStream_t, const uint32_t*, size_t,
                                                  const MsmShape&, MsmTiming*);

template hipError_t msm_window_sums<G1Ops>(MsmWorkspace<G1Ops>&, hipStream_t, const uint32_t*, const uint32_t*, size_t,
                                         const int32_t*, uint32_t, const MsmShape&, MsmTiming*);
template hipError_t msm_front<G1Ops>(MsmWorkspace<G1Ops>&, hipStream_t, const uint32_t*, const uint32_t*, size_t,
                                   const int32_t*, uint32_t, const MsmShape&, MsmTiming*);
template hipError_t msm_back<G1Ops>(MsmWorkspace<G1Ops>&, hipStream_t, size_t, const MsmShape&, typename G1Ops::P*, int, hipEvent_t, const uint32_t*);
template hipError_t msm_selftest_reduce<G1Ops>(int, const uint32_t*, size_t, uint32_t, const uint32_t*, size_t,
                                                const uint32_t*, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t,
                                                uint32_t*, uint32_t*);
template void msm_back_kernels<G1Ops>(std::vector<KernInfo>&);
}  // namespace bh
