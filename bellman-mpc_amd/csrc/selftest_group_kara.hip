// Unit 2 of bh_selftest_group_law: G2's group law with the field form of the bucket accumulation
// (msm_g2_acc.hip: split column chains, column-wise Karatsuba Fp2 products).
#define BH_COLUMN_CHAIN 0
#define BH_FP2_KARATSUBA 1
#include "selftest_group.cuh"

namespace bh {
bh_status selftest_group_law_kara(int device, int op, const uint32_t* in, size_t n, uint32_t* out,
                                  uint32_t* unit_info) {
  return selftest_group_law_unit<G2Ops>(device, op, in, n, out, unit_info);
}
}  // namespace bh
