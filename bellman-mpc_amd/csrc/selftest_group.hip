// bh_selftest_group_law: the group law of curve.cuh on caller-chosen raw limbs (selftest_group.cuh).
// This unit holds G1 and G2 in the default field form (schoolbook Fp2 products, carry-seeded
// columns: what the reduction units compile); selftest_group_kara.hip holds G2 as msm_g2_acc.hip
// compiles it.
#include "selftest_group.cuh"

// unit 0: G1; 1: G2, default form; 2: G2, the accumulation unit's form
extern "C" bh_status bh_selftest_group_law(int device, int unit, int op, const uint32_t* in, size_t n, uint32_t* out,
                                           uint32_t* unit_info) {
  switch (unit) {
    case 0: return selftest_group_law_unit<G1Ops>(device, op, in, n, out, unit_info);
    case 1: return selftest_group_law_unit<G2Ops>(device, op, in, n, out, unit_info);
    case 2: return bh::selftest_group_law_kara(device, op, in, n, out, unit_info);
    default: return BH_ERR_INVALID_ARGUMENT;
  }
}
