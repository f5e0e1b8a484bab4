// The host pairing of verify.cpp (BLS12-381 optimal ate; definitions and conventions there) for the
// other host verifiers of the library (mpc.cpp).
#pragma once
#include <vector>

#include "../../include/bellman_hip.h"
#include "host_arith.h"

namespace bh {

struct Fp12 {  // Fp2[w]/(w^6 - xi)
  Fp2 c[6];
};
struct Pair {
  AffinePt<Fp> p;
  AffinePt<Fp2> q;
};

Fp12 f12_one();
bool f12_is_one(const Fp12& a);
Fp12 f12_mul(const Fp12& a, const Fp12& b);
// prod_i f(p_i, q_i) before the final exponentiation; a term with an identity is skipped (its
// pairing value is one).  The product of two calls' results is the Miller value of their union.
Fp12 multi_miller_loop(const std::vector<Pair>& pairs);
Fp12 final_exponentiation(const Fp12& f);
// prod_i e(p_i, q_i) == 1
bool pairing_product_is_one(const std::vector<Pair>& pairs);

// G1Affine / G2Affine::from_compressed_unchecked of one point (48 / 96 bytes), the identity refused
// as Proof::read refuses it; check_subgroup adds the torsion test of from_compressed.
// BH_ERR_INVALID_ENCODING: the compression flag clear, the infinity flag set, a coordinate >= p or
// x^3 + b not a square, in that order; BH_ERR_NOT_IN_SUBGROUP.
template <class T>
bh_status point_from_compressed(const uint8_t* in, AffinePt<T>* out, bool check_subgroup);

}  // namespace bh
