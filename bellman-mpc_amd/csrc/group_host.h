// What a G1 / G2 point looks like, in the one place that defines it:
//  * on the host: AffinePt<Field> / Jac<Field> in bls12_381's Montgomery form (host_arith.h);
//  * on the device: WORDS packed u32 words per affine point, its Fp components in memory order
//    (x, y; x.c0, x.c1, y.c0, y.c1), 12 little-endian words each, the canonical value of
//    c * 2^406 mod p (the device's Montgomery radix; the all-zero record stands for the identity,
//    which bh_srs::identity_idx lists);
//  * on the wire: WIRE bytes uncompressed (host_arith.h: to_uncompressed / from_uncompressed and
//    wire_component give the slot order and the flag bits).
// Host code that handles points of either group is a template over G1Host / G2Host; with_group()
// is the only place that turns a BH_G1 / BH_G2 value into one of them.
#pragma once
#include "../../include/bellman_hip.h"
#include "curve.cuh"
#include "host_arith.h"

namespace bh {

// the field ops a device curve is built on
template <class C>
struct FieldOf;
template <class Fd>
struct FieldOf<CurveOps<Fd>> { using F = Fd; };

// Device packed words of one Fp component -> host Montgomery.  The words hold a = c * 2^406, the
// host wants c * 2^384 = a * 2^-22 = mont_mul(a, 2^362 mod p).
static_assert(G1F::Cf::N * G1F::Cf::BITS == 406 && FpCfg::N * FpCfg::BITS == 406, "the device radix of both groups");
static inline Fp fp_from_dev_words(const uint32_t* w) {
  Fp a;
  for (int i = 0; i < 6; i++) a.v[i] = (uint64_t)w[2 * i] | ((uint64_t)w[2 * i + 1] << 32);
  static Fp K = [] {
    uint64_t two[6] = {2, 0, 0, 0, 0, 0};
    Fp t = from_int<6>(two);
    uint64_t e[1] = {768 - 406};
    Fp k = pow_vartime(t, e, 1);  // Montgomery(2^362)
    uint64_t raw[6];
    to_int(k, raw);               // canonical 2^362 mod p
    Fp out; memcpy(out.v, raw, sizeof raw);
    return out;
  }();
  return mul(a, K);
}
// one reduced device coordinate (CurveOps::reduce: canonical limbs) -> packed words -> host
static inline Fp coord_from_dev(const DFp& x) {
  uint32_t words[12] = {0};
  for (int i = 0; i < FpCfg::N; i++) {
    const int bit = FpCfg::BITS * i;
    const int wi = bit >> 5, sh = bit & 31;
    const uint64_t v = (uint64_t)x.v[i] << sh;
    words[wi] |= (uint32_t)v;
    if (wi + 1 < 12) words[wi + 1] |= (uint32_t)(v >> 32);
  }
  return fp_from_dev_words(words);
}
static inline Fp2 coord_from_dev(const DFp2& x) { return Fp2{coord_from_dev(x.c0), coord_from_dev(x.c1)}; }

template <class T, class C, int Id, int Words>
struct GroupHost {
  using Field = T;
  using Affine = AffinePt<T>;
  using Jacobian = Jac<T>;
  using Ops = C;
  using DevField = typename FieldOf<C>::F;
  static constexpr int ID = Id;
  static constexpr int WORDS = Words;        // u32 words of a packed device point
  static constexpr size_t WIRE = 4 * Words;  // bytes of an uncompressed encoding
  static_assert(Words == 12 * COMPONENTS<T> && Words == 2 * DevField::PACKED_WORDS, "one layout");

  static Field coord_from_dev(const typename C::T& x) { return bh::coord_from_dev(x); }
  static Affine from_dev_words(const uint32_t* w) {
    Affine a;
    for (int k = 0; k < COMPONENTS<T>; k++) components(a)[k] = fp_from_dev_words(w + 12 * k);
    a.infinity = false;
    return a;
  }
  // the canonical packed words an upload hands to the device conversion (identity: all zero)
  static void canonical_words(const Affine& a, uint32_t* w) {
    if (a.infinity) { memset(w, 0, WORDS * 4); return; }
    for (int k = 0; k < COMPONENTS<T>; k++) {
      uint64_t raw[6];
      to_int(components(a)[k], raw);
      memcpy(w + 12 * k, raw, 48);
    }
  }
  static Jacobian from_xyzz(const XYZZ<DevField>& p) {
    return xyzz_to_jac(coord_from_dev(p.X), coord_from_dev(p.Y), coord_from_dev(p.ZZ), coord_from_dev(p.ZZZ));
  }
};
using G1Host = GroupHost<Fp, G1Ops, BH_G1, 24>;
using G2Host = GroupHost<Fp2, G2Ops, BH_G2, 48>;

// the host description of a device curve / of a host coordinate field
template <class C>
using HostOf = typename std::conditional<std::is_same<C, G1Ops>::value, G1Host, G2Host>::type;
template <class T>
using HostOfField = typename std::conditional<std::is_same<T, Fp>::value, G1Host, G2Host>::type;

// f(G1Host{}) or f(G2Host{}); group is BH_G1 or BH_G2 (the entry points validate it)
template <class Fn>
static inline auto with_group(int group, Fn&& f) {
  return group == BH_G1 ? f(G1Host{}) : f(G2Host{});
}

}  // namespace bh
