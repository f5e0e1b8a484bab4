// The NTT's butterflies and store-path transformations as device functions over values in
// registers (k_ntt_pass in ntt.hip does the LDS staging and the index math around them;
// bh_selftest_ntt_butterfly in selftest_ntt.hip runs each on caller-chosen raw limbs,
// tests/test_gpu_ntt_butterfly.py).
//
// Contracts, with r the scalar modulus (r8 = its top limb, 2^29 / r8 = 70.6):
//   - "normalised": limbs 0..7 <= 2^29 - 1; the top limb holds whatever the value needs.
//   - A DIF butterfly takes normalised values < 2r and returns normalised values < 2r.
//   - A DIT pass is lazy: its first stage takes normalised values < 2r (freshly loaded), a
//     radix-2 stage returns values < 4r, and a radix-4 step whose inputs are < B returns values
//     < B + 4r, all normalised; after D <= 10 stages the values are < 2r(D + 1) <= 22r < 2^261 and
//     the storing pass reduces them (ntt_store_plain, ntt_store_scalars, ntt_store_product).
// An operand that a flag can switch off (a unit stage's twiddle, the optional `sub`) is passed as
// a callable returning the DFr and is called only where the value is read: k_ntt_pass passes the
// table load itself, so no load moves out of the branch it had.
#pragma once
#include "field.cuh"

namespace bh {

// ---- limb-wise (carry-free) butterfly arithmetic.  A value handed to fe_mul needs neither
// normalised limbs nor a reduced value: the largest limbs an operand below takes are
// 5 * 2^29 - 3 = 2^31.32 (lw_sub<8, 2> of two lw_add sums); against a twiddle's normalised limbs a
// column then holds 9 products < 2^60.4 plus 8 m*p products < 2^58, and the worst accumulator is
// < 2^63.4 with the carry (tests/test_field_column_bounds_cpu.py walks the columns with each
// expression's own maxima), and an operand < 70r keeps the product < 2r (70 r^2 < 2^261 r; the
// largest operand here is < 22r).  So the sums and differences that only feed a product skip the
// carry chain (1-2 VALU per limb instead of 3-4).
// K*r with every limb below the top >= J*(2^29-1), i.e. >= a sum of J normalised limbs: J*2^29
// added to limb i is J taken from limb i+1 (the value is unchanged)
template <uint32_t K, uint32_t J>
struct FrBias {
  struct L { uint32_t v[9]; };
  static constexpr L make() {
    L l{};
    for (int i = 0; i < 9; i++) {
      int64_t c = KP<FrCfg, K>::value.v[i];
      if (i < 8) c += (int64_t)J << 29;
      if (i > 0) c -= J;
      l.v[i] = (uint32_t)c;
    }
    return l;
  }
  static constexpr L value = make();
};
__device__ __forceinline__ DFr lw_add(const DFr& a, const DFr& b) {
  DFr r;
#pragma unroll
  for (int l = 0; l < 9; l++) r.v[l] = a.v[l] + b.v[l];
  return r;
}
// a + K*r - b limb-wise; b's limbs below the top must be sums of at most J normalised limbs, and
// its top limb at most K*r's minus J (b < (K/2) r for the callers' bounds; ntt_dit4's a1, with
// K = 2 against a product < 2r, relies on products of twiddles staying < 1.26 r or on the wrap
// being undone by the carried sum that follows)
template <uint32_t K, uint32_t J>
__device__ __forceinline__ DFr lw_sub(const DFr& a, const DFr& b) {
  DFr r;
#pragma unroll
  for (int l = 0; l < 9; l++) r.v[l] = a.v[l] + (FrBias<K, J>::value.v[l] - b.v[l]);
  return r;
}
// carry propagation: the same value in normalised limbs.  Every input limb plus the carry into it
// must stay below 2^32; the two callers feed limbs <= 5 * 2^29 - 3 with carries <= 5 (ntt_dif4:
// lw_sub<8, 2> of two lw_add sums; ntt_dit4: lw_sub<2, 1> of a1, itself a lw_sub<2, 1>).  A top
// limb that wrapped comes out right when the value is in [0, 2^261): it is computed mod 2^32.
__device__ __forceinline__ DFr lw_norm(const DFr& a) {
  DFr r;
  uint32_t c = 0;
#pragma unroll
  for (int l = 0; l < 9; l++) {
    const uint32_t s = a.v[l] + c;
    r.v[l] = l < 8 ? (s & FrCfg::MASK) : s;
    c = s >> FrCfg::BITS;
  }
  return r;
}

// x < 2^261 with normalised limbs below the top one -> x - q*r < 2r, one pass instead of a chain
// of conditional subtractions (fe_csub 16, 8, 4, 2: ~40 VALU each).  r = r8 * 2^232 + r_low with
// 0 < r_low < 2^232 and x < (x8 + 1) * 2^232, so q = floor(x8 / (r8 + 1)) gives q*r <= x and
// x - q*r < (r8 + 1 + q) * 2^232 < 2r (q < 2^29 / r8 = 70).  The quotient comes from one FP64
// fma, exact: (x8 + 1/2) / (r8 + 1) is at least 1/(2(r8 + 1)) ~ 6.6e-8 away from an integer,
// far beyond the product's rounding (< 71 * 2^-52).
__device__ __forceinline__ DFr fr_qreduce(const DFr& x) {
  constexpr double inv = 1.0 / (double)(FrCfg::P[8] + 1u);
  const uint32_t q = (uint32_t)__builtin_fma((double)x.v[8], inv, 0.5 * inv);
  DFr r;
  int64_t c = 0;
#pragma unroll
  for (int l = 0; l < 9; l++) {
    const int64_t t = (int64_t)x.v[l] + c - (int64_t)((uint64_t)q * FrCfg::P[l]);
    r.v[l] = l < 8 ? ((uint32_t)t & FrCfg::MASK) : (uint32_t)t;
    c = t >> FrCfg::BITS;  // arithmetic
  }
  return r;
}

// ---- radix-2.  x, y < 2r (normalised); unit: the twiddle is omega_2^0 = 1 and w is not read.
// DIF (Gentleman-Sande): nx = x + y, ny = (x - y) w, both < 2r
template <class W>
__device__ __forceinline__ void ntt_dif2(const DFr& x, const DFr& y, W&& w, bool unit, DFr& nx, DFr& ny) {
  if (unit) {
    nx = fe_csub<FrCfg, 2>(fe_add<FrCfg>(x, y));
    ny = fe_csub<FrCfg, 2>(fe_sub<FrCfg, 2>(x, y));
  } else {
    nx = fe_csub<FrCfg, 2>(fe_add<FrCfg>(x, y));      // < 4r -> < 2r
    ny = fe_mul<FrCfg>(lw_sub<4, 1>(x, y), w());      // operand in (2r, 6r), limbs < 3 * 2^29
  }
}
// DIT (Cooley-Tukey): nx = x + y w, ny = x - y w.  Always the first stage of its pass: < 2r with
// the unit twiddle, else lazy (no conditional subtraction inside a DIT pass), < 4r
template <class W>
__device__ __forceinline__ void ntt_dit2(const DFr& x, const DFr& y, W&& w, bool unit, DFr& nx, DFr& ny) {
  if (unit) {
    nx = fe_csub<FrCfg, 2>(fe_add<FrCfg>(x, y));
    ny = fe_csub<FrCfg, 2>(fe_sub<FrCfg, 2>(x, y));
  } else {
    const DFr t = fe_mul<FrCfg>(y, w());              // < 2r
    nx = fe_add<FrCfg>(x, t);                         // < 4r
    ny = fe_sub<FrCfg, 2>(x, t);                      // x + 2r - t < 4r
  }
}

// ---- radix-4: two stages in registers.
// DIF: first (x0, x2) by wa0 and (x1, x3) by wa1, then (., .) pairs by wb (unit_b: wb = 1, not
// read).  y0 = x0 + x1 + x2 + x3, y1 = (x0 + x2 - x1 - x3) wb, y2 = (x0 - x2) wa0 + (x1 - x3) wa1,
// y3 = ((x0 - x2) wa0 - (x1 - x3) wa1) wb.  Inputs < 2r (normalised); the sums feeding y0/y1 and
// the differences feeding the products stay limb-wise (see lw_sub), every output is < 2r, normalised
template <class W>
__device__ __forceinline__ void ntt_dif4(const DFr (&x)[4], const DFr& wa0, const DFr& wa1, W&& wb, bool unit_b,
                                         DFr (&y)[4]) {
  const DFr s02 = lw_add(x[0], x[2]), s13 = lw_add(x[1], x[3]);  // < 4r, limbs <= 2^30 - 2
  const DFr u2 = fe_mul<FrCfg>(lw_sub<4, 1>(x[0], x[2]), wa0);   // operand in (2r, 6r); u2 < 2r
  const DFr u3 = fe_mul<FrCfg>(lw_sub<4, 1>(x[1], x[3]), wa1);
  y[0] = fr_qreduce(fe_add<FrCfg>(s02, s13));                    // < 8r (carried) -> < 2r
  y[2] = fe_csub<FrCfg, 2>(fe_add<FrCfg>(u2, u3));               // < 4r -> < 2r
  if (unit_b) {  // omega_2^0 = 1
    y[1] = fr_qreduce(lw_norm(lw_sub<8, 2>(s02, s13)));          // in (4r, 12r) -> < 2r
    y[3] = fr_qreduce(lw_norm(lw_sub<4, 1>(u2, u3)));            // in (2r, 6r) -> < 2r
  } else {
    const DFr w = wb();
    y[1] = fe_mul<FrCfg>(lw_sub<8, 2>(s02, s13), w);  // operand in (4r, 12r), limbs <= 5 * 2^29 - 3
    y[3] = fe_mul<FrCfg>(lw_sub<4, 1>(u2, u3), w);    // operand in (2r, 6r), limbs < 3 * 2^29
  }
}
// DIT: first (x0, x1) and (x2, x3) by wa (unit_a: wa = 1, not read), then (., .) pairs by wb0, wb1.
// With t0 = x1 wa, t1 = x3 wa: y0 = (x0 + t0) + (x2 + t1) wb0, y2 = (x0 + t0) - (x2 + t1) wb0,
// y1 = (x0 - t0) + (x2 - t1) wb1, y3 = (x0 - t0) - (x2 - t1) wb1.
// Lazy reduction: a DIT stage adds a product (< 2r) to, or subtracts it (+2r) from, a value < B,
// so inputs < B (normalised) give outputs < B + 4r (normalised): from < 2r at the pass's first
// stage values stay < 2r(D+1) <= 22r < 2^261 in the 9 limbs, and a Montgomery product of such a
// value with a twiddle (< r) still ends < 2r (22 r^2 < 2^261 r); the storing pass reduces.
// unit_a only occurs at global stage 0, on freshly loaded values (< 2r); the outputs are then < 4r.
// (wb0, wb1 are always read; they are callables so that k_ntt_pass loads them after the first stage.)
template <class W, class W0, class W1>
__device__ __forceinline__ void ntt_dit4(const DFr (&x)[4], W&& wa, W0&& wb0, W1&& wb1, bool unit_a,
                                         DFr (&y)[4]) {
  // a0, a1 stay limb-wise.  a1's top limb is x0's + (2r's - 1) - t0's: it would wrap for x0 < 2^232
  // under a t0 whose top limb equals 2r's, and that is tolerated (a1 only reaches carried sums
  // whose values lie in [0, 2^261), and those come out right mod 2^32 in the top limb; the same
  // holds for a0 + 2r - s0 before lw_norm).  With a twiddle < r no t0 gets there: a product of
  // x < 18r is < r + x r / 2^261 < 1.26 r, so in a pass the top limbs never wrap.
  // p2, p3 are operands of products (limb-wise; p2 < B + 2r, p3 in (2r, B + 4r), so < 22r at the
  // last step of a 10-stage pass, limbs < 3 * 2^29)
  DFr a0, a1, p2, p3;
  if (unit_a) {  // omega_2^0 = 1
    a0 = fe_csub<FrCfg, 2>(fe_add<FrCfg>(x[0], x[1]));
    a1 = fe_csub<FrCfg, 2>(fe_sub<FrCfg, 2>(x[0], x[1]));
    p2 = fe_csub<FrCfg, 2>(fe_add<FrCfg>(x[2], x[3]));
    p3 = fe_csub<FrCfg, 2>(fe_sub<FrCfg, 2>(x[2], x[3]));
  } else {
    const DFr w = wa();
    const DFr t0 = fe_mul<FrCfg>(x[1], w), t1 = fe_mul<FrCfg>(x[3], w);  // < 2r
    a0 = lw_add(x[0], t0);        // < B + 2r, limbs <= 2^30 - 2
    a1 = lw_sub<2, 1>(x[0], t0);  // x0 + 2r - t0 in (0, B + 2r), limbs <= 3 * 2^29 - 2
    p2 = lw_add(x[2], t1);
    p3 = lw_sub<4, 1>(x[2], t1);  // top limb >= 4r's - 1 - 2r's: no wrap
  }
  const DFr w0 = wb0(), w1 = wb1();
  const DFr s0 = fe_mul<FrCfg>(p2, w0), s1 = fe_mul<FrCfg>(p3, w1);  // < 2r
  y[0] = fe_add<FrCfg>(a0, s0);                  // < B + 4r
  y[2] = lw_norm(lw_sub<2, 1>(a0, s0));          // a0 + 2r - s0 in (0, B + 4r), limbs <= 2^31 - 3
  y[1] = fe_add<FrCfg>(a1, s1);                  // < B + 4r (fe_add masks the top limb: mod 2^29)
  y[3] = lw_norm(lw_sub<2, 1>(a1, s1));          // x0 + 4r - t0 - s1 in (0, B + 4r), limbs <= 5 * 2^29 - 3
}

// ---- what the storing pass does to a loaded value x (after the optional post-scale); x is
// updated in place.
// The plain store.  lazy: x is a bare DIT value (< 22r, normalised) and is reduced below 2r for
// the packed form; otherwise x < 2r already (post-scaled, or a DIF value).  has_sub: sub (< 2r) is
// subtracted: x + 2r - sub < 4r, one conditional subtraction back below 2r (sub is not read otherwise)
template <class S>
__device__ __forceinline__ void ntt_store_plain(DFr& x, bool lazy, bool has_sub, S&& sub) {
  if (lazy) x = fr_qreduce(x);
  if (has_sub) x = fe_csub<FrCfg, 2>(fe_sub<FrCfg, 2>(x, sub()));
}
// The SCALARS epilogue: the canonical scalar, packed.  x + 2r - sub with sub < 2r, and x < 2r
// (post-scaled or a DIF value; < 22r from a bare DIT).  Then x < 24r < 2^261 (< 4r in the H
// block), so x * 2^-261 <= r: one subtraction
template <class S>
__device__ __forceinline__ void ntt_store_scalars(DFr& x, bool has_sub, S&& sub, uint32_t (&w8)[8]) {
  if (has_sub) x = fe_sub<FrCfg, 2>(x, sub());
  fe_pack<FrCfg>(fe_csub<FrCfg, 1>(fe_from_mont<FrCfg>(x)), w8);
}
// The PRODUCT epilogue: pa * x * k for x = b (< 22r, normalised limbs), pa < 2r, k < r.
// pa * x < 44 r^2 < 2^261 r, so both Montgomery products end < 2r
__device__ __forceinline__ DFr ntt_store_product(const DFr& pa, const DFr& x, const DFr& k) {
  return fe_mul<FrCfg>(fe_mul<FrCfg>(pa, x), k);
}

}  // namespace bh
