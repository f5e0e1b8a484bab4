// The final exponentiation f^((p^12 - 1) / r) as a short chain, written once for the host and the
// device: a program of steps over a handful of Fp12 slots (fe_program), the ten Frobenius
// constants (fe_consts), and the host interpreter over pairing.h's Fp12 (fe_chain_host).  The
// device interpreter is k_fexp_steps of pairing_dev.hip: the same program, one lane per value.
//
// The exponent is exactly (p^12 - 1) / r, the one verify.cpp's square-and-multiply ladder uses (the
// ladder stays the yardstick: tests/test_final_exp_chain_cpu.py compares the two):
//   (p^12 - 1) / r = (p^6 - 1) (p^2 + 1) h,   h = (p^4 - p^2 + 1) / r = c (x + p) (x^2 + p^2 - 1) + 1,
//   x = -0xd201000000010000,   c = (x - 1)^2 / 3 = 0x396c8c005555e1568c00aaab0000aaab.
// (The common hard part built on 3 h gives the cube of this value.)
//   easy part   t = conj(f) f^-1,  m = frob^2(t) t          -- from here on m^-1 = conj(m)
//   hard part   a = m^c,  b = a^x frob(a),  d = (b^x)^x frob^2(b) conj(b),  result = d m
// with a^x = conj(a^|x|) and (b^x)^x = (b^|x|)^|x|: 314 squarings and 72 other products, against
// the ladder's 4313 and 2100.
//
// The one inversion goes down the tower of subfields to a single Fermat inversion in Fp, through
// norms, so that it needs nothing but Fp12 products and Frobenius maps:
//   n = f conj(f)               in Fp6 = Fp2[w^2]    (conj is the p^6 Frobenius)
//   q = frob^2(n) frob^4(n),    s = n q in Fp2       (the norm of Fp6 over Fp2)
//   n^-1 = q s^-1,              f^-1 = conj(f) n^-1  (s^-1: (a - bu) / (a^2 + b^2), Fermat in Fp)
// f = 0 gives s = 0, whose Fermat "inverse" is 0, and the chain returns 0 like the ladder.
//
// On the flat basis sum_k c_k w^k (c_k in Fp2, w^6 = xi = 1 + u):
//   conj:    c_k -> (-1)^k c_k
//   frob:    c_k -> conj(c_k) g1_k,  g1_k = xi^(k (p - 1) / 6)
//   frob^2:  c_k -> c_k g2_k,        g2_k = xi^(k (p^2 - 1) / 6) = g1_k conj(g1_k), in Fp
// The constants are computed from host_arith.h at first use (fe_consts), never pasted.
#pragma once
#include <stdint.h>

#include <vector>

#include "pairing.h"

namespace bh {

enum : uint8_t {
  FE_MUL = 0,    // slot[dst] = slot[a] slot[b]; dst differs from a and b
  FE_CONJ,       // slot[dst] = conj(slot[a])
  FE_FROB,       // slot[dst] = frob(slot[a])
  FE_FROB2,      // slot[dst] = frob^2(slot[a])
  FE_SCALE_INV,  // slot[dst] = slot[a] / (coefficient 0 of slot[b]), 0 for a zero divisor
  FE_COPY,       // slot[dst] = slot[a]
};
struct FeStep {
  uint8_t op, dst, a, b;
};
constexpr int FE_SLOTS = 6;  // Fp12 values per lane; slot 0 is the input and the result
constexpr uint64_t FE_X_ABS[1] = {0xd201000000010000ull};
constexpr uint64_t FE_C[2] = {0x8c00aaab0000aaabull, 0x396c8c005555e156ull};  // (x - 1)^2 / 3

// slot[dst] = slot[src]^e as squarings and products by slot[src], alternating between dst and tmp
// so that no product writes a slot it reads and the last one writes dst (src differs from both)
inline void fe_emit_pow(std::vector<FeStep>& p, int dst, int tmp, int src, const uint64_t* e, int words) {
  int top = 64 * words - 1;
  while (!((e[top / 64] >> (top % 64)) & 1)) top--;
  int nops = top;
  for (int b = 0; b < top; b++) nops += (int)((e[b / 64] >> (b % 64)) & 1);
  int cur = src, i = 0;
  auto target = [&] { return ((nops - 1 - i++) & 1) ? tmp : dst; };
  for (int b = top - 1; b >= 0; b--) {
    int t = target();
    p.push_back({FE_MUL, (uint8_t)t, (uint8_t)cur, (uint8_t)cur});
    cur = t;
    if ((e[b / 64] >> (b % 64)) & 1) {
      t = target();
      p.push_back({FE_MUL, (uint8_t)t, (uint8_t)cur, (uint8_t)src});
      cur = t;
    }
  }
}

inline const std::vector<FeStep>& fe_program() {
  static const std::vector<FeStep> prog = [] {
    std::vector<FeStep> p;
    auto op = [&](uint8_t o, int d, int a, int b = 0) { p.push_back({o, (uint8_t)d, (uint8_t)a, (uint8_t)b}); };
    // easy part: slot 0 = f
    op(FE_CONJ, 1, 0);          // 1 = conj(f)
    op(FE_MUL, 2, 0, 1);        // 2 = n
    op(FE_FROB2, 3, 2);         // 3 = frob^2(n)
    op(FE_FROB2, 4, 3);         // 4 = frob^4(n)
    op(FE_MUL, 5, 3, 4);        // 5 = q
    op(FE_MUL, 3, 2, 5);        // 3 = s
    op(FE_SCALE_INV, 4, 5, 3);  // 4 = n^-1
    op(FE_MUL, 2, 1, 4);        // 2 = f^-1
    op(FE_MUL, 3, 1, 2);        // 3 = t
    op(FE_FROB2, 1, 3);
    op(FE_MUL, 0, 1, 3);  // 0 = m
    // hard part
    fe_emit_pow(p, 1, 2, 0, FE_C, 2);  // 1 = a = m^c
    fe_emit_pow(p, 2, 3, 1, FE_X_ABS, 1);
    op(FE_CONJ, 3, 2);  // 3 = a^x
    op(FE_FROB, 2, 1);
    op(FE_MUL, 4, 3, 2);  // 4 = b
    fe_emit_pow(p, 1, 2, 4, FE_X_ABS, 1);
    fe_emit_pow(p, 2, 3, 1, FE_X_ABS, 1);  // 2 = (b^x)^x: the two conjugations cancel
    op(FE_FROB2, 1, 4);
    op(FE_MUL, 3, 2, 1);
    op(FE_CONJ, 1, 4);
    op(FE_MUL, 2, 3, 1);  // 2 = d
    op(FE_MUL, 1, 2, 0);
    op(FE_COPY, 0, 1);
    return p;
  }();
  return prog;
}

struct FeConsts {
  Fp2 g1[6];  // xi^(k (p - 1) / 6), g1[0] = 1
  Fp g2[6];   // xi^(k (p^2 - 1) / 6), g2[0] = 1
};

inline const FeConsts& fe_consts() {
  static const FeConsts c = [] {
    uint64_t e[6];  // (p - 1) / 6 by long division; p = 1 mod 6
    memcpy(e, hostc::FP_P, sizeof e);
    e[0] -= 1;
    uint64_t rem = 0;
    for (int i = 5; i >= 0; i--) {
      const u128 t = ((u128)rem << 64) | e[i];
      e[i] = (uint64_t)(t / 6);
      rem = (uint64_t)(t % 6);
    }
    const Fp2 xi{Fp::one(), Fp::one()};
    Fp2 g = Fp2::one();
    for (int i = 5; i >= 0; i--)
      for (int b = 63; b >= 0; b--) {
        g = sqr(g);
        if ((e[i] >> b) & 1) g = mul(g, xi);
      }
    FeConsts r;
    r.g1[0] = Fp2::one();
    r.g2[0] = Fp::one();
    for (int k = 1; k < 6; k++) {
      r.g1[k] = mul(r.g1[k - 1], g);
      r.g2[k] = add(sqr(r.g1[k].c0), sqr(r.g1[k].c1));  // g1_k^(p + 1) = g1_k conj(g1_k)
    }
    return r;
  }();
  return c;
}

inline Fp12 fe_chain_host(const Fp12& f) {
  const FeConsts& C = fe_consts();
  Fp12 s[FE_SLOTS];
  for (auto& v : s) v = f12_one();
  s[0] = f;
  for (const FeStep& st : fe_program()) {
    const Fp12 &a = s[st.a], &b = s[st.b];
    Fp12 r;
    switch (st.op) {
      case FE_MUL: r = f12_mul(a, b); break;
      case FE_CONJ:
        for (int k = 0; k < 6; k++) r.c[k] = (k & 1) ? neg(a.c[k]) : a.c[k];
        break;
      case FE_FROB:
        for (int k = 0; k < 6; k++) r.c[k] = mul(Fp2{a.c[k].c0, neg(a.c[k].c1)}, C.g1[k]);
        break;
      case FE_FROB2:
        for (int k = 0; k < 6; k++) r.c[k] = Fp2{mul(a.c[k].c0, C.g2[k]), mul(a.c[k].c1, C.g2[k])};
        break;
      case FE_SCALE_INV: {
        const Fp2 i = inv(b.c[0]);
        for (int k = 0; k < 6; k++) r.c[k] = mul(a.c[k], i);
        break;
      }
      default: r = a; break;
    }
    s[st.dst] = r;
  }
  return s[0];
}

}  // namespace bh
