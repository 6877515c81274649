// The MSM accumulator in nine-limb form: the mixed addition and the doubling that k_msm_accum (msm.hip) runs and the full addition
// that the bucket folding (k_msm_combine, k_msm_reduce) runs, in a header of their own so that tools/l9_probe.hip and
// tools/ecl9_probe.hip reach the very functions the kernels use.
#pragma once
#include "ec.hpp"
#include "limb9.hpp"

namespace vdb {

// ---- accumulation in nine-limb form ------------------------------------------------------------------------------
// Inside k_msm_accum coordinates are L9 values in Montgomery form with R' = 2^261 (what a 9 x 29-bit product divides
// by), so products need no operand shift, additions and subtractions are carry-free, and nothing is packed / split
// between the ten products of a mixed addition.  Bounds (multiples of q) are tracked in the comments of madd_l9.
struct MsmL9Consts {
  uint32_t c2[9], c8[9];  // 2q and 8q with dominating limbs (l9_sub)
  u256 one_rp;            // 2^261 mod q            (1 in R' form)
  u256 to_std;            // 2^256 mod q: x R' form -> standard Montgomery form (R = 2^256)
  u256 to_rp;             // 2^266 mod q: standard form -> R' form
};
struct AccL9 {
  L9 x, y, zz, zzz;  // exactly normalised; x < 7.5 q, y < 3.6 q, zz, zzz < 1.1 q
};

// rare exact path, acc == p as points: acc = 2p from the affine point   [mdbl-2008-s-1, 5M + 2S]
// x, y exactly normalised, x < q, y <= 2q
__device__ __forceinline__ void mdbl_l9(AccL9& acc, bool& ident, const L9& x, const L9& y, const MsmL9Consts& K) {
  if (l9_is_zero_mod<Fq>(y)) {  // 2-torsion (not on BN254 G1; kept for exactness of the group law)
    ident = true;
    return;
  }
  const L9 u = l9_add(y, y);               // limbs < 2 * 2^29, value <= 4q
  L9 un = u;
  l9_renorm(un);
  const L9 v = l9_sqr<Fq>(un);             // < 1.1 q
  const L9 w = l9_mul<Fq>(u, v);           // < 1.03 q
  const L9 sv = l9_mul<Fq>(x, v);          // < 1.01 q
  const L9 xx = l9_mul<Fq>(x, x);          // < 1.01 q
  const L9 m = l9_add(l9_add(xx, xx), xx); // limbs < 3 * 2^29, value < 3.1 q
  L9 mn = m;
  l9_renorm(mn);
  const L9 mm = l9_sqr<Fq>(mn);            // < 1.06 q
  const L9 ns = l9_neg(sv, K.c2);
  L9 x3 = l9_add(l9_add(mm, ns), ns);      // mm - 2 sv + 4q: limbs < 5 * 2^29, value < 5.1 q
  l9_carry(x3);
  const L9 td = l9_sub(sv, x3, K.c8);      // value < 9.1 q
  const L9 m1 = l9_mul<Fq>(td, mn);        // < 1.2 q
  const L9 m2 = l9_mul<Fq>(w, y);          // < 1.02 q
  L9 y3 = l9_sub(m1, m2, K.c2);
  l9_carry(y3);
  acc.x = x3;
  acc.y = y3;
  acc.zz = v;
  acc.zzz = w;
}

// acc += (neg ? -p : p), p affine in R' form and not the identity   [madd-2008-s, 8M + 2S]
__device__ __forceinline__ void madd_l9(AccL9& acc, bool& ident, const Affine& p, bool neg, const MsmL9Consts& K) {
  L9 x2 = l9_split(p.x), y2 = l9_split(p.y);  // canonical: exactly normalised, below q
  if (neg) {
    y2 = l9_neg(y2, K.c2);  // 2q - y: limbs below 2 * 2^29
    l9_carry(y2);
  }
  if (ident) {
    acc.x = x2;
    acc.y = y2;
    acc.zz = l9_split(K.one_rp);
    acc.zzz = acc.zz;
    ident = false;
    return;
  }
  const L9 u2 = l9_mul<Fq>(acc.zz, x2);    // < 1.01 q
  const L9 s2 = l9_mul<Fq>(acc.zzz, y2);   // < 1.02 q
  L9 pd = l9_sub(u2, acc.x, K.c8);         // u2 - x1 + 8q: limbs < 3 * 2^29, value < 9.1 q  (x1 < 7.5 q: inside l9_sub's domain, top limb <= c8[8])
  L9 rd = l9_sub(s2, acc.y, K.c8);         // s2 - y1 + 8q: same bounds
  L9 pn = pd, rn = rd;
  l9_renorm(pn);
  l9_renorm(rn);
  const L9 pp = l9_sqr<Fq>(pn);            // < 1.5 q
  const L9 r2 = l9_sqr<Fq>(rn);            // < 1.5 q
  if (l9_is_zero_mod<Fq>(pp)) {            // same x (exact test on the product: q is prime)
    if (l9_is_zero_mod<Fq>(r2)) mdbl_l9(acc, ident, x2, y2, K);  // same point
    else ident = true;                                            // opposite points
    return;
  }
  const L9 ppp = l9_mul<Fq>(pd, pp);       // < 1.09 q
  const L9 qq = l9_mul<Fq>(acc.x, pp);     // < 1.07 q
  const L9 nq = l9_neg(qq, K.c2);          // 2q - qq
  L9 x3 = l9_add(l9_add(l9_sub(r2, ppp, K.c2), nq), nq);  // r2 - ppp - 2 qq + 6q: limbs < 6.9 * 2^29, value < 7.5 q
  l9_carry(x3);
  const L9 td = l9_sub(qq, x3, K.c8);      // qq - x3 + 8q: limbs < 3 * 2^29, value < 9.1 q  (x3 < 7.5 q: as above; tests/test_l9_cpu.py::test_sub_domain_edge)
  // y3 = td * rn - y1 * ppp as ONE reduced sum of two products: td * rn + (8q - y1) * ppp  (limbs 3 + 2 units,
  // values 9.1 q * 9.1 q + 8 q * 1.1 q: the result is exactly normalised and below 1.6 q)
  const L9 ny = l9_neg(acc.y, K.c8);
  const L9 y3 = l9_mul2<Fq>(td, rn, ny, ppp);
  acc.zz = l9_mul<Fq>(acc.zz, pp);
  acc.zzz = l9_mul<Fq>(acc.zzz, ppp);
  acc.x = x3;
  acc.y = y3;
}

// ---- bucket folding in nine-limb form ----------------------------------------------------------------------------
// The full addition of two accumulators (k_msm_combine, k_msm_reduce) and the doubling it falls into when both stand for
// the same point.  Operands and results are AccL9 values inside AccL9's bounds (what madd_l9, mdbl_l9 and these two
// leave: x < 7.5 q, y < 3.6 q, zz, zzz < 1.1 q, limbs 0..7 exactly below 2^29), the identity is a flag beside the value.
// A product of values A q and B q is below (A B / 169 + 1) q, since q / 2^261 < 1 / 169.  Host and device: the host
// form is what tools/ecl9_probe.hip runs for tests/test_ecl9_cpu.py.

// acc = 2 acc   [dbl-2008-s-1, a = 0: 6M + 3S, two of the products inside the two-product core]
HD void xyzz_dbl_l9(AccL9& acc, bool& ident, const MsmL9Consts& K) {
  if (ident) return;
  const L9 u = l9_add(acc.y, acc.y);           // limbs < 2 * 2^29, value < 7.2 q
  L9 un = u;
  l9_renorm(un);
  const L9 v = l9_sqr<Fq>(un);                 // < 1.31 q
  if (l9_is_zero_mod<Fq>(v)) {                 // y = 0: 2-torsion (not on BN254 G1; kept for exactness of the group law)
    ident = true;
    return;
  }
  // (the denominators first: the old zz and zzz are then done with, which keeps fewer values live through the rest)
  const L9 w = l9_mul<Fq>(u, v);               // < 1.06 q
  acc.zz = l9_mul<Fq>(acc.zz, v);              // < 1.01 q
  acc.zzz = l9_mul<Fq>(acc.zzz, w);            // < 1.01 q
  const L9 s = l9_mul<Fq>(acc.x, v);           // < 1.06 q
  const L9 xx = l9_sqr<Fq>(acc.x);             // < 1.34 q  (x exactly normalised)
  const L9 m = l9_add(l9_add(xx, xx), xx);     // limbs < 3 * 2^29, value < 4.1 q
  L9 mn = m;
  l9_renorm(mn);
  const L9 mm = l9_sqr<Fq>(mn);                // < 1.1 q
  const L9 ns = l9_neg(s, K.c2);               // 2q - s: limbs < 2 * 2^29
  L9 x3 = l9_add(l9_add(mm, ns), ns);          // mm - 2 s + 4q: limbs < 5 * 2^29, value < 5.1 q
  l9_carry(x3);
  const L9 td = l9_sub(s, x3, K.c8);           // s - x3 + 8q: limbs < 3 * 2^29, value < 9.1 q
  // y3 = m (s - x3) - w y1 as one reduced sum: td * mn + (8q - y1) * w  (limbs 3 + 2 units; 9.1 q * 4.1 q + 8 q * 1.06 q: below 1.3 q)
  const L9 ny = l9_neg(acc.y, K.c8);           // y1 < 3.6 q: inside l9_neg's domain
  acc.y = l9_mul2<Fq>(td, mn, ny, w);
  acc.x = x3;
}

// acc += b   [add-2008-s: 12M + 2S, two of the products inside the two-product core; 13 reductions against the 14 of the eight-word
// xyzz_add, and no split / pack / canonical form between them]
HD void xyzz_add_l9(AccL9& acc, bool& ident, const AccL9& b, bool b_ident, const MsmL9Consts& K) {
  if (b_ident) return;
  if (ident) {
    acc = b;
    ident = false;
    return;
  }
  // acc scaled by b's denominators, (u1, s1, zz1 zz2, zzz1 zzz2), is the point of acc again, and b scaled by acc's is (u2, s2, same
  // zz, same zzz): after these six products neither operand is needed any more, not even by the doubling, which matters in
  // k_msm_reduce, where a second accumulator stays live across the addition (161 VGPRs, no scratch).
  const L9 u1 = l9_mul<Fq>(acc.x, b.zz);       // 7.5 q * 1.1 q: < 1.05 q
  const L9 u2 = l9_mul<Fq>(b.x, acc.zz);       // < 1.05 q
  const L9 s1 = l9_mul<Fq>(acc.y, b.zzz);      // 3.6 q * 1.1 q: < 1.03 q
  const L9 s2 = l9_mul<Fq>(b.y, acc.zzz);      // < 1.03 q
  const L9 z12 = l9_mul<Fq>(acc.zz, b.zz);     // < 1.01 q
  const L9 z123 = l9_mul<Fq>(acc.zzz, b.zzz);  // < 1.01 q
  const L9 pd = l9_sub(u2, u1, K.c2);          // u2 - u1 + 2q: limbs < 3 * 2^29, value < 3.1 q  (u1 < 2q: inside l9_sub's domain)
  const L9 rd = l9_sub(s2, s1, K.c2);          // s2 - s1 + 2q: same bounds
  L9 pn = pd, rn = rd;
  l9_renorm(pn);
  l9_renorm(rn);
  const L9 pp = l9_sqr<Fq>(pn);                // < 1.06 q
  const L9 r2 = l9_sqr<Fq>(rn);                // < 1.06 q
  // same x, exact test on the products (q is prime; both are exactly normalised and below 2q): the canonical comparisons of p and r
  // cost 18 and, only behind the first, another 18 logic operations on values the addition needs anyway
  if (l9_is_zero_mod<Fq>(pp)) {
    if (l9_is_zero_mod<Fq>(r2)) {  // same point: double it in the scaled form, which is inside AccL9's bounds
      acc.x = u1;
      acc.y = s1;
      acc.zz = z12;
      acc.zzz = z123;
      xyzz_dbl_l9(acc, ident, K);
    } else {
      ident = true;  // opposite points
    }
    return;
  }
  const L9 ppp = l9_mul<Fq>(pd, pp);           // < 1.02 q
  const L9 qq = l9_mul<Fq>(u1, pp);            // < 1.01 q
  const L9 nq = l9_neg(qq, K.c2);              // 2q - qq
  L9 x3 = l9_add(l9_add(l9_sub(r2, ppp, K.c2), nq), nq);  // r2 - ppp - 2 qq + 6q: limbs < 6.9 * 2^29, value < 7.1 q
  l9_carry(x3);
  const L9 td = l9_sub(qq, x3, K.c8);          // qq - x3 + 8q: limbs < 3 * 2^29, value < 9.1 q  (x3 < 7.5 q)
  // y3 = r (qq - x3) - s1 ppp as one reduced sum: td * rn + (2q - s1) * ppp  (limbs 3 + 2 units; 9.1 q * 3.1 q + 2 q * 1.02 q: below 1.2 q)
  const L9 ns1 = l9_neg(s1, K.c2);
  const L9 y3 = l9_mul2<Fq>(td, rn, ns1, ppp);
  acc.zz = l9_mul<Fq>(z12, pp);                // < 1.01 q
  acc.zzz = l9_mul<Fq>(z123, ppp);             // < 1.01 q
  acc.x = x3;
  acc.y = y3;
}

}  // namespace vdb
