// The MSM accumulator in nine-limb form: the mixed addition and the doubling that k_msm_accum (msm.hip) runs, in a header of their
// own so that tools/l9_probe.hip reaches the very functions the kernel uses.
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

}  // namespace vdb
