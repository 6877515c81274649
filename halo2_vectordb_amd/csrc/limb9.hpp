// Field elements as nine 29-bit limbs ("L9"): the register / LDS form used inside the NTT tiles and the MSM accumulator.
//
// value = sum l[k] * 2^(29k).  "Normalised": l[0..7] < 2^29 (+ a few units after a parallel carry pass; exactly below
// 2^29 after l9_carry or a product).  Between normalisations limbs may grow to 7 * 2^29 (sums of a few normalised
// values); a product accepts a first operand with limbs below 6.1 * 2^29 and a normalised second operand
// (mont_core29, field.hpp).  Add and subtract propagate no carries: 9, resp. 18, plain 32-bit operations.
// Values are only ever defined modulo p; what is tracked (in comments, at every use) is an upper bound in multiples
// of p, because a product of values A, B returns something below A * B / 2^261 + p.
#pragma once
#include <math.h>

#include "field.hpp"

namespace vdb {

struct L9 {
  uint32_t l[9];
};
HD L9 l9_split(const u256& a) {
  L9 r;
#pragma unroll
  for (int k = 0; k < 9; k++) {
    int pb = 29 * k, wb = pb >> 5, ob = pb & 31;
    uint32_t lo = a.w[wb];
    uint32_t hi = wb + 1 < 8 ? a.w[wb + 1 < 8 ? wb + 1 : 0] : 0u;
    r.l[k] = ob ? ((lo >> ob) | (hi << (32 - ob))) : lo;
    if (k < 8) r.l[k] &= 0x1fffffffu;
  }
  return r;
}
// 32 * a as nine limbs (a < 2^256, so 32 a < 2^261): the second operand that keeps a nine-limb product of two values in
// ordinary Montgomery form (R = 2^256) in that form: (x R)(32 y R) / 2^261 = x y R
HD L9 l9_split32(const u256& a) {
  L9 r;
  r.l[0] = (a.w[0] << 5) & 0x1fffffffu;
#pragma unroll
  for (int k = 1; k < 9; k++) {
    int pb = 29 * k - 5, wb = pb >> 5, ob = pb & 31;
    uint32_t lo = a.w[wb];
    uint32_t hi = wb + 1 < 8 ? a.w[wb + 1 < 8 ? wb + 1 : 0] : 0u;
    r.l[k] = ob ? ((lo >> ob) | (hi << (32 - ob))) : lo;
    if (k < 8) r.l[k] &= 0x1fffffffu;
  }
  return r;
}
// exactly normalised limbs of a value below 2^256 -> eight words
HD u256 l9_pack(const L9& L) {
  u256 r;
  r.w[0] = L.l[0] | (L.l[1] << 29);
  r.w[1] = (L.l[1] >> 3) | (L.l[2] << 26);
  r.w[2] = (L.l[2] >> 6) | (L.l[3] << 23);
  r.w[3] = (L.l[3] >> 9) | (L.l[4] << 20);
  r.w[4] = (L.l[4] >> 12) | (L.l[5] << 17);
  r.w[5] = (L.l[5] >> 15) | (L.l[6] << 14);
  r.w[6] = (L.l[6] >> 18) | (L.l[7] << 11);
  r.w[7] = (L.l[7] >> 21) | (L.l[8] << 8);
  return r;
}
// one parallel carry pass: limbs below 2^32 in, limbs below 2^29 + 8 out (top limb takes what is left: it needs room for a carry
// of at most 7, i.e. value below 2^264 - 7 * 2^232)
HD void l9_renorm(L9& x) {
  uint32_t c[8];
#pragma unroll
  for (int k = 0; k < 8; k++) c[k] = x.l[k] >> 29;
#pragma unroll
  for (int k = 0; k < 8; k++) x.l[k] &= 0x1fffffffu;
#pragma unroll
  for (int k = 1; k < 9; k++) x.l[k] += c[k - 1];
}
// full carry propagation: limbs 0..7 exactly below 2^29.  Every limb takes the carry of the one below before it gives its own:
// limbs at most 2^32 - 8 in (a carry is then at most 7 and nothing wraps)
HD void l9_carry(L9& x) {
#pragma unroll
  for (int k = 0; k < 8; k++) {
    x.l[k + 1] += x.l[k] >> 29;
    x.l[k] &= 0x1fffffffu;
  }
}
HD L9 l9_add(const L9& a, const L9& b) {
  L9 r;
#pragma unroll
  for (int k = 0; k < 9; k++) r.l[k] = a.l[k] + b.l[k];
  return r;
}
// a - t + K p, limb-wise.  `ckp` is K p written with limbs c[0] = v_0 + 2^29, c[k] = v_k + 2^29 - 1 (0 < k < 8),
// c[8] = v_8 - 1 (l9_offset_limbs).  Exact — limb k is a_k + c_k - t_k as integers, for any a whose sums stay below 2^32 — when
// t_k <= c_k for every k.  Limbs 0..7 of c are at least 2^29 - 1, so for a t with limbs 0..7 below 2^29 the condition is on the top
// limb alone: t_8 <= c_8 = floor(K p / 2^232) - 1, which every value below (K - 2^-22) p meets (in particular every value below
// (K - 1) p; the MSM subtracts values below 7.5 q from 8 q).  t_8 = c_8 + 1 wraps.  A t as l9_renorm leaves it (limbs up to
// 2^29 + 7) is covered by the offsets whose limbs v_k are all at least 8 — 9 r, 14 r, 34 r, 8 q, 2 q, but not 2 r (v_0 = 2).
// (tests/test_l9_cpu.py: test_sub_domain_edge, test_sub_renormalised_subtrahend)
HD L9 l9_sub(const L9& a, const L9& t, const uint32_t (&ckp)[9]) {
  L9 r;
#pragma unroll
  for (int k = 0; k < 9; k++) r.l[k] = a.l[k] + (ckp[k] - t.l[k]);
  return r;
}
// K p - t
HD L9 l9_neg(const L9& t, const uint32_t (&ckp)[9]) {
  L9 r;
#pragma unroll
  for (int k = 0; k < 9; k++) r.l[k] = ckp[k] - t.l[k];
  return r;
}
// a * b / 2^261 (+ less than p): exactly normalised limbs
template <class M>
HD L9 l9_mul(const L9& a, const L9& b) {
  L9 r;
  mont_core29<M>(r.l, a.l, b.l);
  return r;
}
// w * v mod p (below 3 p, exactly normalised limbs) for a constant w given as its plain residue with wq = floor(w 2^261 / p)
template <class M>
HD L9 l9_mul_shoup(const L9& v, const L9& w, const L9& wq) {
  L9 r;
  shoup_core29<M>(r.l, v.l, w.l, wq.l);
  return r;
}
// Shoup companions (host and device code: the stage tables and the kernel-argument constants are built on the host, the inter-pass
// records on the device, all from these two functions).  The nine 29-bit limbs of a < 2^256:
HD void limbs29(const u256& a, uint32_t out[9]) {
#pragma unroll
  for (int k = 0; k < 9; k++) {
    const int bit = 29 * k, wd = bit >> 5, sh = bit & 31;
    uint64_t v = (uint64_t)a.w[wd] >> sh;
    if (sh && wd + 1 < 8) v |= (uint64_t)a.w[wd + 1 < 8 ? wd + 1 : 0] << (32 - sh);
    out[k] = (uint32_t)v & 0x1fffffffu;
  }
}
// out[0..8]: the limbs of w (canonical, below r); out[9..17]: those of w' = floor(w 2^261 / r), by 261 steps of long division (the
// remainder starts at w < r and stays below 2 r < 2^255 before each conditional subtraction; bit b of w' is bit b % 29 of limb b / 29)
HD void shoup_pair29(const u256& w, uint32_t out[18]) {
  limbs29(w, out);
  const u256 p = mod_p<Fr>();
  u256 r = w;
#pragma unroll
  for (int k = 8; k >= 0; k--) {
    uint32_t d = 0;
    for (int j = 28; j >= 0; j--) {
      u256 s, t;
      u256_add(s, r, r);
      const uint32_t borrow = u256_sub(t, s, p);
      r = borrow ? s : t;
      d |= (borrow ^ 1u) << j;
    }
    out[9 + k] = d;
  }
}
// (a1 * b1 + a2 * b2) / 2^261 (+ less than p) with one reduction; limbs of a1 and a2 together below 6 * 2^29
template <class M>
HD L9 l9_mul2(const L9& a1, const L9& b1, const L9& a2, const L9& b2) {
  L9 r;
  mont_core29_2<M>(r.l, a1.l, b1.l, a2.l, b2.l);
  return r;
}
// a * a / 2^261 (+ less than p) for a normalised a (limbs below 2^29 + 8)
template <class M>
HD L9 l9_sqr(const L9& a) {
  L9 r;
  mont_sqr_core29<M>(r.l, a.l);
  return r;
}
// exactly normalised limbs of a value below 2p -> canonical eight words
template <class M>
HD u256 l9_canon(const L9& t) {
  return lazy_canon<M>(l9_pack(t));
}
// all limbs zero, or equal to p: the two representations of 0 below 2p (exactly normalised input)
template <class M>
HD bool l9_is_zero_mod(const L9& t) {
  uint32_t z = 0, e = 0;
#pragma unroll
  for (int k = 0; k < 9; k++) {
    z |= t.l[k];
    e |= t.l[k] ^ M::P29[k];
  }
  return z == 0 || e == 0;
}
// host: the dominating limbs of K p for l9_sub; returns the largest of limbs 0..7 in units of 2^29 (the growth a
// difference adds to a limb)
template <class M>
inline double l9_offset_limbs(uint32_t K, uint32_t out[9]) {
  uint64_t carry = 0;
  for (int k = 0; k < 9; k++) {
    uint64_t v = (uint64_t)K * M::P29[k] + carry;
    out[k] = (uint32_t)(v & 0x1fffffffu);
    carry = v >> 29;
  }
  out[8] += (uint32_t)(carry << 29);
  out[0] += 1u << 29;
  for (int k = 1; k < 8; k++) out[k] += (1u << 29) - 1;
  out[8] -= 1;
  double cmax = 0;
  for (int k = 0; k < 8; k++) cmax = fmax(cmax, (double)out[k] / (double)(1u << 29));
  return cmax;
}

// limbs below 2^32, value below 2^259 -> canonical eight words without a multiplication and without a carry pass of its own:
// subtract q r with q = floor(top / (r_8 + 1)), top = l_8 + (l_7 >> 29) — the value's true top limb or one less (what limbs 0..6
// and the low 29 bits of l_7 carry into bit 232 is at most 1) — so q is never too large and, as an exact quotient, at most 1 too
// small (both occur in tests/test_gpu_l9.py; MU's rounding may cost one more); the subtraction's 64-bit column accumulator
// propagates every carry on the way, and two conditional subtractions (2 r, then r) finish anything below 4 r
__device__ __forceinline__ u256 l9_canon_wide(L9 x) {
  constexpr uint32_t MU = 2840127191u;  // floor(2^53 / (0x30644e + 1))
  const uint32_t q = __umulhi((x.l[8] + (x.l[7] >> 29)) << 3, MU) >> 24;
  // x + q (2^261 - r) mod 2^261
  uint64_t acc = 0;
#pragma unroll
  for (int k = 0; k < 9; k++) {
    const uint32_t nk = (k == 0 ? 0x20000000u : 0x1fffffffu) - FrParams::P29[k];  // limbs of 2^261 - r
    acc += (uint64_t)x.l[k] + (uint64_t)q * nk;
    x.l[k] = (uint32_t)acc & 0x1fffffffu;
    acc >>= 29;
  }
  u256 v = l9_pack(x), t, p2, pp = mod_p<Fr>();
  u256_add(p2, pp, pp);
  uint32_t keep = u256_sub(t, v, p2);
#pragma unroll
  for (int i = 0; i < 8; i++) v.w[i] = keep ? v.w[i] : t.w[i];
  return lazy_canon<Fr>(v);
}

}  // namespace vdb
