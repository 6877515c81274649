// The digit code of the MSM sort: sign fold, signed window digits, and the 8-byte record of a short scalar, in a header of their own so
// that tools/msm_digits_probe.hip reaches the very functions k_msm_sort (msm.hip) uses and tests/test_msm_digits_cpu.py can hold them
// to big integers.
#pragma once
#include "field.hpp"

namespace vdb {

// canonical scalar -> (folded magnitude, sign)
HD bool fold_scalar(u256& s) {
  // (r-1)/2
  const uint32_t H[8] = {0xf8000000u, 0xa1f0fac9u, 0x3cdcb848u, 0x9419f424u, 0x40c0ac2eu, 0xdc2822dbu, 0x7098d014u, 0x18322739u};
  u256 half;
#pragma unroll
  for (int i = 0; i < 8; i++) half.w[i] = H[i];
  // s > half  <=>  !(half >= s)
  if (!u256_geq(half, s)) {
    u256 r = mod_p<Fr>(), t;
    u256_sub(t, r, s);
    s = t;
    return true;
  }
  return false;
}

// signed window digits of a folded magnitude s (nb = its bit length): f(window, |digit|, negative)
template <class F>
HD void emit_digits(u256 s, bool neg, uint32_t nb, uint32_t c, uint32_t W, F&& f, size_t idx = 0) {
  uint32_t carry = 0;
  const uint32_t half = 1u << (c - 1), full = 1u << c;
  // witness scalars are mostly short: stop after the window that can still receive a carry
  uint32_t wend = nb / c + 2;
  if (wend > W) wend = W;
  for (uint32_t j = 0; j < wend; j++) {
    uint32_t d = (s.w[0] & (full - 1)) + carry;
    s = u256_shr_small(s, c);
    bool dneg = false;
    if (d > half) {
      d = full - d;
      dneg = true;
      carry = 1;
    } else {
      carry = 0;
    }
    if (d) f(j, d, neg != dneg, idx);
  }
}
// same for a magnitude below 2^32
template <class F>
HD void emit_digits32(uint32_t mag, bool neg, uint32_t nb, uint32_t c, uint32_t W, F&& f, size_t idx) {
  uint32_t carry = 0;
  const uint32_t half = 1u << (c - 1), full = 1u << c;
  uint32_t wend = nb / c + 2;
  if (wend > W) wend = W;
  for (uint32_t j = 0; j < wend; j++) {
    uint32_t d = (mag & (full - 1)) + carry;
    mag >>= c;
    bool dneg = false;
    if (d > half) {
      d = full - d;
      dneg = true;
      carry = 1;
    } else {
      carry = 0;
    }
    if (d) f(j, d, neg != dneg, idx);
  }
}

// ---- the scaled-short record ---------------------------------------------------------------------------------------------------------
// A folded magnitude s != 0 is written s = s' * 2^(c * j0), j0 = (trailing zero bits of s) / c the first window that holds a bit.  It is
// short iff s' < 2^32 and its bit length nb' is at most short_bits = min(3c - 1, 32): at most three windows of its own and the one
// that takes the last carry.  The record of a short scalar:
//   bits 0-31 s'   bit 32 sign   bits 33-39 j0 (W <= 127 for every window size c >= 2)   bits 40-47 nb'   bit 63 MSM_REC_VALID
#define MSM_REC_VALID (1ull << 63)

HD uint32_t msm_short_bits(uint32_t c) { return 3 * c - 1 < 32 ? 3 * c - 1 : 32; }
// x / c for x < 256 is (x * msm_recip16(c)) >> 16: with inv = (2^16 + e) / c, 0 <= e < c, the product is x / c + x e / (c 2^16), and the
// excess stays below 255 / 2^16 < 1 / c, the distance of x / c from the next integer
HD uint32_t msm_recip16(uint32_t c) { return (65536u + c - 1) / c; }

// trailing zero bits (256 for zero)
HD unsigned u256_ctz(const u256& a) {
  unsigned r = 256;
#pragma unroll
  for (int i = 7; i >= 0; i--)
    if (a.w[i]) r = 32u * i + (unsigned)__builtin_ctz(a.w[i]);
  return r;
}
// bits [pos, pos + 32) of a, pos < 256; static limb indices only (see u256_shr)
HD uint32_t u256_window32(const u256& a, unsigned pos) {
  const unsigned ws = pos >> 5, bs = pos & 31;
  uint32_t lo = a.w[0], hi = a.w[1];
#pragma unroll
  for (int i = 1; i < 8; i++)
    if (ws == (unsigned)i) {
      lo = a.w[i];
      hi = i + 1 < 8 ? a.w[i + 1 < 8 ? i + 1 : 0] : 0u;
    }
  return (uint32_t)(((((uint64_t)hi) << 32) | lo) >> bs);
}

// classification of a folded magnitude s != 0 of bit length nb: j0 and nb' always, s' (mag) when the scalar is short
HD bool msm_classify(const u256& s, uint32_t nb, uint32_t c, uint32_t inv_c, uint32_t short_bits, uint32_t& mag, uint32_t& nbs, uint32_t& j0) {
  j0 = (u256_ctz(s) * inv_c) >> 16;
  const uint32_t sh = c * j0;
  nbs = nb - sh;
  mag = 0;
  if (nbs > short_bits) return false;
  mag = u256_window32(s, sh);  // nb' <= 32: all of s'
  return true;
}

HD unsigned long long msm_rec_encode(uint32_t mag, bool neg, uint32_t nbs, uint32_t j0) {
  return MSM_REC_VALID | ((unsigned long long)nbs << 40) | ((unsigned long long)j0 << 33) | ((unsigned long long)(neg ? 1 : 0) << 32) | mag;
}
struct MsmRec {
  uint32_t mag, nbs, j0;
  bool neg;
};
HD MsmRec msm_rec_decode(unsigned long long r) {
  MsmRec o;
  o.mag = (uint32_t)r;
  o.neg = ((r >> 32) & 1) != 0;
  o.j0 = (uint32_t)(r >> 33) & 0x7fu;
  o.nbs = (uint32_t)(r >> 40) & 0xffu;
  return o;
}
// the digits of a short scalar: those of s' over the W - j0 windows that remain, handed on as windows j0, j0 + 1, ...
template <class F>
HD void emit_digits_short(uint32_t mag, bool neg, uint32_t nbs, uint32_t j0, uint32_t c, uint32_t W, F&& f, size_t idx) {
  emit_digits32(mag, neg, nbs, c, W - j0, [&](uint32_t j, uint32_t d, bool ng, size_t i) { f(j + j0, d, ng, i); }, idx);
}

}  // namespace vdb
