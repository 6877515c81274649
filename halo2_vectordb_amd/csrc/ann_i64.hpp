// The native-integer head of a distance over PACKED rows (include/vdb.h vdb_fp_pack_i64_dev, vdb_ann_search_i64_dev): one
// signed 64-bit integer a coordinate in place of a 32-byte Montgomery word.  Shared by k_ann_search_i64 and k_ann_norm_sums_i64
// (witness.hip); what the packed word is, what a term is and how a sum returns to the field are stated here once.
//
// The packed word.  The signed value of a canonical field word a is a when a < 2^63 and -(r - a) when r - a < 2^63; every other word is
// NOT PACKABLE (so -2^63 is excluded, and the definition does not depend on P).  quantize(x, P) of real data lies in that domain.
//
// The head, x the vector's word and y the query's (assign_term's operand order), P in 32 .. 63:
//   euclidean  d = |x - y| as an unsigned 64-bit value (below 2^64); the term is (d d) >> P over the 128-bit product
//   cosine     the term is ((__int128)x y) >> P, an ARITHMETIC shift: the floor.  v_signed_div_scale takes floor(p / 2^P) of a
//              non-negative product and -ceil(|p| / 2^P) of a negative one, which is floor(p / 2^P) again.  Norms: sum (x x) >> P
//   manhattan  the term is |x - y|
//   hamming    the term is x == y
// Bounds: a product is below 2^128 and P >= 32, so a term is below 2^96 in magnitude; dim <= 2^24, so a sum is below 2^120: the 128-bit
// accumulator never wraps, the sum stays far below r, and the integer sum IS the field sum of the terms (fr_add of them, in any order).
// The rescale is per term — sum floor(p_i / 2^P) is not floor(sum p_i / 2^P) — so the head is no GEMM over limbs.
#pragma once
#include <stdint.h>

#include "field.hpp"

namespace vdb {

typedef unsigned __int128 ann_u128;
typedef __int128 ann_i128;

// the metrics of a head, M_EUCLID .. M_HAMMING of gadgets.hpp in their order
enum { ANN_I64_EUCLID = 0, ANN_I64_COSINE = 1, ANN_I64_MANHATTAN = 2, ANN_I64_HAMMING = 3 };

// words of the dim axis staged at a time: four times the field form's 16, a quarter of its barriers a pair
#define ANN_I64_DC 64

// p >> P for P in 32 .. 63 on the two halves (a shift of the 128-bit type by a runtime amount also selects for amounts of 64 and more);
// ARITH: the high half keeps its sign, the floor of a negative product
template <bool ARITH>
HD ann_u128 ann_i64_shr(ann_u128 p, uint32_t P) {
  const uint64_t lo = (uint64_t)p, hi = (uint64_t)(p >> 64);
  const uint64_t h = ARITH ? (uint64_t)((int64_t)hi >> P) : hi >> P;
  return ((ann_u128)h << 64) | (ann_u128)((lo >> P) | (hi << (64 - P)));
}
HD uint64_t ann_i64_absdiff(int64_t x, int64_t y) { return x >= y ? (uint64_t)x - (uint64_t)y : (uint64_t)y - (uint64_t)x; }

// One term added to a head sum.  The sum is kept as an unsigned 128-bit pattern; cosine's is two's complement.
template <int METRIC>
HD ann_u128 ann_i64_accumulate(ann_u128 acc, int64_t x, int64_t y, uint32_t P) {
  if (METRIC == ANN_I64_HAMMING) return acc + (ann_u128)(x == y ? 1u : 0u);
  if (METRIC == ANN_I64_COSINE) return acc + ann_i64_shr<true>((ann_u128)((ann_i128)x * (ann_i128)y), P);
  const uint64_t d = ann_i64_absdiff(x, y);
  if (METRIC == ANN_I64_MANHATTAN) return acc + (ann_u128)d;
  return acc + ann_i64_shr<false>((ann_u128)d * (ann_u128)d, P);
}
// a term of a norm: (x x) >> P, never negative
HD ann_u128 ann_i64_norm_term(int64_t x, uint32_t P) {
  const uint64_t a = x < 0 ? 0 - (uint64_t)x : (uint64_t)x;
  return ann_i64_shr<false>((ann_u128)a * (ann_u128)a, P);
}
// A head sum as a field word (Montgomery): the magnitude to u256, to_mont, fr_neg for a negative sum.  `is_signed`: cosine.
HD u256 ann_i64_sum_to_fr(ann_u128 s, bool is_signed) {
  const bool neg = is_signed && (ann_i128)s < 0;
  const ann_u128 m = neg ? (ann_u128)0 - s : s;
  u256 c = u256_zero();
  c.w[0] = (uint32_t)m;
  c.w[1] = (uint32_t)(m >> 32);
  c.w[2] = (uint32_t)(m >> 64);
  c.w[3] = (uint32_t)(m >> 96);
  const u256 f = to_mont<Fr>(c);
  return neg ? fr_neg(f) : f;
}
// The packed value of the field word `a` (Montgomery); false where it is not packable.
HD bool ann_i64_pack(const u256& a, int64_t* out) {
  const u256 c = from_mont<Fr>(a);
  u256 m;
  u256_sub(m, mod_p<Fr>(), c);
  const bool pos = (c.w[2] | c.w[3] | c.w[4] | c.w[5] | c.w[6] | c.w[7] | (c.w[1] >> 31)) == 0;
  const bool neg = (m.w[2] | m.w[3] | m.w[4] | m.w[5] | m.w[6] | m.w[7] | (m.w[1] >> 31)) == 0;
  const uint64_t cv = ((uint64_t)c.w[1] << 32) | c.w[0], mv = ((uint64_t)m.w[1] << 32) | m.w[0];
  *out = pos ? (int64_t)cv : (int64_t)(0 - mv);
  return pos || neg;
}

}  // namespace vdb
