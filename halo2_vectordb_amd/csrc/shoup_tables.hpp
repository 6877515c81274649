// The Shoup companions of the NTT's constant multiplicands (shoup_core29, field.hpp), as ntt.hip builds them: host and device code,
// so that tools/shoup_tables.hip can hold the same functions to Python's integers on a machine without a GPU.
#pragma once
#include <vector>

#include "limb9.hpp"

namespace vdb {

// (w, w') of a constant given in Montgomery form: w = its canonical residue
inline void shoup_const_of_mont(const u256& mont, uint32_t out[18]) { shoup_pair29(from_mont<Fr>(mont), out); }

// the stage table of one pass (NttPass::sh_tab, sh2_tab): entry j, for e = j << res_log, is (w, w') of omega_m^e = omega^(e n / m),
// 18 words; omega in Montgomery form
inline std::vector<uint32_t> shoup_stage_entries(uint32_t log_n, const u256& omega, uint32_t S, uint32_t res_log) {
  const uint32_t m = 1u << S, ns = (m / 2) >> res_log;
  std::vector<uint32_t> tab((size_t)ns * 18);
  const u256 step = mont_pow<Fr>(omega, u256_from_u64(((uint64_t)1 << (log_n - S)) << res_log));  // omega_m^(2^res_log)
  u256 cur = mont_one<Fr>();
  for (uint32_t j = 0; j < ns; j++) {
    shoup_const_of_mont(cur, &tab[18 * (size_t)j]);
    cur = fr_mul(cur, step);
  }
  return tab;
}

// one record of the inter-pass table (NttPass::tw_rec) from the twiddle-table entry t = 32 c (Montgomery form; c = omega^e, or
// omega^e / n in the table of an inverse transform's first pass): (c, c') and two zero words, 20 words = five 16-byte loads.
// inv32: 1/32 in Montgomery form
HD void shoup_record_of_tw(const u256& t, const u256& inv32, uint32_t out[20]) {
  shoup_pair29(from_mont<Fr>(fr_mul(t, inv32)), out);
  out[18] = out[19] = 0;
}

}  // namespace vdb
