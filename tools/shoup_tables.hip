// Host check of the NTT's Shoup companions (halo2_vectordb_amd/csrc/shoup_tables.hpp) against Python integers
// (tests/test_shoup_tables_cpu.py): hipcc -O2 -std=c++17 --offload-arch=gfx950 -o shoup_tables tools/shoup_tables.hip
// stdin: lines "k omega zeta" (canonical hex; omega a primitive 2^k-th root of unity).  For every k, stdout lines
//   "st k S rl j w q"   stage tables (NttPass::sh_tab, sh2_tab) of the pass sizes S <= min(k, 9), every resolution rl <= 2
//   "ip k f e w q"      inter-pass records (NttPass::tw_rec) of the table entries e (f = 1: the 1/n-scaled table), a sample of e
//   "c k i w q"         kernel-argument constants: 1, zeta, zeta^2 (NttPass::zsh), i = 0, 1, 2
// all numbers hex; w, q are the limbs read back as integers (w must be canonical, q = floor(w 2^261 / r)).
#include <cstdio>
#include <cstdint>
#include "../halo2_vectordb_amd/csrc/shoup_tables.hpp"
using namespace vdb;

static u256 from_hex(const char* s) {
  u256 v = u256_zero();
  for (; *s; s++) {
    const char c = *s;
    const uint32_t d = c <= '9' ? c - '0' : (c | 32) - 'a' + 10;
    for (int i = 7; i > 0; i--) v.w[i] = (v.w[i] << 4) | (v.w[i - 1] >> 28);
    v.w[0] = (v.w[0] << 4) | d;
  }
  return v;
}
// nine 29-bit limbs -> hex (the value may exceed 256 bits: w' < 2^261)
static void pr9(const uint32_t* l) {
  uint32_t w[9] = {0};
  for (int k = 0; k < 9; k++)
    for (int b = 0; b < 29; b++)
      if ((l[k] >> b) & 1) w[(29 * k + b) >> 5] |= 1u << ((29 * k + b) & 31);
  printf(" %x", w[8]);
  for (int i = 7; i >= 0; i--) printf("%08x", w[i]);
}
int main() {
  char hw[80], hz[80];
  unsigned k;
  const u256 r2 = mont_r2<Fr>();
  while (scanf("%u %79s %79s", &k, hw, hz) == 3) {
    const u256 omega = mont_mul<Fr>(from_hex(hw), r2), zeta = mont_mul<Fr>(from_hex(hz), r2);
    for (uint32_t S = 1; S <= (k < 9 ? k : 9); S++)
      for (uint32_t rl = 0; rl <= 2 && rl < S; rl++) {
        const std::vector<uint32_t> tab = shoup_stage_entries(k, omega, S, rl);
        for (size_t j = 0; j < tab.size() / 18; j++) {
          printf("st %x %x %x %zx", k, S, rl, j);
          pr9(&tab[18 * j]);
          pr9(&tab[18 * j + 9]);
          printf("\n");
        }
      }
    // inter-pass tables as get_twiddles fills them (k_twiddles: entry e = omega^e * factor), factor 32 or 32 / n
    const uint64_t n = 1ull << k;
    const u256 m32 = mont_mul<Fr>(u256_from_u64(32), r2);
    const u256 inv32 = mont_inv<Fr>(m32);
    const u256 fin = fr_mul(mont_inv<Fr>(mont_mul<Fr>(u256_from_u64(n), r2)), m32);
    for (int f = 0; f < 2; f++)
      for (uint64_t i = 0; i < 48; i++) {
        const uint64_t e = i < 16 ? i % n : (i < 32 ? (n - 1 - (i - 16)) % n : (i * 0x9E3779B97F4Aull) % n);
        const u256 t = fr_mul(mont_pow<Fr>(omega, u256_from_u64(e)), f ? fin : m32);
        uint32_t o[20];
        shoup_record_of_tw(t, inv32, o);
        printf("ip %x %x %llx", k, f, (unsigned long long)e);
        pr9(o);
        pr9(o + 9);
        printf(" %x %x\n", o[18], o[19]);
      }
    const u256 cs[3] = {mont_one<Fr>(), zeta, fr_mul(zeta, zeta)};
    for (int i = 0; i < 3; i++) {
      uint32_t o[18];
      shoup_const_of_mont(cs[i], o);
      printf("c %x %x", k, i);
      pr9(o);
      pr9(o + 9);
      printf("\n");
    }
  }
  return 0;
}
