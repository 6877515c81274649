// Stand-alone check of the host-side arithmetic of the cover (halo2_vectordb_amd/csrc/ann_update_host.hpp annc_blocks): the first cell of
// every block and the total against a brute-force count that appends the circuit's gadgets one after the other, over random (K, sizes),
// and its refusals.  No device call: build it with the host sanitizers and run it on the CPU,
//   clang++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I halo2_vectordb_amd/csrc tools/ann_cover_host_check.cpp -o ann_cover_host_check && ./ann_cover_host_check
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "ann_update_host.hpp"

using namespace vdb;

#define CHECK(x)                                                     \
  do {                                                               \
    if (!(x)) {                                                      \
      std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #x);   \
      std::exit(1);                                                  \
    }                                                                \
  } while (0)

// the nodes of the tree over m leaves, level by level, and whether its padding reads the zero cell
static uint64_t tree_nodes(uint64_t m, bool* padded) {
  uint64_t lp = 1;
  while (lp < m) lp *= 2;
  *padded = lp > m;
  uint64_t nodes = 0;
  for (uint64_t w = lp; w > 1; w /= 2) nodes += w / 2;
  return nodes;
}

int main() {
  std::mt19937_64 rng(23);
  const uint64_t max_n = (uint64_t)1 << 24;
  for (int it = 0; it < 20000; it++) {
    const uint64_t K = it < 32 ? 1 + it % 4 : 1 + rng() % 70;
    std::vector<uint64_t> sizes(K);
    for (auto& s : sizes) s = it < 32 ? 1 + (it / 4 + rng() % 3) % 9 : (rng() % 5 ? 1 + rng() % 40 : (uint64_t)1 << (rng() % 8));
    const uint64_t sponge = 1 + rng() % 9000, node = 1 + rng() % 9000;
    AnncBlocks b;
    CHECK(annc_blocks(sizes.data(), K, max_n, sponge, node, &b) == 0);
    uint64_t n = 0;
    for (uint64_t s : sizes) n += s;
    CHECK(b.n == n);
    // the stream, gadget by gadget
    uint64_t at = 0;
    at += K + 1;                                        // A
    CHECK(b.b_a == at);
    for (uint64_t i = 0; i < n; i++) at += 1;           // I: a
    CHECK(b.b_b == at);
    for (uint64_t i = 0; i < n; i++) at += 1;           // I: b
    CHECK(b.n_in == at && b.b_z == at);
    bool pad_d, any_pad;
    const uint64_t nodes_d = tree_nodes(n, &pad_d);
    any_pad = pad_d;
    std::vector<uint64_t> nodes_c(K);
    for (uint64_t c = 0; c < K; c++) {
      bool p;
      nodes_c[c] = tree_nodes(sizes[c], &p);
      any_pad = any_pad || p;
      CHECK(sizes[c] > 1 || nodes_c[c] == 0);           // a cluster of one member has no node
    }
    if (any_pad) at += 1;                               // Z: load_zero caches, one cell for all trees
    CHECK(b.zero == (any_pad ? 1u : 0u) && b.b_td == at);
    for (uint64_t g = 0; g < nodes_d; g++) at += node;  // TD
    CHECK(b.b_tc == at && b.lp == nodes_d + 1);
    uint64_t total_c = 0;
    for (uint64_t c = 0; c < K; c++) {                  // TC
      CHECK(at == b.b_tc + total_c * node);
      for (uint64_t g = 0; g < nodes_c[c]; g++) at += node;
      total_c += nodes_c[c];
    }
    CHECK(b.nodes_c == total_c && b.b_d == at);
    at += sponge;                                       // D
    CHECK(b.b_g == at);
    at += node;                                         // G: two words, a node's cells
    for (int side = 0; side < 2; side++) {
      CHECK((side ? b.b_sb : b.b_sa) == at);
      for (uint64_t i = 0; i < n; i++) at += 4;         // g_sub(gamma, x_i)
      CHECK((side ? b.b_mb : b.b_ma) == at);
      for (uint64_t i = 1; i < n; i++) {                // g_mul(acc, t_i)
        CHECK(at == (side ? b.b_mb : b.b_ma) + 4 * (i - 1));
        at += 4;
      }
    }
    CHECK(b.total == at);
  }
  // n = 1: no node, no zero cell, one factor a side and no product cell
  {
    const uint64_t one = 1;
    AnncBlocks b;
    CHECK(annc_blocks(&one, 1, max_n, 100, 10, &b) == 0);
    CHECK(b.zero == 0 && b.b_td == 4 && b.b_tc == 4 && b.b_d == 4 && b.b_g == 104 && b.b_sa == 114 && b.b_ma == 118 && b.b_sb == 118 && b.b_mb == 122 &&
          b.total == 122);
  }
  // the refusals: K = 0, an empty cluster, n above the limit (without overflow of the sum)
  {
    AnncBlocks b;
    const uint64_t empty[3] = {2, 0, 1}, big[2] = {max_n, 1}, huge[2] = {~0ull, ~0ull}, fits[2] = {max_n - 1, 1};
    CHECK(annc_blocks(empty, 0, max_n, 1, 1, &b) == 1);
    CHECK(annc_blocks(empty, 3, max_n, 1, 1, &b) == 1);
    CHECK(annc_blocks(big, 2, max_n, 1, 1, &b) == 2);
    CHECK(annc_blocks(huge, 2, max_n, 1, 1, &b) == 2);
    CHECK(annc_blocks(fits, 2, max_n, 1, 1, &b) == 0 && b.n == max_n && b.zero == 1);
  }
  std::puts("ann_cover_host_check: ok");
  return 0;
}
