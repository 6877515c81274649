// Stand-alone check of the host-side arithmetic of the recentre (halo2_vectordb_amd/csrc/ann_update_host.hpp annr_blocks over ann_head):
// the first cell of every block and the totals against a brute-force count that appends the circuit's gadgets one after the other.
// No device call: build it with the host sanitizers and run it on the CPU,
//   clang++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I halo2_vectordb_amd/csrc tools/ann_recentre_host_check.cpp -o ann_recentre_host_check && ./ann_recentre_host_check
#include <cstdio>
#include <cstdlib>
#include <random>

#include "ann_update_host.hpp"

using namespace vdb;

#define CHECK(x)                                                     \
  do {                                                               \
    if (!(x)) {                                                      \
      std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #x);   \
      std::exit(1);                                                  \
    }                                                                \
  } while (0)

int main() {
  std::mt19937_64 rng(17);
  for (int it = 0; it < 20000; it++) {
    const uint64_t K = it < 64 ? 2 + it % 8 : 2 + rng() % 70, n_c = it < 64 ? 1 + it / 8 : 1 + rng() % 40, dim = 1 + rng() % 9;
    const uint64_t sponge = 1 + rng() % 5000, qdiv = 8 + rng() % 3000, qdiv_l = rng() % 200;
    const uint64_t mm = 1 + rng() % 100000, leaf = 1 + rng() % 9000, level = 1 + rng() % 9000;
    // the update block of the centroids' tree with one write: [new vector dim | old leaf | bits depth | siblings depth], the leaf sponge,
    // depth levels, the index inner product 1 + 3 (depth - 1)
    uint64_t lp;
    uint32_t depth;
    tree_shape(K, &lp, &depth);
    CHECK(depth >= 1 && lp >= K && lp < 2 * K);
    uint64_t upd = dim + 1 + 2 * depth + leaf;
    for (uint32_t l = 0; l < depth; l++) upd += level;
    upd += 1;
    for (uint32_t l = 1; l < depth; l++) upd += 3;
    const AnnrBlocks b = annr_blocks(K, n_c, dim, sponge, qdiv, qdiv_l, mm, upd);
    const AnnHead& h = b.h;
    // the stream, gadget by gadget: a cursor over the cells and one over the lookup cells
    uint64_t at = 0, lk = 0;
    at += K + 2;                                    // A
    CHECK(h.n_in == at && h.b_ind == at);
    for (uint64_t j = 0; j < K; j++) {              // B
      CHECK(h.b_ind + annu_indicator_off(j) == at);
      at += j ? 12 : 8;
    }
    CHECK(h.b_sel == at);
    at += 1;                                        // C
    for (uint64_t j = 0; j < K; j++) at += 3;
    CHECK(h.b_old == at);
    at += sponge;                                   // D
    CHECK(h.end == at && b.b_in == at);
    for (uint64_t r = 0; r < n_c; r++) at += dim;   // I: the members alone, no centroid
    CHECK(b.b_m == at);
    at += 1;                                        // M: load_constant(quantization(n_c))
    CHECK(b.b_chain == at);
    for (uint64_t i = 1; i < n_c; i++)              // the qadd chain, member-major
      for (uint64_t j = 0; j < dim; j++) {
        CHECK(at == b.b_chain + 4 * ((i - 1) * dim + j));
        at += 4;
      }
    CHECK(b.b_div == at);
    for (uint64_t j = 0; j < dim; j++) {            // one qdiv per word
      CHECK(at == b.b_div + j * qdiv && lk == j * qdiv_l);
      at += qdiv, lk += qdiv_l;
    }
    CHECK(b.b_mm == at);
    at += mm;                                       // MM
    CHECK(b.b_upd == at);
    at += upd;                                      // U
    CHECK(b.b_root == at);
    at += sponge;                                   // G: no select in front of it
    CHECK(b.total == at && b.total_l == lk);
    // the head is the frame's, and block M is the mean audit's with the K centroids and block S taken out from in front of it
    const AnnuBlocks u = annu_blocks(K, sponge, 0);
    CHECK(u.h.n_in == h.n_in && u.h.b_ind == h.b_ind && u.h.b_sel == h.b_sel && u.h.b_old == h.b_old && u.b_upd == b.b_in);
    const AnnmBlocks a = annm_blocks(K, n_c, dim, sponge, qdiv, qdiv_l, 1, mm);
    const uint64_t shift = K * dim + dim * (1 + 3 * K);
    CHECK(a.b_m == b.b_m + shift && a.b_chain == b.b_chain + shift && a.b_div == b.b_div + shift && a.f.b_mc == b.b_mm + shift && a.total_l == b.total_l);
    // against the update's frame around the same block: the recentre has I, M and MM in front of it and no block F behind it
    const AnnuBlocks w = annu_blocks(K, sponge, upd);
    CHECK(w.b_upd == h.end && b.b_upd == w.b_upd + n_c * dim + 1 + (n_c - 1) * dim * 4 + dim * qdiv + mm);
    CHECK(w.b_root - w.b_new == 8 * K && b.total - b.b_root == w.total - w.b_root && b.total + 8 * K == w.total + (b.b_upd - w.b_upd));
  }
  // n_c = 1: no chain, the quotients follow the constant
  {
    const AnnrBlocks b = annr_blocks(2, 1, 3, 10, 100, 7, 30, 50);
    CHECK(b.b_chain == b.b_div && b.b_div == b.b_m + 1 && b.b_mm == b.b_div + 300 && b.b_upd == b.b_mm + 30 && b.b_root == b.b_upd + 50 && b.total_l == 21);
    CHECK(b.total == b.b_root + 10);
  }
  std::puts("ann_recentre_host_check: ok");
  return 0;
}
