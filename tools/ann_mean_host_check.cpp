// Stand-alone check of the host-side arithmetic of the mean audit (halo2_vectordb_amd/csrc/ann_update_host.hpp annm_blocks over ann_head and
// ann_cluster): the first
// cell of every block and the totals against a brute-force count that appends the circuit's gadgets one after the other.  No device
// call: build it with the host sanitizers and run it on the CPU,
//   clang++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I halo2_vectordb_amd/csrc tools/ann_mean_host_check.cpp -o ann_mean_host_check && ./ann_mean_host_check
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
  std::mt19937_64 rng(13);
  for (int it = 0; it < 20000; it++) {
    const uint64_t K = it < 64 ? 1 + it % 8 : 1 + rng() % 70, n_c = it < 64 ? 1 + it / 8 : 1 + rng() % 40, dim = 1 + rng() % 9;
    const uint64_t sponge = 1 + rng() % 5000, qdiv = 8 + rng() % 3000, qdiv_l = rng() % 200;
    const uint64_t mc = 1 + rng() % 100000, mm = 1 + rng() % 100000;
    const AnnmBlocks b = annm_blocks(K, n_c, dim, sponge, qdiv, qdiv_l, mc, mm);
    const AnnCluster& f = b.f;
    const AnnHead& h = f.h;
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
    CHECK(h.end == at && f.b_in == at);
    for (uint64_t r = 0; r < K + n_c; r++) at += dim;   // I
    CHECK(f.b_own == at && b.b_s == at);
    for (uint64_t j = 0; j < dim; j++) {            // S: select_by_indicator over the K centroids, word by word
      at += 1;
      for (uint64_t k = 0; k < K; k++) at += 3;
    }
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
    CHECK(f.b_mc == at);
    at += mc;                                       // MC
    CHECK(f.b_mm == at);
    at += mm;                                       // MM
    CHECK(f.total == at && b.total_l == lk);
    // the head is the frame's: the same first cells as annu_blocks gives the update and the delete, and as the routing audit has (by construction:
    // all three start from ann_head, the two audits from ann_cluster)
    const AnnuBlocks u = annu_blocks(K, sponge, 0);
    CHECK(u.h.n_in == h.n_in && u.h.b_ind == h.b_ind && u.h.b_sel == h.b_sel && u.h.b_old == h.b_old && u.b_upd == f.b_in);
    const AnnaBlocks a = anna_blocks(K, n_c, dim, sponge, 1, 0, 1, 0, mc, mm);
    CHECK(a.f.b_in == f.b_in && a.f.b_own == b.b_s);
  }
  // the head alone, against its closed forms
  for (uint64_t K = 1; K <= 70; K++) {
    const uint64_t sponge = 1 + 37 * K;
    const AnnHead h = ann_head(K, sponge);
    CHECK(h.n_in == K + 2 && h.b_ind == h.n_in && h.b_sel == h.b_ind + 8 + 12 * (K - 1) && h.b_old == h.b_sel + 1 + 3 * K && h.end == h.b_old + sponge);
  }
  // n_c = 1: no chain, the quotients follow the constant
  {
    const AnnmBlocks b = annm_blocks(2, 1, 3, 10, 100, 7, 20, 30);
    CHECK(b.b_chain == b.b_div && b.b_div == b.b_m + 1 && b.f.b_mc == b.b_div + 300 && b.total_l == 21);
  }
  std::puts("ann_mean_host_check: ok");
  return 0;
}
