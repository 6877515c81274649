// Stand-alone check of the host-side arithmetic of the routing audit (halo2_vectordb_amd/csrc/ann_update_host.hpp anna_blocks over ann_head and
// ann_cluster): the first
// cell of every block, the per-member strides and the totals against a brute-force count that appends the circuit's gadgets one after
// the other.  No device call: build it with the host sanitizers and run it on the CPU,
//   clang++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I halo2_vectordb_amd/csrc tools/ann_audit_host_check.cpp -o ann_audit_host_check && ./ann_audit_host_check
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

int main() {
  std::mt19937_64 rng(11);
  for (int it = 0; it < 20000; it++) {
    const uint64_t K = it < 64 ? 1 + it % 8 : 1 + rng() % 70, n_c = 1 + rng() % 40, dim = 1 + rng() % 9;
    const uint64_t sponge = 1 + rng() % 5000, dist = 8 + rng() % 3000, dist_l = rng() % 200, qmin = 1 + rng() % 300, qmin_l = rng() % 40;
    const uint64_t mc = 1 + rng() % 100000, mm = 1 + rng() % 100000;
    const AnnaBlocks b = anna_blocks(K, n_c, dim, sponge, dist, dist_l, qmin, qmin_l, mc, mm);
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
    CHECK(f.b_own == at);
    std::vector<uint64_t> first(n_c), first_l(n_c);
    for (uint64_t i = 0; i < n_c; i++) {            // R
      first[i] = at, first_l[i] = lk;
      CHECK(at == f.b_own + i * b.per_member && lk == i * b.per_member_l);
      for (uint64_t j = 0; j < K; j++) at += dist, lk += dist_l;
      CHECK(at - first[i] == b.chain_off && lk - first_l[i] == b.chain_loff);
      for (uint64_t j = 1; j < K; j++) at += qmin, lk += qmin_l;
      CHECK(at - first[i] == b.pick_off);
      at += 1 + 3 * K;
    }
    CHECK(f.b_mc == at);
    at += mc;                                       // MC
    CHECK(f.b_mm == at);
    at += mm;                                       // MM
    CHECK(f.total == at && b.total_l == lk);
    // the head is the frame's: the same first cells as annu_blocks gives the update and the delete
    const AnnuBlocks u = annu_blocks(K, sponge, 0);
    CHECK(u.h.n_in == h.n_in && u.h.b_ind == h.b_ind && u.h.b_sel == h.b_sel && u.h.b_old == h.b_old && u.b_upd == f.b_in);
  }
  // the head alone, against its closed forms
  for (uint64_t K = 1; K <= 70; K++) {
    const uint64_t sponge = 1 + 37 * K;
    const AnnHead h = ann_head(K, sponge);
    CHECK(h.n_in == K + 2 && h.b_ind == h.n_in && h.b_sel == h.b_ind + 8 + 12 * (K - 1) && h.b_old == h.b_sel + 1 + 3 * K && h.end == h.b_old + sponge);
  }
  // K = 1: no chain, the pick follows the one distance
  {
    const AnnaBlocks b = anna_blocks(1, 3, 4, 10, 100, 7, 50, 5, 20, 30);
    CHECK(b.chain_off == 100 && b.pick_off == 100 && b.per_member == 104 && b.per_member_l == 7 && b.total_l == 21);
  }
  std::puts("ann_audit_host_check: ok");
  return 0;
}
