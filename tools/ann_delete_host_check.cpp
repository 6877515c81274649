// Stand-alone check of the host-side arithmetic of the index delete (halo2_vectordb_amd/csrc/ann_update_host.hpp): the expansion of m
// deletes to 2 m path updates, the origin tracking behind the carried leaves and the move table, the halvings s, the blocks' first cells,
// the offsets of the index after the batch and every refusal code, each against a brute-force simulation on a plain list.  No device
// call: build it with the host sanitizers and run it on the CPU,
//   clang++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I halo2_vectordb_amd/csrc tools/ann_delete_host_check.cpp -o ann_delete_host_check && ./ann_delete_host_check
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

static uint64_t pow2_at_least(uint64_t n) {
  uint64_t p = 1;
  while (p < n) p *= 2;
  return p;
}

int main() {
  std::mt19937_64 rng(11);
  for (int it = 0; it < 40000; it++) {
    const uint64_t n_c = 1 + rng() % 20;
    const size_t m = rng() % 8, max_updates = it % 7 == 0 ? 8 : 4096;
    std::vector<uint64_t> slots(m + 1);
    // mostly legal slots (below the fill at their turn), sometimes one at or above it
    for (size_t j = 0; j < m; j++) slots[j] = rng() % ((n_c > j ? n_c - j : 1) + (rng() % 8 == 0 ? 2 : 0));
    // brute force: the members as a list of original slots
    int want = 0;
    size_t want_bad = 0;
    std::vector<uint64_t> members(n_c), idx, src;
    for (uint64_t i = 0; i < n_c; i++) members[i] = i;
    if (m == 0 || 2 * m > max_updates) want = 1;
    else if (m >= n_c) want = 2;
    for (size_t j = 0; j < m && !want; j++) {
      if (slots[j] >= members.size()) {
        want = 3, want_bad = j;
        break;
      }
      idx.push_back(slots[j]);
      idx.push_back(members.size() - 1);
      src.push_back(members.back());
      members[slots[j]] = members.back();
      members.pop_back();
    }
    AnndPlan p;
    size_t bad = ~(size_t)0;
    const int got = annd_expand(slots.data(), m, n_c, max_updates, &p, &bad);
    CHECK(got == want);
    if (want == 3) CHECK(bad == want_bad);
    if (want) continue;
    CHECK(p.indices.size() == 2 * m && p.kinds.size() == 2 * m && p.carry_src.size() == 2 * m);
    for (size_t j = 0; j < m; j++) {
      CHECK(p.indices[2 * j] == idx[2 * j] && p.indices[2 * j + 1] == idx[2 * j + 1] && p.indices[2 * j + 1] == n_c - 1 - j);
      CHECK(p.kinds[2 * j] == 2 && p.kinds[2 * j + 1] == 1 && p.carry_src[2 * j] == src[j] && p.carry_src[2 * j] < n_c);
    }
    CHECK(p.lp == pow2_at_least(n_c) && p.lp_new == pow2_at_least(n_c - m) && (p.lp >> p.shrink) == p.lp_new && ((uint64_t)1 << p.depth) == p.lp);
    CHECK(p.shrink <= p.depth && members.size() == n_c - m);
    // the move table: exactly the surviving positions whose member is not the original one, each once
    std::vector<uint64_t> after(n_c - m);
    for (uint64_t i = 0; i < n_c - m; i++) after[i] = i;
    CHECK(p.move_pos.size() == p.move_src.size() && p.move_pos.size() <= m);
    std::vector<char> seen(n_c, 0);
    for (size_t i = 0; i < p.move_pos.size(); i++) {
      CHECK(p.move_pos[i] < n_c - m && p.move_src[i] < n_c && !seen[p.move_pos[i]] && p.move_src[i] != p.move_pos[i]);
      seen[p.move_pos[i]] = 1;
      after[p.move_pos[i]] = p.move_src[i];
    }
    CHECK(after == members);
    // the blocks
    const uint64_t K = 1 + rng() % 5, sc = annd_shrink_cells(p.depth, p.shrink, 4506);
    CHECK(sc == (p.shrink ? 2 + (uint64_t)(p.depth - 1 + p.shrink) * 4506 : 0));
    const AnnuBlocks b = annu_blocks(K, 1000, 77, sc);
    const AnnuBlocks u = annu_blocks(K, 1000, 77);
    CHECK(b.b_upd == u.b_upd && b.b_shr == u.b_upd + 77 && b.b_new == b.b_shr + sc && b.total == u.total + sc && b.b_root - b.b_new == 8 * K);
    // the index after the batch
    const size_t c = rng() % K;
    std::vector<uint64_t> sizes(K);
    for (auto& s : sizes) s = 1 + rng() % 9;
    sizes[c] = n_c;
    AnndRemovePlan r;
    CHECK(annd_remove_plan(sizes.data(), K, c, m, p.lp, p.lp_new, &r) == 0);
    uint64_t rows = 0, dig = 0, dig_old = 0;
    for (size_t s = 0; s <= K; s++) {
      CHECK(r.seg_off[s] == dig);
      if (s < K) CHECK(r.offsets[s] == rows);
      const uint64_t old_sz = s < K ? sizes[s] : K, sz = old_sz - (s == c ? m : 0);
      if (s == c) CHECK(r.off_c == rows && r.keep_c == n_c - m);
      if (s < K) rows += sz;
      dig += 2 * pow2_at_least(sz);
      dig_old += 2 * pow2_at_least(old_sz);
    }
    CHECK(r.offsets[K] == rows && r.n_new == rows && r.seg_off[K + 1] == dig && r.delta == dig_old - dig);
  }
  {
    AnndRemovePlan r;
    const uint64_t sizes[3] = {3, 0, 3};
    CHECK(annd_remove_plan(sizes, 3, 0, 1, 4, 2, &r) == 1);    // an empty cluster
    // the issue's shapes: 5 -> 4 halves once, 5 -> 2 twice, 4 -> 3 not at all, 2 -> 1 leaves one leaf
    AnndPlan p;
    const uint64_t one[1] = {1}, three[3] = {4, 0, 0}, zero[1] = {0};
    CHECK(annd_expand(one, 1, 5, 4096, &p, nullptr) == 0 && p.shrink == 1 && p.carry_src[0] == 4 && p.move_pos.size() == 1);
    CHECK(annd_expand(three, 3, 5, 4096, &p, nullptr) == 0 && p.shrink == 2 && p.carry_src[0] == 4 && p.carry_src[2] == 3 && p.carry_src[4] == 2);
    CHECK(p.move_pos.size() == 1 && p.move_pos[0] == 0 && p.move_src[0] == 2);
    CHECK(annd_expand(one, 1, 4, 4096, &p, nullptr) == 0 && p.shrink == 0);
    CHECK(annd_expand(zero, 1, 2, 4096, &p, nullptr) == 0 && p.shrink == 1 && p.lp_new == 1 && p.depth == 1);
  }
  std::puts("ann_delete_host_check: ok");
  return 0;
}
