// Stand-alone check of the host-side arithmetic of the index move (halo2_vectordb_amd/csrc/ann_update_host.hpp): the expansion of m moves
// to 2 m path updates of the source and m appends to the destination, origin tracking across the two trees (which slot of a held, before
// the batch, what every surviving position of a and every new position of b holds after it), s and g, the blocks' first cells, the row
// and segment maps of the index after the batch and every refusal code, each against a brute-force simulation on plain lists.  No device
// call: build it with the host sanitizers and run it on the CPU,
//   clang++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I halo2_vectordb_amd/csrc tools/ann_move_host_check.cpp -o ann_move_host_check && ./ann_move_host_check
#include <cstdio>
#include <cstdlib>
#include <random>
#include <utility>

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
static unsigned log2_of(uint64_t p) {
  unsigned d = 0;
  while (((uint64_t)1 << d) < p) d++;
  return d;
}

// the source row of new row r, as k_ann_rows_move finds it from the plan's tables
static uint64_t row_source(const AnnMovePlan& mp, const AnnMoveIndexPlan& p, size_t K, size_t a, size_t b, uint64_t n_b, uint64_t r) {
  size_t lo = 0, hi = K;
  while (hi - lo > 1) {
    const size_t mid = (lo + hi) / 2;
    if (p.offsets[mid] <= r) lo = mid; else hi = mid;
  }
  const uint64_t pos = r - p.offsets[lo];
  uint64_t from = p.offsets_old[lo] + pos;
  if (lo == a) {
    for (size_t i = 0; i < mp.d.move_pos.size(); i++)
      if (mp.d.move_pos[i] == pos) {
        from = p.offsets_old[a] + mp.d.move_src[i];
        break;
      }
  } else if (lo == b && pos >= n_b) {
    from = p.offsets_old[a] + mp.d.removed_src[pos - n_b];
  }
  return from;
}

int main() {
  std::mt19937_64 rng(13);
  for (int it = 0; it < 40000; it++) {
    const uint64_t n_a = 1 + rng() % 20, n_b = rng() % 16 == 0 ? 0 : 1 + rng() % 20;
    const size_t m = rng() % 8, max_updates = it % 7 == 0 ? 8 : 4096;
    std::vector<uint64_t> slots(m + 1);
    for (size_t j = 0; j < m; j++) slots[j] = rng() % ((n_a > j ? n_a - j : 1) + (rng() % 8 == 0 ? 2 : 0));
    // brute force: a's members as a list of original slots, b's as (from a?, original slot)
    int want = 0;
    size_t want_bad = 0;
    std::vector<uint64_t> mem_a(n_a), removed;
    std::vector<std::pair<int, uint64_t>> mem_b;
    for (uint64_t i = 0; i < n_a; i++) mem_a[i] = i;
    for (uint64_t i = 0; i < n_b; i++) mem_b.push_back({0, i});
    if (m == 0 || 2 * m > max_updates) want = 1;
    else if (m >= n_a) want = 2;
    for (size_t j = 0; j < m && !want; j++) {
      if (slots[j] >= mem_a.size()) {
        want = 3, want_bad = j;
        break;
      }
      removed.push_back(mem_a[slots[j]]);
      mem_b.push_back({1, mem_a[slots[j]]});
      mem_a[slots[j]] = mem_a.back();
      mem_a.pop_back();
    }
    if (!want && n_b == 0) want = 4;
    unsigned g = 0;
    if (!want)
      while ((pow2_at_least(n_b) << g) < n_b + m) g++;
    // a grow that is given and wrong is refused; -1 lets the plan compute it
    const int given = rng() % 4 == 0 ? (int)(g + 1 - 2 * (rng() % 2)) : rng() % 2 ? (int)g : -1;
    if (!want && given >= 0 && (unsigned)given != g) want = 5;
    AnnMovePlan mp;
    size_t bad = ~(size_t)0;
    const int got = annmv_expand(slots.data(), m, n_a, n_b, given, max_updates, &mp, &bad);
    CHECK(got == want);
    if (want == 3) CHECK(bad == want_bad);
    if (want) continue;
    CHECK(mp.grow == g && annmv_grow(n_b, m) == g && mp.lp_b == pow2_at_least(n_b) && mp.glp_b == pow2_at_least(n_b + m) && (mp.lp_b << g) == mp.glp_b);
    CHECK(mp.depth_b == log2_of(mp.glp_b) && mp.depth_b >= 1 && mp.dest.size() == m && mp.kinds.size() == m && mp.d.removed_src.size() == m);
    for (size_t j = 0; j < m; j++) CHECK(mp.dest[j] == n_b + j && mp.dest[j] < mp.glp_b && mp.kinds[j] == 2 && mp.d.removed_src[j] == removed[j] && removed[j] < n_a);
    CHECK(mp.d.indices.size() == 2 * m && (mp.d.lp >> mp.d.shrink) == pow2_at_least(n_a - m) && mp.d.lp_new == pow2_at_least(n_a - m));
    // the multiset of a's original slots is kept: survivors plus arrivals are 0 .. n_a - 1, each once
    std::vector<char> seen(n_a, 0);
    for (uint64_t x : mem_a) CHECK(!seen[x]++);
    for (uint64_t x : removed) CHECK(!seen[x]++);
    // the blocks
    const uint64_t K = 2 + rng() % 5, sc = annd_shrink_cells(mp.d.depth, mp.d.shrink, 4506), ua = 77 + rng() % 9, ub = 55 + rng() % 9, sp = 1000;
    const AnnMoveBlocks B = annmv_blocks(K, sp, ua, sc, ub);
    const uint64_t ind = 8 + 12 * (K - 1), sel = 1 + 3 * K;
    CHECK(B.n_in == K + 3 && B.b_ind_a == K + 3 && B.b_sel_a == B.b_ind_a + ind && B.b_old == B.b_sel_a + sel && B.b_upd_a == B.b_old + sp);
    CHECK(B.b_shr == B.b_upd_a + ua && B.b_mid == B.b_shr + sc && B.b_ind_b == B.b_mid + 8 * K && B.b_sel_b == B.b_ind_b + ind);
    CHECK(B.b_upd_b == B.b_sel_b + sel && B.b_new == B.b_upd_b + ub && B.b_root == B.b_new + 8 * K && B.total == B.b_root + sp);
    // against the delete's and the update's frames: the delete's blocks lie one cell later (the header's second cluster), and the whole is
    // the two circuits' cells less one frame's two sponges and all but one cell of a header
    const AnnuBlocks del = annu_blocks(K, sp, ua, sc), upd = annu_blocks(K, sp, ub);
    CHECK(B.b_upd_a == del.b_upd + 1 && B.b_mid == del.b_new + 1);
    CHECK(B.total == del.total + upd.total + 1 - 2 * sp - (K + 2));
    // the index after the batch
    size_t a = rng() % K, b = rng() % K;
    if (a == b) b = (a + 1) % K;
    std::vector<uint64_t> sizes(K);
    for (auto& s : sizes) s = 1 + rng() % 9;
    sizes[a] = n_a, sizes[b] = n_b;
    AnnMoveIndexPlan p;
    CHECK(annmv_index_plan(sizes.data(), K, a, b, m, mp.d.lp_new, mp.glp_b, &p) == 0);
    // brute force: the old index as rows (cluster, original slot), the new one by lists
    std::vector<std::vector<std::pair<size_t, uint64_t>>> now(K);
    for (size_t s = 0; s < K; s++)
      for (uint64_t i = 0; i < sizes[s]; i++) now[s].push_back({s, i});
    now[a].clear();
    for (uint64_t x : mem_a) now[a].push_back({a, x});
    now[b].clear();
    for (auto& e : mem_b) now[b].push_back({e.first ? a : b, e.second});
    uint64_t rows = 0, rows_old = 0, dig = 0, dig_old = 0;
    for (size_t s = 0; s <= K; s++) {
      CHECK(p.seg_off[s] == dig && p.seg_off_old[s] == dig_old);
      const uint64_t old_sz = s < K ? sizes[s] : K, sz = s < K ? now[s].size() : K;
      if (s < K) {
        CHECK(p.offsets[s] == rows && p.offsets_old[s] == rows_old);
        for (uint64_t i = 0; i < sz; i++) {
          const uint64_t from = row_source(mp, p, K, a, b, n_b, rows + i);
          CHECK(from < p.n && from == p.offsets_old[now[s][i].first] + now[s][i].second);
        }
        rows += sz, rows_old += old_sz;
      }
      dig += 2 * pow2_at_least(sz);
      dig_old += 2 * pow2_at_least(old_sz);
    }
    CHECK(p.offsets[K] == rows && p.n == rows && rows == rows_old && p.seg_off[K + 1] == dig && p.seg_off_old[K + 1] == dig_old);
    CHECK(p.seg_off[a + 1] - p.seg_off[a] == 2 * mp.d.lp_new && p.seg_off[b + 1] - p.seg_off[b] == 2 * mp.glp_b);
    // every source row is read exactly once: the new rows are a permutation of the old ones
    std::vector<char> read(p.n, 0);
    for (uint64_t r = 0; r < p.n; r++) CHECK(!read[row_source(mp, p, K, a, b, n_b, r)]++);
  }
  {
    AnnMoveIndexPlan p;
    const uint64_t sizes[3] = {3, 0, 3};
    CHECK(annmv_index_plan(sizes, 3, 0, 2, 1, 2, 4, &p) == 1);    // an empty cluster
    // the issue's shapes
    AnnMovePlan mp;
    const uint64_t one[1] = {1}, zero[1] = {0}, three[3] = {4, 0, 0}, two[2] = {0, 2};
    CHECK(annmv_expand(one, 1, 5, 4, -1, 4096, &mp, nullptr) == 0 && mp.d.shrink == 1 && mp.grow == 1 && mp.d.removed_src[0] == 1 && mp.depth_b == 3);
    CHECK(annmv_expand(zero, 1, 4, 3, -1, 4096, &mp, nullptr) == 0 && mp.d.shrink == 0 && mp.grow == 0 && mp.depth_b == 2);
    CHECK(annmv_expand(three, 3, 5, 2, -1, 4096, &mp, nullptr) == 0 && mp.d.shrink == 2 && mp.grow == 2);
    CHECK(mp.d.removed_src[0] == 4 && mp.d.removed_src[1] == 0 && mp.d.removed_src[2] == 3);   // slot 0 again takes what the second move put there
    CHECK(annmv_expand(zero, 1, 2, 1, -1, 4096, &mp, nullptr) == 0 && mp.d.shrink == 1 && mp.grow == 1 && mp.d.depth == 1 && mp.depth_b == 1 && mp.lp_b == 1);
    CHECK(annmv_expand(two, 2, 5, 3, -1, 4096, &mp, nullptr) == 0 && mp.d.shrink == 1 && mp.grow == 1 && mp.d.removed_src[1] == 2);
    CHECK(annmv_expand(one, 1, 5, 4, 0, 4096, &mp, nullptr) == 5 && annmv_expand(one, 1, 5, 4, 2, 4096, &mp, nullptr) == 5);
    CHECK(annmv_expand(one, 1, 5, 0, -1, 4096, &mp, nullptr) == 4);
    // the batch beyond one workgroup: 130 -> 63 and 3 -> 70
    std::vector<uint64_t> many(67, 0);
    CHECK(annmv_expand(many.data(), 67, 130, 3, -1, 4096, &mp, nullptr) == 0 && mp.d.shrink == 2 && mp.grow == 5 && mp.d.lp == 256 && mp.glp_b == 128);
  }
  std::puts("ann_move_host_check: ok");
  return 0;
}
