// Stand-alone check of the host-side arithmetic of the index update (halo2_vectordb_amd/csrc/ann_update_host.hpp): the blocks' first
// cells, the fill tracking with its refusals, and the offsets of the index after a batch, each against a brute-force count.  No device
// call: build it with the host sanitizers and run it on the CPU,
//   clang++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I halo2_vectordb_amd/csrc tools/ann_update_host_check.cpp -o ann_update_host_check && ./ann_update_host_check
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
  // tree_shape
  for (uint64_t n = 1; n <= 1025; n++) {
    uint64_t lp;
    uint32_t d;
    tree_shape(n, &lp, &d);
    CHECK(lp == pow2_at_least(n) && ((uint64_t)1 << d) == lp);
  }
  // the blocks: sizes add up, the indicator offsets tile block B
  for (uint64_t K : {1ull, 2ull, 3ull, 64ull, 4096ull}) {
    const AnnuBlocks b = annu_blocks(K, 1000, 77);
    CHECK(b.h.n_in == K + 2 && b.h.b_ind == K + 2);
    CHECK(b.h.b_sel - b.h.b_ind == 8 + 12 * (K - 1));
    CHECK(b.h.b_old - b.h.b_sel == 1 + 3 * K && b.b_upd - b.h.b_old == 1000 && b.b_upd == b.h.end && b.b_new - b.b_upd == 77 && b.b_shr == b.b_new);
    CHECK(b.b_root - b.b_new == 8 * K && b.total - b.b_root == 1000);
    uint64_t at = 0;
    for (uint64_t j = 0; j < K; j++) {
      CHECK(annu_indicator_off(j) == at);
      at += j ? 12 : 8;
    }
    CHECK(at == b.h.b_sel - b.h.b_ind);
  }
  // fill tracking against a set of occupied slots
  std::mt19937_64 rng(7);
  for (int it = 0; it < 20000; it++) {
    const uint64_t n_c = 1 + rng() % 9, glp = pow2_at_least(n_c) << (rng() % 3);
    const size_t m = 1 + rng() % 6;
    std::vector<uint64_t> idx(m);
    for (auto& x : idx) x = rng() % (glp + 2);
    std::vector<char> used(glp + 4, 0);
    for (uint64_t i = 0; i < n_c; i++) used[i] = 1;
    int want = 0;
    size_t want_bad = 0;
    uint64_t want_app = 0;
    for (size_t j = 0; j < m && !want; j++) {
      if (idx[j] >= glp) want = 2, want_bad = j;
      else if (!used[idx[j]] && (idx[j] == 0 || !used[idx[j] - 1])) want = 1, want_bad = j;
      else if (!used[idx[j]]) used[idx[j]] = 1, want_app++;
    }
    uint64_t app = ~0ull;
    size_t bad = ~(size_t)0;
    const int got = annu_track_fill(idx.data(), m, n_c, glp, &app, &bad);
    CHECK(got == want);
    if (want) CHECK(bad == want_bad && app == ~0ull);
    else CHECK(app == want_app);
  }
  CHECK(annu_track_fill(nullptr, 0, 3, 4, nullptr, nullptr) == 0);
  // the index after a batch: prefix sums against a recount, the refusals
  for (int it = 0; it < 20000; it++) {
    const size_t K = 1 + rng() % 6, c = rng() % K;
    std::vector<uint64_t> sizes(K);
    for (auto& s : sizes) s = 1 + rng() % 9;
    const uint64_t appends = rng() % 12;
    const unsigned grow = (unsigned)(rng() % 4);
    AnnuApplyPlan p;
    const int rc = annu_apply_plan(sizes.data(), K, c, grow, appends, &p);
    const uint64_t lp_old = pow2_at_least(sizes[c]), lp_new = pow2_at_least(sizes[c] + appends);
    CHECK((rc == 0) == ((lp_old << grow) == lp_new));
    if (rc) {
      CHECK(rc == 2);
      continue;
    }
    uint64_t rows = 0, dig = 0;
    for (size_t s = 0; s <= K; s++) {
      CHECK(p.seg_off[s] == dig);
      if (s < K) CHECK(p.offsets[s] == rows);
      const uint64_t sz = s < K ? sizes[s] + (s == c ? appends : 0) : K;
      if (s == c) CHECK(p.off_c == rows && p.end_c == rows + sizes[c] && p.glp_c == lp_new && p.delta == 2 * (lp_new - lp_old));
      if (s < K) rows += sz;
      dig += 2 * pow2_at_least(sz);
    }
    CHECK(p.offsets[K] == rows && p.seg_off[K + 1] == dig && p.n_new == rows && p.n_old == rows - appends && p.appends == appends);
  }
  {
    AnnuApplyPlan p;
    const uint64_t sizes[3] = {2, 0, 3};
    CHECK(annu_apply_plan(sizes, 3, 0, 0, 0, &p) == 1);    // an empty cluster
    const uint64_t ok[3] = {2, 1, 3};
    CHECK(annu_apply_plan(ok, 3, 0, 63, 0, &p) == 2);       // a shift that would overflow is refused, not evaluated
  }
  std::puts("ann_update_host_check: ok");
  return 0;
}
