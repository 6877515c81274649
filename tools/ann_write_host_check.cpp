// Stand-alone check of the host-side arithmetic of the linked write (halo2_vectordb_amd/csrc/ann_update_host.hpp): the database slot of
// every write of a batch into one cluster (a replacement's from the cluster's recorded slots, an append's from the database's fill, a
// write to a member the batch itself appended from the batch), the number of appends, the smallest growth of the database tree, the
// blocks' first cells and every refusal code, each against a brute-force simulation on two plain lists.  No device call: build it with
// the host sanitizers and run it on the CPU,
//   clang++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I halo2_vectordb_amd/csrc tools/ann_write_host_check.cpp -o ann_write_host_check && ./ann_write_host_check
#include <algorithm>
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
static unsigned log2_of(uint64_t p) {
  unsigned d = 0;
  while (((uint64_t)1 << d) < p) d++;
  return d;
}

int main() {
  std::mt19937_64 rng(17);
  for (int it = 0; it < 40000; it++) {
    const uint64_t n = rng() % 24 == 0 ? 0 : 1 + rng() % 40;
    const uint64_t n_c = rng() % 24 == 0 ? n + 1 + rng() % 3 : (n ? 1 + rng() % n : 0);
    const size_t m = 1 + rng() % 8;
    // the cluster's members hold distinct database slots; now and then one lies outside the database
    std::vector<uint64_t> all(std::max<uint64_t>(n, n_c)), slots;
    for (uint64_t i = 0; i < all.size(); i++) all[i] = i;
    std::shuffle(all.begin(), all.end(), rng);
    slots.assign(all.begin(), all.begin() + n_c);
    const bool known = rng() % 3 != 0;   // does the caller know the cluster's slots?
    size_t broken = ~(size_t)0;
    if (known && n_c && n_c <= n && rng() % 16 == 0) {
      broken = rng() % n_c;
      slots[broken] = n + rng() % 3;
    }
    std::vector<uint64_t> idx(m);
    uint64_t f = n_c;
    for (size_t j = 0; j < m; j++) {
      idx[j] = rng() % 12 == 0 ? f + 1 + rng() % 2 : rng() % 2 ? f : rng() % (f + 1);
      f += idx[j] == f;
    }
    // brute force: two lists, the cluster's members as database slots and the database as a row count, one write after the other
    int want = 0;
    size_t want_bad = 0;
    std::vector<uint64_t> members = slots, db_idx;
    uint64_t rows = n, appends = 0;
    if (n == 0 || n_c > n) want = 2;
    if (!want && known)
      for (uint64_t i = 0; i < n_c && !want; i++)
        if (slots[i] >= n) want = 3, want_bad = i;
    for (size_t j = 0; j < m && !want; j++) {
      if (idx[j] > members.size()) {
        want = 1, want_bad = j;
        break;
      }
      if (idx[j] == members.size()) members.push_back(rows++), appends++;
      db_idx.push_back(members[idx[j]]);
    }
    // what the caller passes as its own: the truth, or one entry off.  Where the expansion knows the entry (the slots are given, an append,
    // a member the batch appended) any other value is refused; an old member's entry under unknown slots only outside the database
    std::vector<uint64_t> given = db_idx;
    given.resize(m, 0);
    const bool pass_given = !known || rng() % 2;
    if (!want && pass_given && rng() % 4 == 0) {
      const size_t at = rng() % m;
      uint64_t so_far = 0, fill = n_c;
      for (size_t j = 0; j < at; j++)
        if (idx[j] == fill) so_far++, fill++;
      const bool exact = known || idx[at] >= n_c;
      given[at] = exact ? given[at] + 1 : n + so_far + rng() % 2;
      want = 4, want_bad = at;
    }
    unsigned g = 0;
    if (!want)
      while ((pow2_at_least(n) << g) < n + appends) g++;
    const int grow = rng() % 4 == 0 ? (int)(g + 1 - 2 * (rng() % 2)) : rng() % 2 ? (int)g : -1;
    if (!want && grow >= 0 && (unsigned)grow != g) want = 5;
    AnnwPlan p;
    size_t bad = ~(size_t)0;
    const int got = annw_expand(known ? slots.data() : nullptr, idx.data(), m, n_c, n, pass_given ? given.data() : nullptr, grow, &p, &bad);
    CHECK(got == want);
    if (want == 1 || want == 3 || want == 4) CHECK(bad == want_bad);
    if (want) continue;
    CHECK(p.appends == appends && p.grow_db == g && p.lp_db == pow2_at_least(n) && p.glp_db == pow2_at_least(n + appends));
    CHECK((p.lp_db << g) == p.glp_db && p.depth_db == log2_of(p.glp_db) && p.db_idx.size() == m);
    uint64_t track = 0;
    CHECK(annu_track_fill(idx.data(), m, n_c, pow2_at_least(n_c + appends), &track, nullptr) == 0 && track == appends);
    for (size_t j = 0; j < m; j++) CHECK(p.db_idx[j] == db_idx[j] && p.db_idx[j] < p.glp_db && p.db_idx[j] < n + appends);
    // the database after the batch is dense: the members' slots are distinct, the appended ones n .. n + appends - 1 in order
    if (broken == ~(size_t)0) {
      std::vector<char> seen(n + appends, 0);
      for (uint64_t x : members) CHECK(x < n + appends && !seen[x]++);
    }
    for (uint64_t i = 0; i < appends; i++) CHECK(members[n_c + i] == n + i);
    // the blocks, gadget by gadget
    const uint64_t K = 1 + rng() % 6, sp = 900 + rng() % 9, ue = 77 + rng() % 9, udb = 55 + rng() % 9;
    const AnnwBlocks B = annw_blocks(K, m, sp, ue, udb);
    uint64_t at = 0;
    at += K + 2;                          // A: c, the centroids' root, K cluster roots
    CHECK(B.u.h.n_in == at && B.u.h.b_ind == at);
    at += 8;                              // B: is_zero(c)
    for (uint64_t j = 1; j < K; j++) {
      CHECK(B.u.h.b_ind + annu_indicator_off(j) == at);
      at += 12;                           // is_equal(c, j)
    }
    CHECK(B.u.h.b_sel == at);
    at += 1 + 3 * K;                      // C: select_by_indicator
    CHECK(B.u.h.b_old == at);
    at += sp;                             // D
    CHECK(B.u.h.end == at && B.u.b_upd == at);
    at += ue;                             // E
    CHECK(B.b_upd_db == at);
    at += udb;                            // E_db
    CHECK(B.u.b_new == at);
    at += 8 * K;                          // F: K selects
    CHECK(B.u.b_root == at);
    at += sp;                             // G
    CHECK(B.u.total == at && B.n_pub == 4 * m + 5);
    // A - E lie where the plain update has them, F and G udb cells later
    const AnnuBlocks U = annu_blocks(K, sp, ue);
    CHECK(U.b_upd == B.u.b_upd && U.b_new + udb == B.u.b_new && U.total + udb == B.u.total);
  }
  {
    // the issue's shapes
    AnnwPlan p;
    const uint64_t s32[3] = {4, 0, 2}, s22[2] = {3, 1}, one[1] = {1}, two[1] = {2}, app_rep[3] = {2, 2, 0}, twice[2] = {1, 1};
    // sizes (3, 2), one replacement: no growth; its database slot is not its cluster slot
    CHECK(annw_expand(s32, one, 1, 3, 5, nullptr, -1, &p, nullptr) == 0 && p.appends == 0 && p.grow_db == 0 && p.db_idx[0] == 0 && p.depth_db == 3);
    // sizes (2, 2), one append into cluster 0: the database doubles (4 -> 5)
    CHECK(annw_expand(s22, two, 1, 2, 4, nullptr, -1, &p, nullptr) == 0 && p.appends == 1 && p.grow_db == 1 && p.db_idx[0] == 4 && p.glp_db == 8);
    // an append, then a replacement of the member just appended: its slot comes from the batch
    CHECK(annw_expand(s22, app_rep, 3, 2, 4, nullptr, -1, &p, nullptr) == 0 && p.appends == 1 && p.db_idx[0] == 4 && p.db_idx[1] == 4 && p.db_idx[2] == 3);
    // a slot written twice
    CHECK(annw_expand(s22, twice, 2, 2, 4, nullptr, 0, &p, nullptr) == 0 && p.db_idx[0] == 1 && p.db_idx[1] == 1 && p.grow_db == 0);
    // refusals
    size_t bad = 9;
    const uint64_t above[2] = {2, 4}, wrong[1] = {2}, out[1] = {5};
    CHECK(annw_expand(s22, above, 2, 2, 4, nullptr, -1, &p, &bad) == 1 && bad == 1);
    CHECK(annw_expand(s22, one, 1, 2, 0, nullptr, -1, &p, nullptr) == 2 && annw_expand(s22, one, 1, 5, 4, nullptr, -1, &p, nullptr) == 2);
    CHECK(annw_expand(s32, one, 1, 3, 4, nullptr, -1, &p, &bad) == 3 && bad == 0);
    CHECK(annw_expand(s22, one, 1, 2, 4, wrong, -1, &p, &bad) == 4 && bad == 0);           // the recorded slot is 1
    CHECK(annw_expand(nullptr, one, 1, 2, 4, wrong, -1, &p, nullptr) == 0 && p.db_idx[0] == 2);   // unknown slots: inside the database
    CHECK(annw_expand(nullptr, one, 1, 2, 4, out, -1, &p, &bad) == 4 && bad == 0);
    CHECK(annw_expand(nullptr, one, 1, 2, 4, nullptr, -1, &p, &bad) == 4);
    CHECK(annw_expand(nullptr, two, 1, 2, 4, out, -1, &p, &bad) == 4 && bad == 0);         // an append goes to the fill: 4
    CHECK(annw_expand(s22, two, 1, 2, 4, nullptr, 0, &p, nullptr) == 5 && annw_expand(s22, two, 1, 2, 4, nullptr, 2, &p, nullptr) == 5);
    // a batch beyond one workgroup: 67 appends to a database of 100
    std::vector<uint64_t> many(67), sl(3);
    for (size_t j = 0; j < 67; j++) many[j] = 3 + j;
    sl[0] = 7, sl[1] = 99, sl[2] = 0;
    CHECK(annw_expand(sl.data(), many.data(), 67, 3, 100, nullptr, -1, &p, nullptr) == 0 && p.appends == 67 && p.grow_db == 1 && p.db_idx[66] == 166);
  }
  std::puts("ann_write_host_check: ok");
  return 0;
}
