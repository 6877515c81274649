// The plan of the batch search (k_ann_search and k_ann_search_merge, witness.hip; include/vdb.h vdb_ann_search_dev and
// vdb_ann_search_probed_dev): everything the driver decides before it touches a pointer — the tile (R queries, chunks of C
// database rows), the span of rows a task walks, the task list, the queries' order in the tiles, the CSR of partial lists the merge
// folds, every query's `last`, the bytes of work space and LDS, and the refusals — in a header with no HIP runtime call and no device
// allocation (the lists are host vectors), as ann_assign_plan.hpp, ntt_plan.hpp and msm_plan.hpp are, so that vdb_ann_search_plan hands
// the very plan the driver launches with to tests/test_ann_search_plan_cpu.py.  The tile's constants are ann_assign_plan.hpp's.
//
// Both forms are one plan over GROUPS: a group is a range [lo, hi) of rows of the vectors array and the (query, base) entries that
// search it.  The dense form is one group, rows [0, n), every query at base 0; the index form is one group per probed cluster, its
// entries the queries that probe it, each at the cluster's offset in that query's candidate list (the probed clusters' members end to
// end in round order).  A group's entries are cut into tiles of R, its range into pieces of `span` rows; a task is (tile, piece).  Since
// the queries of one tile probe their cluster in different rounds, the per-query offset cannot live in the task: the task's idx_base is
// the piece's offset in its group (v_lo - lo), and the CSR entry of a partial list carries the query's base, added by the merge.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "ann_assign_plan.hpp"

namespace vdb {

#define ANN_SEARCH_T_MAX 64
// entries of all the running lists of a tile: R t <= (1,024 / C) C
#define ANN_SEARCH_LIST_WORDS (ANN_ASSIGN_THREADS * ANN_ASSIGN_PAIRS)

constexpr size_t ANN_SEARCH_MAX_ROWS = 0xffffffffull, ANN_SEARCH_MAX_DIM = (size_t)1 << 24;
constexpr uint64_t ANN_SEARCH_MAX_TASKS = 0x7fffffffull;   // one workgroup a task: what a grid holds
constexpr uint32_t ANN_SEARCH_WG_PER_CU = 2;   // the workgroups a CU holds at once (LDS and registers: DESIGN §4r); span = 0 aims at one round of them

// One workgroup's work: queries order[q_start .. q_start + q_count) against rows [v_lo, v_hi) of the vectors array; row v is reported
// as idx_base + (v - v_lo); query i of the tile leaves its partial list in slot slot0 + i.
struct AnnSearchTask {
  uint32_t q_start, q_count, v_lo, v_hi, idx_base, slot0;
};

struct AnnSearchGroup {
  uint64_t lo, hi;       // rows of the vectors array
  uint64_t e_lo, e_hi;   // its entries in `order` / `base`
};

struct AnnSearchPlan {
  uint32_t R, C, t;
  uint64_t span;            // rows of a piece, a multiple of C
  uint32_t lds_bytes;       // the stage, the R t list entries with their indices, the fill counts and the tile's query numbers
  uint64_t n_slots;         // partial lists: one per (task, query of its tile)
  uint64_t norm_words;      // cosine alone: the norms of the Q queries, then of the rows of the vectors array
  uint64_t work_bytes;      // device work space: the lists (t (32 + 4) + 4 bytes a slot) and the norms
  std::vector<AnnSearchTask> tasks;
  std::vector<uint32_t> order;        // query numbers, group by group: a tile is a run of at most R of them
  std::vector<uint32_t> base;         // per entry of `order`: the group's offset in that query's candidate list
  std::vector<uint32_t> list_off;     // (Q + 1): query j's partial lists are list_slots[list_off[j] .. list_off[j + 1])
  std::vector<uint32_t> list_slots;   // the slot of a partial list ...
  std::vector<uint32_t> list_base;    // ... and the base the merge adds to its indices
  std::vector<uint32_t> last;         // (Q): the largest candidate index of every query, N_j - 1
};

static inline int ann_search_refuse(const char** why, const char* text) {
  *why = text;
  return ANN_ASSIGN_PLAN_REFUSED;
}

// What both forms share once the groups and their entries stand in p->order / p->base: `n_cand[j]` the candidates of query j.
static inline int ann_search_plan_groups(const std::vector<AnnSearchGroup>& groups, const std::vector<uint64_t>& n_cand, size_t dim, size_t t,
                                         uint64_t span, uint32_t cus, bool cosine, uint64_t vec_rows, AnnSearchPlan* p, const char** why) {
  const size_t Q = n_cand.size();
  if (dim == 0 || dim > ANN_SEARCH_MAX_DIM) return ann_search_refuse(why, "ann search: dim = 0 or above 2^24");
  if (t == 0 || t > ANN_SEARCH_T_MAX) return ann_search_refuse(why, "ann search: t = 0 or above 64");
  uint64_t longest = 0;
  for (const AnnSearchGroup& g : groups)
    if (g.e_hi > g.e_lo && g.hi - g.lo > longest) longest = g.hi - g.lo;
  for (size_t j = 0; j < Q; j++) {
    if (n_cand[j] < t) return ann_search_refuse(why, "ann search: t above a query's candidate count");
    if (n_cand[j] > ANN_SEARCH_MAX_ROWS) return ann_search_refuse(why, "ann search: a query has more than 2^32 - 1 candidates");
  }
  // C: the smallest of 16, 32, 64 that holds max(t, min(longest range, 64)); R takes what is left of the workgroup's 1,024 pairs
  const uint64_t hold = t > (longest < 64 ? longest : 64) ? t : (longest < 64 ? longest : 64);
  uint32_t C = ANN_ASSIGN_C_MIN;
  while (C < ANN_ASSIGN_C_MAX && C < hold) C *= 2;
  const uint32_t R = ANN_ASSIGN_THREADS * ANN_ASSIGN_PAIRS / C;
  p->C = C;
  p->R = R;
  p->t = (uint32_t)t;
  uint64_t tiles = 0;   // with one piece a group
  for (const AnnSearchGroup& g : groups)
    if (g.hi > g.lo) tiles += (g.e_hi - g.e_lo + R - 1) / R;
  if (span == 0) {
    // pieces enough for one round of resident workgroups on every CU, none below one chunk
    const uint64_t target = (uint64_t)(cus ? cus : 1) * ANN_SEARCH_WG_PER_CU;
    const uint64_t pieces = tiles && tiles < target ? (target + tiles - 1) / tiles : 1;
    span = (longest + pieces - 1) / pieces;
  }
  span = span < C ? C : (span + C - 1) / C * C;
  p->span = span;
  uint64_t n_tasks = 0, n_slots = 0;
  for (const AnnSearchGroup& g : groups) {
    if (g.hi == g.lo) continue;
    const uint64_t pieces = (g.hi - g.lo + span - 1) / span;
    n_tasks += (g.e_hi - g.e_lo + R - 1) / R * pieces;
    n_slots += (g.e_hi - g.e_lo) * pieces;
    if (n_tasks > ANN_SEARCH_MAX_TASKS || n_slots > ANN_SEARCH_MAX_ROWS) return ann_search_refuse(why, "ann search: more than 2^31 - 1 tasks (a grid) or 2^32 - 1 partial lists");
  }
  p->n_slots = n_slots;
  p->lds_bytes = (uint32_t)(ANN_ASSIGN_STAGE_WORDS * 32 + ANN_SEARCH_LIST_WORDS * (32 + 4) + 2 * ANN_ASSIGN_R_MAX * 4);
  p->norm_words = cosine ? (uint64_t)Q + vec_rows : 0;
  p->work_bytes = n_slots * (t * (32 + 4) + 4) + p->norm_words * 32;
  p->tasks.clear();
  p->tasks.reserve(n_tasks);
  std::vector<uint32_t> count(Q + 1, 0);
  for (const AnnSearchGroup& g : groups) {
    if (g.hi == g.lo) continue;
    const uint64_t pieces = (g.hi - g.lo + span - 1) / span;
    for (uint64_t e = g.e_lo; e < g.e_hi; e++) count[p->order[e] + 1] += (uint32_t)pieces;
  }
  p->list_off.assign(Q + 1, 0);
  for (size_t j = 0; j < Q; j++) p->list_off[j + 1] = p->list_off[j] + count[j + 1];
  p->list_slots.assign(n_slots, 0);
  p->list_base.assign(n_slots, 0);
  std::vector<uint32_t> cursor(p->list_off.begin(), p->list_off.end() - 1);
  uint32_t slot = 0;
  for (const AnnSearchGroup& g : groups) {
    if (g.hi == g.lo) continue;
    for (uint64_t e0 = g.e_lo; e0 < g.e_hi; e0 += R) {
      const uint32_t qc = (uint32_t)(g.e_hi - e0 < R ? g.e_hi - e0 : R);
      for (uint64_t v = g.lo; v < g.hi; v += span) {
        const uint64_t hi = g.hi - v < span ? g.hi : v + span;
        p->tasks.push_back(AnnSearchTask{(uint32_t)e0, qc, (uint32_t)v, (uint32_t)hi, (uint32_t)(v - g.lo), slot});
        for (uint32_t i = 0; i < qc; i++) {
          const uint32_t at = cursor[p->order[e0 + i]]++;
          p->list_slots[at] = slot + i;
          p->list_base[at] = p->base[e0 + i];
        }
        slot += qc;
      }
    }
  }
  p->last.resize(Q);
  for (size_t j = 0; j < Q; j++) p->last[j] = (uint32_t)(n_cand[j] - 1);
  return ANN_ASSIGN_PLAN_OK;
}

// The dense form: every query against rows [0, n).
static inline int ann_search_plan_dense(size_t Q, size_t n, size_t dim, size_t t, uint64_t span, uint32_t cus, bool cosine, AnnSearchPlan* p,
                                        const char** why) {
  if (Q == 0 || n == 0) return ann_search_refuse(why, "ann search: no query or no vector");
  if (Q > ANN_SEARCH_MAX_ROWS || n > ANN_SEARCH_MAX_ROWS) return ann_search_refuse(why, "ann search: Q and n at most 2^32 - 1");
  if (t > n) return ann_search_refuse(why, "ann search: t above a query's candidate count");
  p->order.resize(Q);
  for (size_t j = 0; j < Q; j++) p->order[j] = (uint32_t)j;
  p->base.assign(Q, 0);
  return ann_search_plan_groups({AnnSearchGroup{0, n, 0, Q}}, std::vector<uint64_t>(Q, n), dim, t, span, cus, cosine, n, p, why);
}

// The index form: query j probes clusters[j p .. j p + p) in round order, cluster k being rows [offsets[k], offsets[k + 1]) of the
// grouped array.  The (query, round) pairs are grouped by cluster with a counting sort (stable: a cluster's queries rise).
static inline int ann_search_plan_probed(const uint64_t* offsets, const uint32_t* clusters, size_t Q, size_t K, size_t dim, size_t probes, size_t t,
                                         uint64_t span, uint32_t cus, bool cosine, AnnSearchPlan* p, const char** why) {
  if (Q == 0 || K == 0 || probes == 0) return ann_search_refuse(why, "ann search: no query, no cluster or no probe");
  if (Q > ANN_SEARCH_MAX_ROWS || K > ANN_SEARCH_MAX_ROWS || probes > K) return ann_search_refuse(why, "ann search: Q and K at most 2^32 - 1, probes at most K");
  if ((uint64_t)Q * probes > ANN_SEARCH_MAX_ROWS) return ann_search_refuse(why, "ann search: more than 2^32 - 1 (query, probe) pairs");
  if (offsets[0] != 0 || offsets[K] > ANN_SEARCH_MAX_ROWS) return ann_search_refuse(why, "ann search: offsets do not start at 0, or more than 2^32 - 1 rows");
  for (size_t k = 0; k < K; k++)
    if (offsets[k] > offsets[k + 1]) return ann_search_refuse(why, "ann search: offsets that do not rise");
  std::vector<uint64_t> start(K + 1, 0);
  for (size_t e = 0; e < Q * probes; e++) {
    if (clusters[e] >= K) return ann_search_refuse(why, "ann search: a probed cluster at or above K");
    start[clusters[e] + 1]++;
  }
  for (size_t k = 0; k < K; k++) start[k + 1] += start[k];
  std::vector<AnnSearchGroup> groups;
  for (size_t k = 0; k < K; k++)
    if (start[k + 1] > start[k]) groups.push_back(AnnSearchGroup{offsets[k], offsets[k + 1], start[k], start[k + 1]});
  p->order.assign(Q * probes, 0);
  p->base.assign(Q * probes, 0);
  std::vector<uint64_t> n_cand(Q, 0), cursor(start.begin(), start.end() - 1);
  for (size_t j = 0; j < Q; j++)
    for (size_t r = 0; r < probes; r++) {
      const uint32_t k = clusters[j * probes + r];
      const uint64_t at = cursor[k]++;
      p->order[at] = (uint32_t)j;
      p->base[at] = (uint32_t)(n_cand[j] > ANN_SEARCH_MAX_ROWS ? ANN_SEARCH_MAX_ROWS : n_cand[j]);   // (refused below where it is cut)
      n_cand[j] += offsets[k + 1] - offsets[k];
    }
  return ann_search_plan_groups(groups, n_cand, dim, t, span, cus, cosine, offsets[K], p, why);
}

}  // namespace vdb
