// Host-side arithmetic of the index update (include/vdb.h vdb_wit_ann_update, vdb_ann_index_apply_dev): where the circuit's blocks
// start, the fill of the cluster over a batch of writes, and the offsets of the index after it.  Plain C++ without a device call, so
// that a stand-alone program can hold it under the host sanitizers (tools/ann_update_host_check.cpp).
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#if defined(__HIPCC__)
#define ANNU_HD __host__ __device__
#else
#define ANNU_HD
#endif

namespace vdb {

// the tree over n leaves: its padded leaf count and its depth
static inline void tree_shape(uint64_t n, uint64_t* lp, uint32_t* depth) {
  for (*lp = 1, *depth = 0; *lp < n; *lp <<= 1) ++*depth;
}

// first stream cell of every block of the update circuit over K clusters: A the header [c | centroids_root | cluster roots],
// B the indicators, C select_by_indicator, D the old sponge, E the update block, F the K selects, G the new sponge
struct AnnuBlocks {
  uint64_t n_in, b_ind, b_sel, b_old, b_upd, b_new, b_root, total;
};
static inline AnnuBlocks annu_blocks(uint64_t K, uint64_t sponge_cells, uint64_t update_cells) {
  AnnuBlocks o;
  o.n_in = K + 2;
  o.b_ind = o.n_in;
  o.b_sel = o.b_ind + 8 + 12 * (K - 1);
  o.b_old = o.b_sel + 1 + 3 * K;
  o.b_upd = o.b_old + sponge_cells;
  o.b_new = o.b_upd + update_cells;
  o.b_root = o.b_new + 8 * K;
  o.total = o.b_root + sponge_cells;
  return o;
}
// where lane j's indicator starts inside block B: is_zero (8 cells) for j = 0, then is_equal (12 cells) each
ANNU_HD static inline uint64_t annu_indicator_off(uint64_t j) { return j ? 8 + 12 * (j - 1) : 0; }

// The members of a cluster stay dense: write j goes to a slot below the fill at its turn (a replacement) or exactly at it (an append,
// which raises the fill by one).  n_c: the fill before the batch, glp: the padded leaf count of the grown tree.
// -> 0 and *appends; 1: indices[*bad] lies above the fill at its turn; 2: it lies outside the grown tree
static inline int annu_track_fill(const uint64_t* indices, size_t m, uint64_t n_c, uint64_t glp, uint64_t* appends, size_t* bad) {
  uint64_t fill = n_c;
  for (size_t j = 0; j < m; j++) {
    if (indices[j] >= glp || indices[j] > fill) {
      if (bad) *bad = j;
      return indices[j] >= glp ? 2 : 1;
    }
    if (indices[j] == fill) fill++;
  }
  if (appends) *appends = fill - n_c;
  return 0;
}

// The index after a batch with `appends` appends into cluster c whose tree was doubled `grow` times: the K + 1 row offsets, the K + 2
// segment offsets of the forest (segment K: the centroids' tree over K leaves) and what the kernels need of the old layout.
struct AnnuApplyPlan {
  std::vector<uint64_t> offsets;   // K + 1, rows
  std::vector<uint64_t> seg_off;   // K + 2, digests
  uint64_t n_old, n_new, off_c, end_c, appends, glp_c, delta;   // delta: digests by which the segments behind c move
};
// -> 0; 1: an empty cluster; 2: the grown tree is not the tree over the cluster's new size (a fresh build would differ)
static inline int annu_apply_plan(const uint64_t* sizes, size_t K, size_t c, unsigned grow, uint64_t appends, AnnuApplyPlan* p) {
  p->offsets.assign(K + 1, 0);
  p->seg_off.assign(K + 2, 0);
  p->appends = appends;
  p->delta = 0;
  for (size_t s = 0; s <= K; s++) {
    const uint64_t old_sz = s < K ? sizes[s] : K, sz = old_sz + (s == c ? appends : 0);
    if (old_sz == 0) return 1;
    uint64_t lp, lp_old;
    uint32_t d;
    tree_shape(sz, &lp, &d);
    tree_shape(old_sz, &lp_old, &d);
    if (s == c) {
      if (grow > 40 || (lp_old << grow) != lp) return 2;
      p->glp_c = lp;
      p->delta = 2 * (lp - lp_old);
      p->off_c = p->offsets[s];
      p->end_c = p->offsets[s] + old_sz;
    }
    if (s < K) p->offsets[s + 1] = p->offsets[s] + sz;
    p->seg_off[s + 1] = p->seg_off[s] + 2 * lp;
  }
  p->n_new = p->offsets[K];
  p->n_old = p->n_new - appends;
  return 0;
}

}  // namespace vdb
