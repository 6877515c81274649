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

// The head of every circuit against the index root over K clusters, first stream cell of each block: A the header [c | centroids_root |
// cluster roots] (n_in cells from 0), B the indicators, C select_by_indicator, D the sponge over the header's roots; `end`: behind D
struct AnnHead {
  uint64_t n_in, b_ind, b_sel, b_old, end;
};
static inline AnnHead ann_head(uint64_t K, uint64_t sponge_cells) {
  const uint64_t b_ind = K + 2, b_sel = b_ind + 8 + 12 * (K - 1), b_old = b_sel + 1 + 3 * K;
  return AnnHead{K + 2, b_ind, b_sel, b_old, b_old + sponge_cells};
}
// a batch against the index root (the update's and the delete's), behind the head: E the update block, S the delete's proof that the
// dropped half is empty (b_shr; no cells in the update and when the tree keeps its size), F the K selects, G the new sponge
struct AnnuBlocks {
  AnnHead h;
  uint64_t b_upd, b_shr, b_new, b_root, total;
};
static inline AnnuBlocks annu_blocks(uint64_t K, uint64_t sponge_cells, uint64_t update_cells, uint64_t shrink_cells = 0) {
  AnnuBlocks o;
  o.h = ann_head(K, sponge_cells);
  o.b_upd = o.h.end;
  o.b_shr = o.b_upd + update_cells;
  o.b_new = o.b_shr + shrink_cells;
  o.b_root = o.b_new + 8 * K;
  o.total = o.b_root + sponge_cells;
  return o;
}
// where lane j's indicator starts inside block B: is_zero (8 cells) for j = 0, then is_equal (12 cells) each
ANNU_HD static inline uint64_t annu_indicator_off(uint64_t j) { return j ? 8 + 12 * (j - 1) : 0; }

// an audit of one cluster (the routing audit and the mean audit), behind the head: I the assigned [centroids K x dim | members n_c x dim],
// the audit's own blocks (own_cells of them from b_own), MC and MM the merkle_commitments of the centroids and of the members
struct AnnCluster {
  AnnHead h;
  uint64_t b_in, b_own, b_mc, b_mm, total;
};
static inline AnnCluster ann_cluster(const AnnHead& h, uint64_t K, uint64_t n_c, uint64_t dim, uint64_t own_cells, uint64_t mc_cells, uint64_t mm_cells) {
  const uint64_t b_own = h.end + (K + n_c) * dim, b_mc = b_own + own_cells, b_mm = b_mc + mc_cells;
  return AnnCluster{h, h.end, b_own, b_mc, b_mm, b_mm + mm_cells};
}

// ------------------------------------------------------------------ the audit of one cluster's routing (include/vdb.h vdb_wit_ann_audit)
// its own block R in the cluster frame f: one sub-block of per_member cells per member from f.b_own on: K distances, the K - 1 qmin of
// the chain (at chain_off), then select_by_indicator over the K distances (1 + 3 K cells, at pick_off inside the sub-block).
// Lookup cells are R's alone, per_member_l per member: the distance runs, then the qmin runs (at chain_loff).
struct AnnaBlocks {
  AnnCluster f;
  uint64_t per_member, per_member_l, chain_off, chain_loff, pick_off, total_l;
};
static inline AnnaBlocks anna_blocks(uint64_t K, uint64_t n_c, uint64_t dim, uint64_t sponge_cells, uint64_t dist_cells, uint64_t dist_lk,
                                     uint64_t qmin_cells, uint64_t qmin_lk, uint64_t mc_cells, uint64_t mm_cells) {
  AnnaBlocks o;
  o.chain_off = K * dist_cells;
  o.chain_loff = K * dist_lk;
  o.pick_off = o.chain_off + (K - 1) * qmin_cells;
  o.per_member = o.pick_off + 1 + 3 * K;
  o.per_member_l = o.chain_loff + (K - 1) * qmin_lk;
  o.total_l = n_c * o.per_member_l;
  o.f = ann_cluster(ann_head(K, sponge_cells), K, n_c, dim, n_c * o.per_member, mc_cells, mm_cells);
  return o;
}

// ------------------------------------------------------------------ the mean audit of one cluster (include/vdb.h vdb_wit_ann_mean)
// its own blocks in the cluster frame f, first stream cell of each: S select_by_indicator(centroids, ind) word by word (1 + 3 K cells each,
// from b_s = f.b_own) -> own, M: the constant len = quantization(n_c) at b_m, the qadd chain from b_chain on (4 cells per member after the
// first and word, member-major), the dim qdiv blocks from b_div on.  Lookup cells are the qdiv blocks' alone, word j's from j * qdiv_lk on.
struct AnnmBlocks {
  AnnCluster f;
  uint64_t b_s, b_m, b_chain, b_div, total_l;
};
static inline AnnmBlocks annm_blocks(uint64_t K, uint64_t n_c, uint64_t dim, uint64_t sponge_cells, uint64_t qdiv_cells, uint64_t qdiv_lk,
                                     uint64_t mc_cells, uint64_t mm_cells) {
  AnnmBlocks o;
  const uint64_t s_cells = dim * (1 + 3 * K), chain_cells = (n_c - 1) * dim * 4;
  o.f = ann_cluster(ann_head(K, sponge_cells), K, n_c, dim, s_cells + 1 + chain_cells + dim * qdiv_cells, mc_cells, mm_cells);
  o.b_s = o.f.b_own;
  o.b_m = o.b_s + s_cells;
  o.b_chain = o.b_m + 1;
  o.b_div = o.b_chain + chain_cells;
  o.total_l = dim * qdiv_lk;
  return o;
}

// ------------------------------------------------------------------ the recentre of one cluster (include/vdb.h vdb_wit_ann_recentre)
// behind the head, first stream cell of each block: I the assigned members n_c x dim (b_in), M as the mean audit has it (the constant
// len at b_m, the qadd chain from b_chain, the dim qdiv blocks from b_div), MM merkle_commitment(members) (b_mm), U the update block
// of the centroids' tree with one write (b_upd), G the sponge over [new centroids' root | cluster roots] (b_root).  Lookup cells are the
// qdiv blocks' alone, word j's from j * qdiv_lk on.
struct AnnrBlocks {
  AnnHead h;
  uint64_t b_in, b_m, b_chain, b_div, b_mm, b_upd, b_root, total, total_l;
};
static inline AnnrBlocks annr_blocks(uint64_t K, uint64_t n_c, uint64_t dim, uint64_t sponge_cells, uint64_t qdiv_cells, uint64_t qdiv_lk,
                                     uint64_t mm_cells, uint64_t update_cells) {
  AnnrBlocks o;
  o.h = ann_head(K, sponge_cells);
  o.b_in = o.h.end;
  o.b_m = o.b_in + n_c * dim;
  o.b_chain = o.b_m + 1;
  o.b_div = o.b_chain + (n_c - 1) * dim * 4;
  o.b_mm = o.b_div + dim * qdiv_cells;
  o.b_upd = o.b_mm + mm_cells;
  o.b_root = o.b_upd + update_cells;
  o.total = o.b_root + sponge_cells;
  o.total_l = dim * qdiv_lk;
  return o;
}

// ------------------------------------------------------------------ the cover of the database by the index (include/vdb.h vdb_wit_ann_cover)
// first stream cell of each block: A the header [centroids_root | cluster roots] (from 0), I the assigned leaf digests a_0 .. a_{n-1}
// (b_a, database slot order) and b_0 .. b_{n-1} (b_b, grouped order), Z the one load_zero cell (zero: 1 where the database tree or a
// cluster tree is padded), TD the database tree's nodes (b_td), TC the K cluster trees' nodes one tree after the other (b_tc; tree c
// from b_tc + node_pre[c] * node_cells; a cluster of one member has no node), D the sponge over the header (b_d), G the sponge over
// [droot, index_root] (b_g: two words, the cells of a node), then the products: SA the n g_sub(gamma, a_i) (b_sa), MA the n - 1 g_mul
// (b_ma), SB and MB the same over b.  No lookup cell.
struct AnncBlocks {
  uint64_t n, lp, zero, nodes_c, n_in, b_a, b_b, b_z, b_td, b_tc, b_d, b_g, b_sa, b_ma, b_sb, b_mb, total;
};
// sizes: the K cluster sizes.  -> 0; 1: K = 0 or an empty cluster; 2: n above max_n (the sum is cut off there: no overflow)
static inline int annc_blocks(const uint64_t* sizes, uint64_t K, uint64_t max_n, uint64_t sponge_cells, uint64_t node_cells, AnncBlocks* o) {
  if (K == 0) return 1;
  uint64_t n = 0, nodes_c = 0, padded = 0;
  for (uint64_t c = 0; c < K; c++) {
    if (sizes[c] == 0) return 1;
    if (sizes[c] > max_n || n + sizes[c] > max_n) return 2;
    uint64_t lp_c;
    uint32_t d;
    tree_shape(sizes[c], &lp_c, &d);
    n += sizes[c];
    nodes_c += lp_c - 1;
    padded |= lp_c > sizes[c];
  }
  uint32_t d;
  o->n = n;
  tree_shape(n, &o->lp, &d);
  o->zero = (o->lp > n || padded) ? 1 : 0;
  o->nodes_c = nodes_c;
  o->n_in = K + 1 + 2 * n;
  o->b_a = K + 1;
  o->b_b = o->b_a + n;
  o->b_z = o->b_b + n;
  o->b_td = o->b_z + o->zero;
  o->b_tc = o->b_td + (o->lp - 1) * node_cells;
  o->b_d = o->b_tc + nodes_c * node_cells;
  o->b_g = o->b_d + sponge_cells;
  o->b_sa = o->b_g + node_cells;
  o->b_ma = o->b_sa + 4 * n;
  o->b_sb = o->b_ma + 4 * (n - 1);
  o->b_mb = o->b_sb + 4 * n;
  o->total = o->b_mb + 4 * (n - 1);
  return 0;
}

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

// ------------------------------------------------------------------ deletes (include/vdb.h vdb_wit_ann_delete, vdb_ann_index_remove_dev)
// A delete of slot i moves the last member into i and empties the last slot, so the members stay dense: delete j of a batch is two
// path updates, 2 j at slot_j with the CARRIED leaf (the one at fill - 1 at that turn) and 2 j + 1 at fill - 1, a plain delete.  In a
// delete-only batch every leaf of the cluster is an original leaf or 0, so where a leaf came from is tracked without a value:
// origin[p] = the slot that held, before the batch, what position p holds now.  Only positions a delete wrote differ from p itself
// (at most m of them): they are kept as a short list, latest first wins.
struct AnndPlan {
  std::vector<uint64_t> indices;      // 2 m: the path updates' slots
  std::vector<uint8_t> kinds;         // 2 m: 2 (carried), 1 (delete), alternating
  std::vector<uint32_t> carry_src;    // 2 m: for update 2 j the slot whose leaf, as the tree stood before the batch, it carries
  std::vector<uint64_t> move_pos, move_src;   // the surviving positions p < n_c - m whose member is not the original one: p, origin[p]
  std::vector<uint64_t> removed_src;  // m: the slot that held, before the batch, the member delete j removes (origin[slot_j] at its turn)
  uint64_t lp, lp_new;                // padded leaf counts before and after: lp_new = lp >> shrink is the power of two >= n_c - m
  uint32_t depth, shrink;
};
// -> 0; 1: m == 0 or 2 m above max_updates; 2: m >= n_c (an emptied cluster is refused, as the build refuses one);
// 3: slots[*bad] is at or above the fill at its turn
static inline int annd_expand(const uint64_t* slots, size_t m, uint64_t n_c, size_t max_updates, AnndPlan* p, size_t* bad) {
  if (m == 0 || m > max_updates / 2) return 1;
  if (m >= n_c) return 2;
  tree_shape(n_c, &p->lp, &p->depth);
  uint32_t d_new;
  tree_shape(n_c - m, &p->lp_new, &d_new);
  p->shrink = p->depth - d_new;
  p->indices.assign(2 * m, 0);
  p->kinds.assign(2 * m, 1);
  p->carry_src.assign(2 * m, 0);
  p->removed_src.assign(m, 0);
  std::vector<uint64_t> w_pos, w_src;   // the writes so far, in order: position, origin
  auto origin = [&](uint64_t pos) {
    for (size_t i = w_pos.size(); i-- > 0;)
      if (w_pos[i] == pos) return w_src[i];
    return pos;
  };
  for (size_t j = 0; j < m; j++) {
    const uint64_t fill = n_c - j, last = fill - 1;
    if (slots[j] >= fill) {
      if (bad) *bad = j;
      return 3;
    }
    const uint64_t src = origin(last);
    p->removed_src[j] = origin(slots[j]);
    p->indices[2 * j] = slots[j];
    p->kinds[2 * j] = 2;
    p->carry_src[2 * j] = (uint32_t)src;
    p->indices[2 * j + 1] = last;
    w_pos.push_back(slots[j]);
    w_src.push_back(src);
  }
  p->move_pos.clear();
  p->move_src.clear();
  for (size_t i = w_pos.size(); i-- > 0;) {
    const uint64_t pos = w_pos[i];
    if (pos >= n_c - m || w_src[i] == pos) continue;
    bool later = false;
    for (size_t k = i + 1; k < w_pos.size() && !later; k++) later = w_pos[k] == pos;
    if (later) continue;
    p->move_pos.push_back(pos);
    p->move_src.push_back(w_src[i]);
  }
  return 0;
}
// cells of block S, the proof that the dropped half is empty: [S_0 | Z_0 | Z_{l+1} = H(Z_l, Z_l), l < d - 1 | S_{i+1} = H(S_i, Z_{d-s+i}),
// i < s]; nothing when the tree keeps its size
static inline uint64_t annd_shrink_cells(uint32_t depth, uint32_t shrink, uint64_t node_cells) {
  return shrink ? 2 + (uint64_t)(depth - 1 + shrink) * node_cells : 0;
}
// The index after m deletes from cluster c: the K + 1 row offsets and the K + 2 segment offsets of the forest, cluster c's tree cut
// to lp_new leaves.  delta: digests by which the segments behind c move down.  -> 0; 1: an empty cluster
struct AnndRemovePlan {
  std::vector<uint64_t> offsets, seg_off;
  uint64_t n_new, off_c, keep_c, delta;   // keep_c = n_c - m, the rows of cluster c that stay
};
static inline int annd_remove_plan(const uint64_t* sizes, size_t K, size_t c, uint64_t m, uint64_t lp, uint64_t lp_new, AnndRemovePlan* p) {
  p->offsets.assign(K + 1, 0);
  p->seg_off.assign(K + 2, 0);
  for (size_t s = 0; s <= K; s++) {
    const uint64_t old_sz = s < K ? sizes[s] : K;
    if (old_sz == 0) return 1;
    uint64_t l;
    uint32_t d;
    tree_shape(old_sz, &l, &d);
    if (s == c) {
      l = lp_new;
      p->off_c = p->offsets[s];
      p->keep_c = old_sz - m;
    }
    if (s < K) p->offsets[s + 1] = p->offsets[s] + (s == c ? old_sz - m : old_sz);
    p->seg_off[s + 1] = p->seg_off[s] + 2 * l;
  }
  p->n_new = p->offsets[K];
  p->delta = 2 * (lp - lp_new);
  return 0;
}

// ------------------------------------------------------------------ moves (include/vdb.h vdb_wit_ann_move, vdb_ann_index_move_dev)
// m members pass from cluster a to cluster b: move j is delete j of a (annd_expand: two path updates of a's tree, a's tree halved s
// times) and an append to b at dest_j = n_b + j whose new leaf is CARRIED from a: the removed leaf of delete j, the digest slot
// removed_src[j] of a's tree held before the batch.  b's tree is doubled g times before the first append: g is the smallest that fits.
struct AnnMovePlan {
  AnndPlan d;                  // a's side: 2 m path updates, origin tracking, s
  std::vector<uint64_t> dest;  // m: n_b + j
  std::vector<uint8_t> kinds;  // m: 2 (carried), b's side
  uint64_t lp_b, glp_b;        // b's padded leaf counts before and after the growth
  uint32_t depth_b, grow;      // depth_b: of the grown tree
};
// the doublings after which the tree over n_b members holds n_b + m
static inline unsigned annmv_grow(uint64_t n_b, uint64_t m) {
  uint64_t lp, glp;
  uint32_t d, gd;
  tree_shape(n_b, &lp, &d);
  tree_shape(n_b + m, &glp, &gd);
  return gd - d;
}
// -> 0; 1 .. 3: annd_expand's; 4: n_b == 0; 5: `grow` (< 0: not given) is not the smallest that fits
static inline int annmv_expand(const uint64_t* slots, size_t m, uint64_t n_a, uint64_t n_b, int grow, size_t max_updates, AnnMovePlan* p, size_t* bad) {
  const int rc = annd_expand(slots, m, n_a, max_updates, &p->d, bad);
  if (rc) return rc;
  if (n_b == 0) return 4;
  uint32_t d;
  tree_shape(n_b, &p->lp_b, &d);
  tree_shape(n_b + m, &p->glp_b, &p->depth_b);
  p->grow = p->depth_b - d;
  if (grow >= 0 && (unsigned)grow != p->grow) return 5;
  p->dest.resize(m);
  for (size_t j = 0; j < m; j++) p->dest[j] = n_b + j;
  p->kinds.assign(m, 2);
  return 0;
}
// block offsets of the move circuit: A [a | b | centroids_root | cluster roots] (K + 3 cells), B_a, C_a, D, E' (b_upd_a), S (b_shr),
// F_a (b_mid), B_b (b_ind_b), C_b (b_sel_b), E_b (b_upd_b), F_b (b_new), G (b_root)
struct AnnMoveBlocks {
  uint64_t n_in, b_ind_a, b_sel_a, b_old, b_upd_a, b_shr, b_mid, b_ind_b, b_sel_b, b_upd_b, b_new, b_root, total;
};
static inline AnnMoveBlocks annmv_blocks(uint64_t K, uint64_t sponge_cells, uint64_t update_a_cells, uint64_t shrink_cells, uint64_t update_b_cells) {
  AnnMoveBlocks o;
  const uint64_t ind_cells = 8 + 12 * (K - 1), sel_cells = 1 + 3 * K;
  o.n_in = K + 3;
  o.b_ind_a = o.n_in;
  o.b_sel_a = o.b_ind_a + ind_cells;
  o.b_old = o.b_sel_a + sel_cells;
  o.b_upd_a = o.b_old + sponge_cells;
  o.b_shr = o.b_upd_a + update_a_cells;
  o.b_mid = o.b_shr + shrink_cells;
  o.b_ind_b = o.b_mid + 8 * K;
  o.b_sel_b = o.b_ind_b + ind_cells;
  o.b_upd_b = o.b_sel_b + sel_cells;
  o.b_new = o.b_upd_b + update_b_cells;
  o.b_root = o.b_new + 8 * K;
  o.total = o.b_root + sponge_cells;
  return o;
}
// The index after the batch.  Rows: cluster a's surviving position p holds its original member origin_a[p] (annd_expand's move table),
// the moved rows follow b's old rows in move order, every other row keeps its place in its cluster; a lane finds its cluster in the new
// offsets and its source through the old ones, so the rows between a and b shift by m whichever of the two comes first.  Forest: segment
// a is its updated tree cut to lp_a >> s, segment b its grown, updated tree, the others are copied from where the old forest holds them.
struct AnnMoveIndexPlan {
  std::vector<uint64_t> offsets, seg_off;          // new: K + 1 rows, K + 2 digests
  std::vector<uint64_t> offsets_old, seg_off_old;  // old, the same shapes
  uint64_t n;
};
// -> 0; 1: an empty cluster
static inline int annmv_index_plan(const uint64_t* sizes, size_t K, size_t a, size_t b, uint64_t m, uint64_t lp_a_new, uint64_t glp_b, AnnMoveIndexPlan* p) {
  p->offsets.assign(K + 1, 0);
  p->seg_off.assign(K + 2, 0);
  p->offsets_old.assign(K + 1, 0);
  p->seg_off_old.assign(K + 2, 0);
  for (size_t s = 0; s <= K; s++) {
    const uint64_t old_sz = s < K ? sizes[s] : K;
    if (old_sz == 0) return 1;
    uint64_t l_old, l;
    uint32_t d;
    tree_shape(old_sz, &l_old, &d);
    l = s == a ? lp_a_new : s == b ? glp_b : l_old;
    if (s < K) {
      p->offsets_old[s + 1] = p->offsets_old[s] + old_sz;
      p->offsets[s + 1] = p->offsets[s] + (s == a ? old_sz - m : s == b ? old_sz + m : old_sz);
    }
    p->seg_off_old[s + 1] = p->seg_off_old[s] + 2 * l_old;
    p->seg_off[s + 1] = p->seg_off[s] + 2 * l;
  }
  p->n = p->offsets[K];
  return 0;
}

// ------------------------------------------------------------------ linked writes (include/vdb.h vdb_wit_ann_write, vdb_ann_index_write_dev)
// m inserts or replacements into cluster c run through TWO trees: write j is update j of the cluster's tree at indices[j] (the update's
// block E, annu_track_fill's dense fill) and update j of the database tree at db_idx[j] with the CARRIED leaf E's update j hashed.  A
// replacement takes the database slot recorded for its member (slots[indices[j]]: what the index's slots hold for cluster c); an append
// takes n + the appends so far and records it, so a later write of the batch to the appended member finds it.  The database tree is
// doubled g_db times before the first update: g_db is the smallest that fits n + appends.
struct AnnwPlan {
  std::vector<uint64_t> db_idx;   // m
  uint64_t appends, lp_db, glp_db;   // the database's padded leaf counts before and after the growth
  uint32_t depth_db, grow_db;        // depth_db: of the grown tree
};
// slots: the n_c database slots of the cluster's members (null: unknown to the caller; then `given` is checked as far as the fills
// allow: an append's entry is n + the appends so far, a replacement's lies below that).  given (null: not given; it is required when slots
// is null): the caller's own db_idx, which must be what the expansion yields.  grow_db < 0: not given.
// -> 0; 1: indices[*bad] lies above the cluster's fill at its turn; 2: n == 0 or n_c > n; 3: slots[*bad] >= n; 4: given[*bad] is not what
// the expansion yields; 5: grow_db is not the smallest that fits
static inline int annw_expand(const uint64_t* slots, const uint64_t* indices, size_t m, uint64_t n_c, uint64_t n, const uint64_t* given, int grow_db,
                              AnnwPlan* p, size_t* bad) {
  if (n == 0 || n_c > n) return 2;
  if (slots)
    for (uint64_t i = 0; i < n_c; i++)
      if (slots[i] >= n) {
        if (bad) *bad = (size_t)i;
        return 3;
      }
  p->db_idx.assign(m, 0);
  p->appends = 0;
  uint64_t fill = n_c;
  for (size_t j = 0; j < m; j++) {
    const uint64_t s = indices[j];
    if (s > fill) {
      if (bad) *bad = j;
      return 1;
    }
    uint64_t d;
    bool known = true;
    if (s == fill) {
      d = n + p->appends++;
      fill++;
    } else if (s >= n_c) {
      d = n + (s - n_c);   // a member this batch appended: its slot was recorded at its append
    } else if (slots) {
      d = slots[s];
    } else {
      d = given ? given[j] : 0;
      known = false;
      if (!given || d >= n + p->appends) {
        if (bad) *bad = j;
        return 4;
      }
    }
    if (known && given && given[j] != d) {
      if (bad) *bad = j;
      return 4;
    }
    p->db_idx[j] = d;
  }
  tree_shape(n, &p->lp_db, &p->depth_db);
  uint32_t d0 = p->depth_db;
  tree_shape(n + p->appends, &p->glp_db, &p->depth_db);
  p->grow_db = p->depth_db - d0;
  if (grow_db >= 0 && (unsigned)grow_db != p->grow_db) return 5;
  return 0;
}
// block offsets of the linked write: the update's frame (annu_blocks: A - D, E at u.b_upd, F at u.b_new, G at u.b_root) with E_db, the
// update block of the database tree, between E and F (b_upd_db); n_pub = 4 m + 5 public values
struct AnnwBlocks {
  AnnuBlocks u;
  uint64_t b_upd_db, n_pub;
};
static inline AnnwBlocks annw_blocks(uint64_t K, uint64_t m, uint64_t sponge_cells, uint64_t update_cells, uint64_t update_db_cells) {
  AnnwBlocks o;
  o.u = annu_blocks(K, sponge_cells, update_cells, update_db_cells);   // (E_db lies where the delete has its block S)
  o.b_upd_db = o.u.b_shr;
  o.n_pub = 4 * m + 5;
  return o;
}

}  // namespace vdb
