// The committed database as it lies on the device, values only (include/vdb.h): the resident Poseidon Merkle tree over the vectors
// (build, grow) and the index of the approximate-nearest-neighbour queries (group, forest, roots, apply).  Nothing here emits a cell
// of a witness stream, and nothing here can read a witness call's context: gadgets.hpp is not included.  The kernels that trace the
// same trees cell by cell are witness.hip's; what both sides share is resident.hpp.
#include "resident.hpp"

#include <algorithm>
#include <cstring>
#include <vector>

#include "hostglue.hpp"

namespace vdb {

// ------------------------------------------------------------------ the resident tree (include/vdb.h vdb_merkle_tree_build_dev)
// sponge states before every permutation of every leaf (value only); leaf v's digest goes to leaves[leaf_at[v]] (null: leaves[v])
__global__ __launch_bounds__(64) void k_mk_leaf_states(const PoseidonSpec* __restrict__ sp, const u256* __restrict__ vectors, uint32_t n, uint32_t D,
                                                       uint32_t nperm, u256* __restrict__ states /* n * nperm * 3 */, u256* __restrict__ leaves,
                                                       const uint32_t* __restrict__ leaf_at) {
  uint32_t v = blockIdx.x * 64 + threadIdx.x;
  if (v >= n) return;
  u256 st[PSD_T] = {sp->cap, u256_zero(), u256_zero()};
  const u256* msg = vectors + (size_t)v * D;
  for (uint32_t p = 0; p < nperm; p++) {
    for (int i = 0; i < PSD_T; i++) states[((size_t)v * nperm + p) * PSD_T + i] = st[i];
    const int cnt = leaf_absorbs(D, p);
    u256 in[PSD_RATE] = {cnt > 0 ? msg[2 * p] : u256_zero(), cnt > 1 ? msg[2 * p + 1] : u256_zero()};
    psd_permute_absorb(sp, st, in, cnt);
  }
  leaves[leaf_at ? leaf_at[v] : v] = st[1];
}
// its one launch form (resident.hpp), for the witness drivers too: a kernel is launched only from the file that defines it
int mk_leaf_states(const PoseidonSpec* sp, const u256* vectors, uint32_t n, uint32_t D, uint32_t nperm, u256* states, u256* leaves,
                   const uint32_t* leaf_at) {
  VDB_LAUNCH(k_mk_leaf_states, dim3(std::max(1u, (unsigned)(((uint64_t)n + 63) / 64))), dim3(64), sp, vectors, n, D, nperm, states, leaves, leaf_at);
  return VDB_OK;
}
// level l + 1 of a tree from its level l (value only), a lane per node: the permutation absorbing [left, right], then the padding-only one
__global__ __launch_bounds__(64) void k_mk_level_values(const PoseidonSpec* __restrict__ sp, const u256* __restrict__ in_lv, uint32_t n_out,
                                                        u256* __restrict__ out_lv) {
  uint32_t t = blockIdx.x * 64 + threadIdx.x;
  if (t >= n_out) return;
  u256 st[PSD_T] = {sp->cap, u256_zero(), u256_zero()};
  u256 in[PSD_RATE] = {in_lv[2 * t], in_lv[2 * t + 1]};
  psd_permute_absorb(sp, st, in, 2);
  psd_permute_absorb(sp, st, in, 0);
  out_lv[t] = st[1];
}
// the levels above the lp leaf digests that `levels` holds (its layout: resident.hpp), a launch per level; the root is at *root_off
int mk_levels_from_leaves(const PoseidonSpec* sp, u256* levels, uint64_t lp, uint64_t* root_off) {
  uint64_t off = 0;
  for (uint64_t lv = lp; lv > 1; off += lv, lv /= 2)
    VDB_LAUNCH(k_mk_level_values, dim3((unsigned)((lv / 2 + 63) / 64)), dim3(64), sp, levels + off, (uint32_t)(lv / 2), levels + off + lv);
  if (root_off) *root_off = off;
  return VDB_OK;
}
// The digests of every level of merkle_commitment's tree, values only, into `levels` in the layout of resident.hpp: the lp padded leaf
// digests, then the levels one after the other (lp + lp / 2 + ... + 1 of the 2 lp entries, the last unused); the root is at *root_off.
// `states` receives the sponge state before every permutation of every leaf (n * nperm * PSD_T entries).
int mk_tree_values(const PoseidonSpec* sp, const u256* vectors, size_t n, size_t dim, const MkShape& ml, u256* states, u256* levels,
                   uint64_t* root_off) {
  const uint64_t lp = ml.n_leaves_pow2;
  VDB_HIP(hipMemsetAsync(levels, 0, 2 * lp * sizeof(u256), ctx().stream));
  TRY(mk_leaf_states(sp, vectors, (uint32_t)n, (uint32_t)dim, ml.nperm, states, levels, nullptr));
  return mk_levels_from_leaves(sp, levels, lp, root_off);
}
// the resident tree of the path updates: mk_tree_values into the caller's buffer
int merkle_tree_build_dev(const u256* vectors, size_t n, size_t dim, u256* levels) {
  const PoseidonSpec* sp;
  TRY(poseidon_spec_dev(&sp, nullptr));
  MkShape ml;
  mk_shape(n, dim, &ml);
  u256* states = (u256*)scratch_get(0, (n * ml.nperm * PSD_T + 8) * sizeof(u256));
  if (!states) return VDB_ERR_OOM;
  uint64_t root_off;
  return mk_tree_values(sp, vectors, n, dim, ml, states, levels, &root_off);
}

// ------------------------------------------------------------------ growing the resident tree (include/vdb.h vdb_merkle_tree_grow_dev)
// The tree over lp leaves (depth d) laid out again as the tree over lp << grow leaves whose new slots are empty, a lane per entry:
// level l < d keeps its lp >> l digests and continues with Z_l; level d + i holds R_i at entry 0 (R_0: the old root; R_{i+1} =
// H(R_i, Z_{d+i}): k_mk_level_values on one node, `grow` launches after this one, which leaves 0 there) and Z_{d+i} behind it.
__global__ __launch_bounds__(256) void k_mk_tree_grow(const u256* __restrict__ old_lv, uint64_t lp, uint32_t d, uint32_t grow,
                                                      const u256* __restrict__ empty, u256* __restrict__ out) {
  const uint64_t e = (uint64_t)blockIdx.x * 256 + threadIdx.x, glp = lp << grow;
  if (e >= 2 * glp) return;
  uint32_t l = 0;
  while (l < d + grow && e >= mku_level_off(glp, l + 1)) l++;
  const uint64_t i = e - mku_level_off(glp, l);
  u256 v;
  if (i >= (glp >> l)) v = u256_zero();                   // the unused last entry
  else if (l < d) v = i < (lp >> l) ? old_lv[mku_level_off(lp, l) + i] : empty[l];
  else if (i) v = empty[l];
  else v = l == d ? old_lv[mku_level_off(lp, d)] : u256_zero();
  out[e] = v;
}

// the tree of vdb_merkle_tree_build_dev with its padded leaf count doubled `grow` times, the new slots empty, into `grown`
int merkle_tree_grow_dev(const u256* levels, size_t n, unsigned grow, u256* grown) {
  VDB_ARG(n > 0 && n <= ((size_t)1 << 30), "empty database or tree deeper than 30 levels");
  uint64_t lp;
  uint32_t d;
  tree_shape(n, &lp, &d);
  VDB_ARG(d + (uint64_t)grow <= 30, "grown tree deeper than 30 levels");
  const PoseidonSpec* sp;
  TRY(poseidon_spec_dev(&sp, nullptr));
  const u256* empty;
  TRY(poseidon_empty_subtrees_dev(&empty));
  const uint64_t glp = lp << grow;
  VDB_LAUNCH(k_mk_tree_grow, dim3((unsigned)((2 * glp + 255) / 256)), dim3(256), levels, lp, d, (uint32_t)grow, empty, grown);
  for (uint32_t i = 0; i < grow; i++)
    VDB_LAUNCH(k_mk_level_values, dim3(1), dim3(64), sp, grown + mku_level_off(glp, d + i), 1u, grown + mku_level_off(glp, d + i + 1));
  return VDB_OK;
}

// ------------------------------------------------------------------ the index of an approximate-nearest-neighbour query (include/vdb.h
// vdb_ann_index_build_dev; the query's circuit is witness.hip's).  The index commits to K centroids and to the database grouped by cluster:
// index_root = sponge over [merkle_commitment(centroids), merkle_commitment(members(0)), ..., merkle_commitment(members(K - 1))].
// The K + 1 trees lie one after the other in a forest, segment s = 2 lp_s digests in mk_tree_values' layout (segment K: the centroids'),
// and are hashed level by level by ONE launch per level over all segments.
struct AnnForest {
  std::vector<uint64_t> seg_off;   // K + 2: where segment s starts in the forest, in digests
  std::vector<uint32_t> seg_lp;    // K + 1
  std::vector<uint32_t> prefix;    // depth x (K + 2): nodes of level l + 1 in the segments before s
  uint32_t depth = 0;
};
static int ann_forest_plan(const uint32_t* ids, size_t n, size_t K, AnnForest* f) {
  VDB_ARG(ids && n > 0 && K > 0, "null pointer, empty database or K = 0");
  VDB_ARG(n <= VDB_ANN_MAX_VECTORS && K <= VDB_ANN_MAX_CLUSTERS, "index too large: n at most 2^24, K at most 4096 (include/vdb.h)");
  std::vector<uint64_t> cnt(K, 0);
  for (size_t i = 0; i < n; i++) {
    VDB_ARG(ids[i] < K, "cluster id >= K");
    cnt[ids[i]]++;
  }
  f->seg_off.assign(K + 2, 0);
  f->seg_lp.assign(K + 1, 1);
  f->depth = 0;
  for (size_t s = 0; s <= K; s++) {
    const uint64_t m = s < K ? cnt[s] : K;
    VDB_ARG(m > 0, "empty cluster: merkle_commitment is undefined over zero vectors");
    uint64_t lp;
    uint32_t d;
    tree_shape(m, &lp, &d);
    f->seg_lp[s] = (uint32_t)lp;
    f->seg_off[s + 1] = f->seg_off[s] + 2 * lp;
    if (d > f->depth) f->depth = d;
  }
  f->prefix.assign((size_t)f->depth * (K + 2), 0);
  for (uint32_t l = 0; l < f->depth; l++)
    for (size_t s = 0; s <= K; s++) f->prefix[(size_t)l * (K + 2) + s + 1] = f->prefix[(size_t)l * (K + 2) + s] + (f->seg_lp[s] >> (l + 1));
  return VDB_OK;
}
// Stable grouping of the rows by cluster id, one wavefront: 64 rows at a time, a row's rank = the rows of its cluster in the tiles before
// (counts in LDS) + the lower lanes of its tile with the same id.  Then the K + 1 offsets (a serial prefix sum by lane 0), and per row
// its place among the grouped rows, the database slot that place holds and where its leaf digest goes in the forest.
__global__ __launch_bounds__(64) void k_ann_group(const uint32_t* __restrict__ ids, uint32_t n, uint32_t K, const uint64_t* __restrict__ seg_off,
                                                   uint64_t* __restrict__ offsets, uint32_t* __restrict__ rank, uint32_t* __restrict__ slots,
                                                   uint32_t* __restrict__ leaf_at) {
  __shared__ uint32_t cnt[VDB_ANN_MAX_CLUSTERS];
  const uint32_t lane = threadIdx.x;
  for (uint32_t c = lane; c < K; c += 64) cnt[c] = 0;
  __syncthreads();
  for (uint32_t c0 = 0; c0 < n; c0 += 64) {
    const uint32_t i = c0 + lane;
    const bool live = i < n;
    const uint32_t id = live ? ids[i] : 0xffffffffu;
    uint32_t lower = 0, r = 0;
    bool last = true;
    for (int l = 0; l < 64; l++) {
      const uint32_t o = (uint32_t)__shfl((int)id, l);
      if (o == id) {
        if (l < (int)lane) lower++;
        if (l > (int)lane) last = false;
      }
    }
    if (live) {
      r = cnt[id] + lower;
      rank[i] = r;
    }
    __syncthreads();
    if (live && last) cnt[id] = r + 1;
    __syncthreads();
  }
  if (lane == 0) {
    uint32_t acc = 0;
    for (uint32_t c = 0; c < K; c++) {
      const uint32_t m = cnt[c];
      offsets[c] = acc;
      cnt[c] = acc;
      acc += m;
    }
    offsets[K] = acc;
  }
  __syncthreads();
  for (uint32_t i = lane; i < n; i += 64) {
    const uint32_t id = ids[i], r = rank[i], pos = cnt[id] + r;
    slots[pos] = i;
    leaf_at[pos] = (uint32_t)seg_off[id] + r;
  }
}
// the rows in grouped order, a lane per word
__global__ __launch_bounds__(256) void k_ann_gather(const u256* __restrict__ db, const uint32_t* __restrict__ slots, uint64_t n, uint32_t D,
                                                    u256* __restrict__ grouped) {
  const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= n * D) return;
  grouped[t] = db[(uint64_t)slots[t / D] * D + t % D];
}
// level l + 1 of every tree of the forest from its level l: a lane per (segment, node), the segment found in the prefix sums of the
// level's node counts (a segment shallower than the level has no node and no lane)
__global__ __launch_bounds__(64) void k_ann_forest_level(const PoseidonSpec* __restrict__ sp, u256* __restrict__ forest, const uint64_t* __restrict__ seg_off,
                                                          const uint32_t* __restrict__ seg_lp, const uint32_t* __restrict__ prefix, uint32_t n_seg,
                                                          uint32_t l) {
  const uint32_t t = blockIdx.x * 64 + threadIdx.x;
  if (t >= prefix[n_seg]) return;
  uint32_t lo = 0, hi = n_seg;   // the last segment s with prefix[s] <= t (segments without a node share their successor's prefix)
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) / 2;
    if (prefix[mid] <= t) lo = mid; else hi = mid;
  }
  const uint32_t node = t - prefix[lo];
  const uint64_t lp = seg_lp[lo];
  const u256* in_lv = forest + seg_off[lo] + mku_level_off(lp, l);
  u256 st[PSD_T] = {sp->cap, u256_zero(), u256_zero()};
  u256 in[PSD_RATE] = {in_lv[2 * node], in_lv[2 * node + 1]};
  psd_permute_absorb(sp, st, in, 2);
  psd_permute_absorb(sp, st, in, 0);
  forest[seg_off[lo] + mku_level_off(lp, l + 1) + node] = st[1];
}
// [centroids' root | the K cluster roots]: the words the index root is the sponge of
__global__ __launch_bounds__(64) void k_ann_roots(const u256* __restrict__ forest, const uint64_t* __restrict__ seg_off, const uint32_t* __restrict__ seg_lp,
                                                   uint32_t K, u256* __restrict__ roots) {
  const uint32_t s = blockIdx.x * 64 + threadIdx.x;
  if (s > K) return;
  roots[s == K ? 0 : 1 + s] = forest[seg_off[s] + 2 * (uint64_t)seg_lp[s] - 2];
}

int ann_index_build_dev(const u256* db, const uint32_t* ids, const u256* centroids, size_t n, size_t K, size_t dim, u256* grouped, uint32_t* slots,
                        uint64_t* offsets, u256* forest, u256* roots) {
  static thread_local AnnForest f;   // (pageable source of an asynchronous upload: it outlives the call)
  TRY(ann_forest_plan(ids, n, K, &f));
  const PoseidonSpec* sp;
  TRY(poseidon_spec_dev(&sp, nullptr));
  hipStream_t s = ctx().stream;
  const size_t n_seg = K + 1, n_pre = (size_t)f.depth * (K + 2);
  // work space: [seg_off | seg_lp, prefix, ids, rank, leaf_at] and the sponge states of the larger of the two leaf launches
  uint8_t* w = (uint8_t*)scratch_get(7, (K + 2) * 8 + (n_seg + n_pre + 3 * n + 16) * 4);
  if (!w) return VDB_ERR_OOM;
  uint64_t* d_off = (uint64_t*)w;
  uint32_t* d_lp = (uint32_t*)(d_off + K + 2);
  uint32_t *d_pre = d_lp + n_seg, *d_ids = d_pre + n_pre, *d_rank = d_ids + n, *d_at = d_rank + n;
  MkShape ml, mw;
  mk_shape(n, dim, &ml);
  mk_shape(1, K + 1, &mw);
  const size_t n_states = std::max((n > K ? n : K) * (size_t)ml.nperm, (size_t)mw.nperm) * PSD_T;
  u256* states = (u256*)scratch_get(0, (n_states + 8) * sizeof(u256));
  if (!states) return VDB_ERR_OOM;
  VDB_HIP(hipMemcpyAsync(d_off, f.seg_off.data(), (K + 2) * 8, hipMemcpyHostToDevice, s));
  VDB_HIP(hipMemcpyAsync(d_lp, f.seg_lp.data(), n_seg * 4, hipMemcpyHostToDevice, s));
  if (n_pre) VDB_HIP(hipMemcpyAsync(d_pre, f.prefix.data(), n_pre * 4, hipMemcpyHostToDevice, s));
  VDB_HIP(hipMemcpyAsync(d_ids, ids, n * 4, hipMemcpyHostToDevice, s));
  VDB_HIP(hipMemsetAsync(forest, 0, f.seg_off[K + 1] * sizeof(u256), s));
  VDB_LAUNCH(k_ann_group, dim3(1), dim3(64), d_ids, (uint32_t)n, (uint32_t)K, d_off, offsets, d_rank, slots, d_at);
  VDB_LAUNCH(k_ann_gather, dim3((unsigned)((n * dim + 255) / 256)), dim3(256), db, slots, (uint64_t)n, (uint32_t)dim, grouped);
  // the leaf of a row does not depend on its cluster: one launch over the grouped rows, one over the centroids
  TRY(mk_leaf_states(sp, grouped, (uint32_t)n, (uint32_t)dim, ml.nperm, states, forest, d_at));
  TRY(mk_leaf_states(sp, centroids, (uint32_t)K, (uint32_t)dim, ml.nperm, states, forest + f.seg_off[K], nullptr));
  for (uint32_t l = 0; l < f.depth; l++)
    VDB_LAUNCH(k_ann_forest_level, dim3((unsigned)((f.prefix[(size_t)l * (K + 2) + n_seg] + 63) / 64)), dim3(64), sp, forest, d_off, d_lp,
               d_pre + (size_t)l * (K + 2), (uint32_t)n_seg, l);
  VDB_LAUNCH(k_ann_roots, dim3((unsigned)(K / 64 + 1)), dim3(64), forest, d_off, d_lp, (uint32_t)K, roots);
  TRY(mk_leaf_states(sp, roots, 1u, (uint32_t)(K + 1), mw.nperm, states, roots + K + 1, nullptr));
  // (the host arrays are read when the copies are enqueued on this runtime; the synchronisation makes that no assumption here, where
  //  the next call of this thread rewrites them)
  VDB_HIP(hipStreamSynchronize(s));
  return VDB_OK;
}

// ------------------------------------------------------------------ the index after a batch of writes (include/vdb.h
// vdb_ann_index_apply_dev; the batch's circuit is witness.hip's).
// The next index from the old one, the updated tree of cluster c and the batch (values only; the old buffers are only read).
// One lane per word of the new grouped rows, then per new slot entry: rows up to the end of cluster c's old rows stay where they are,
// the appended rows follow them, later rows move by the number of appends; inside cluster c the last write of the batch to a slot wins
__global__ __launch_bounds__(256) void k_ann_rows_apply(const u256* __restrict__ grouped, const uint32_t* __restrict__ slots,
                                                        const u256* __restrict__ new_vectors, const uint32_t* __restrict__ idx, uint32_t m,
                                                        const uint32_t* __restrict__ db_slots, uint64_t off_c, uint64_t end_c, uint64_t appends,
                                                        uint64_t n_new, uint32_t D, u256* __restrict__ grouped_out, uint32_t* __restrict__ slots_out) {
  const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x, n_words = n_new * D;
  if (t >= n_words + n_new) return;
  const bool is_slot = t >= n_words;
  const uint64_t r = is_slot ? t - n_words : t / D;
  if (is_slot) {
    slots_out[r] = r < end_c ? slots[r] : r < end_c + appends ? db_slots[r - end_c] : slots[r - appends];
    return;
  }
  const uint32_t wd = (uint32_t)(t % D);
  if (r < off_c || r >= end_c + appends) {
    grouped_out[t] = grouped[(r < off_c ? r : r - appends) * D + wd];
    return;
  }
  const uint32_t s = (uint32_t)(r - off_c);
  int32_t from = -1;
  for (int32_t j = (int32_t)m - 1; j >= 0; j--)
    if (idx[j] == s) {
      from = j;
      break;
    }
  // (an appended slot always has a write: the host's fill tracking)
  grouped_out[t] = from >= 0 ? new_vectors[(uint64_t)from * D + wd] : grouped[r * D + wd];
}
// one lane per digest of the new forest: its segment by bisection in the new segment offsets; segment c comes from the updated tree,
// every other one from where the old forest holds it (the segments behind c lie `delta` digests earlier there)
__global__ __launch_bounds__(256) void k_ann_forest_move(const u256* __restrict__ forest, const u256* __restrict__ updated,
                                                         const uint64_t* __restrict__ seg_off, uint32_t n_seg, uint32_t c, uint64_t delta,
                                                         u256* __restrict__ forest_out) {
  const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= seg_off[n_seg]) return;
  uint32_t lo = 0, hi = n_seg;   // the segment s with seg_off[s] <= t < seg_off[s + 1] (no segment is empty)
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) / 2;
    if (seg_off[mid] <= t) lo = mid; else hi = mid;
  }
  forest_out[t] = lo == c ? updated[t - seg_off[lo]] : forest[lo < c ? t : t - delta];
}
// the K + 1 words of the index root: the old ones, word 1 + c the updated tree's root
__global__ __launch_bounds__(64) void k_ann_roots_apply(const u256* __restrict__ roots, const u256* __restrict__ updated, uint64_t glp, uint32_t K,
                                                        uint32_t c, u256* __restrict__ roots_out) {
  const uint32_t s = blockIdx.x * 64 + threadIdx.x;
  if (s > K) return;
  roots_out[s] = s == 1 + c ? updated[2 * glp - 2] : roots[s];
}
// what the two apply entry points share: the batch against cluster c's fill and the offsets after it (VDB_ERR_ARG, nothing launched)
static int ann_apply_plan(const uint64_t* sizes, size_t K, size_t dim, size_t cluster, unsigned grow, const uint64_t* indices, size_t m,
                          AnnuApplyPlan* p) {
  VDB_ARG(sizes && indices, "null pointer");
  VDB_ARG(K > 0 && K <= VDB_ANN_MAX_CLUSTERS && cluster < K, "K = 0, K above VDB_ANN_MAX_CLUSTERS or cluster >= K");
  VDB_ARG(dim > 0 && dim <= ((size_t)1 << 20), "dim outside [1, 2^20]");
  VDB_ARG(m > 0 && m <= MKU_MAX_UPDATES, "a batch holds 1 .. VDB_MERKLE_UPDATE_MAX_UPDATES updates");
  VDB_ARG(grow <= 30 && sizes[cluster] > 0 && sizes[cluster] <= VDB_ANN_MAX_VECTORS, "empty cluster, cluster too large or more than 30 doublings");
  uint64_t lp, appends = 0;
  uint32_t d;
  tree_shape(sizes[cluster], &lp, &d);
  VDB_ARG(annu_track_fill(indices, m, sizes[cluster], lp << grow, &appends, nullptr) == 0,
          "a write above the cluster's fill at its turn or outside the grown tree");
  const int rc = annu_apply_plan(sizes, K, cluster, grow, appends, p);
  VDB_ARG(rc != 1, "empty cluster");
  VDB_ARG(rc == 0, "the grown tree is not the tree over the cluster's new size: grow is the smallest number of doublings that fits the appends");
  VDB_ARG(p->n_new <= VDB_ANN_MAX_VECTORS, "index too large: n at most VDB_ANN_MAX_VECTORS");
  return VDB_OK;
}
// the launches of a planned batch (`p` outlives the call: the pageable source of asynchronous uploads); db_slots null: the appends go to
// the database slots n, n + 1, .. (the linked write's)
static int ann_apply_run(const AnnuApplyPlan& p, const u256* grouped, const uint32_t* slots, const u256* forest, const u256* roots, size_t K, size_t dim,
                         size_t cluster, const u256* updated, const u256* new_vectors, const uint64_t* indices, const uint32_t* db_slots, size_t m,
                         u256* grouped_out, uint32_t* slots_out, uint64_t* offsets_out, u256* forest_out, u256* roots_out) {
  static thread_local std::vector<uint32_t> tab;  // [idx m | db_slots appends]
  const PoseidonSpec* sp;
  TRY(poseidon_spec_dev(&sp, nullptr));
  hipStream_t s = ctx().stream;
  MkShape mw;
  mk_shape(1, K + 1, &mw);
  tab.resize(m + p.appends + 1);
  for (size_t j = 0; j < m; j++) tab[j] = (uint32_t)indices[j];
  for (size_t i = 0; i < p.appends; i++) tab[m + i] = db_slots ? db_slots[i] : (uint32_t)(p.n_old + i);
  uint8_t* w = (uint8_t*)scratch_get(7, (K + 2) * 8 + (m + p.appends + 16) * 4);
  if (!w) return VDB_ERR_OOM;
  uint64_t* d_off = (uint64_t*)w;
  uint32_t* d_idx = (uint32_t*)(d_off + K + 2);
  u256* states = (u256*)scratch_get(0, ((size_t)mw.nperm * PSD_T + 8) * sizeof(u256));
  if (!states) return VDB_ERR_OOM;
  VDB_HIP(hipMemcpyAsync(d_off, p.seg_off.data(), (K + 2) * 8, hipMemcpyHostToDevice, s));
  VDB_HIP(hipMemcpyAsync(d_idx, tab.data(), (m + p.appends) * 4, hipMemcpyHostToDevice, s));
  VDB_HIP(hipMemcpyAsync(offsets_out, p.offsets.data(), (K + 1) * 8, hipMemcpyHostToDevice, s));
  const uint64_t lanes = p.n_new * dim + p.n_new;
  VDB_LAUNCH(k_ann_rows_apply, dim3((unsigned)((lanes + 255) / 256)), dim3(256), grouped, slots, new_vectors, d_idx, (uint32_t)m, d_idx + m, p.off_c,
             p.end_c, p.appends, p.n_new, (uint32_t)dim, grouped_out, slots_out);
  VDB_LAUNCH(k_ann_forest_move, dim3((unsigned)((p.seg_off[K + 1] + 255) / 256)), dim3(256), forest, updated, d_off, (uint32_t)(K + 1), (uint32_t)cluster,
             p.delta, forest_out);
  VDB_LAUNCH(k_ann_roots_apply, dim3((unsigned)(K / 64 + 1)), dim3(64), roots, updated, p.glp_c, (uint32_t)K, (uint32_t)cluster, roots_out);
  TRY(mk_leaf_states(sp, roots_out, 1u, (uint32_t)(K + 1), mw.nperm, states, roots_out + K + 1, nullptr));
  VDB_HIP(hipStreamSynchronize(s));
  return VDB_OK;
}
int ann_index_apply_dev(const u256* grouped, const uint32_t* slots, const u256* forest, const u256* roots, const uint64_t* sizes, size_t K, size_t dim,
                        size_t cluster, unsigned grow, const u256* updated, const u256* new_vectors, const uint64_t* indices, const uint32_t* db_slots,
                        size_t m, u256* grouped_out, uint32_t* slots_out, uint64_t* offsets_out, u256* forest_out, u256* roots_out) {
  static thread_local AnnuApplyPlan p;
  TRY(ann_apply_plan(sizes, K, dim, cluster, grow, indices, m, &p));
  VDB_ARG(db_slots || p.appends == 0, "null pointer: an append needs its database slot");
  return ann_apply_run(p, grouped, slots, forest, roots, K, dim, cluster, updated, new_vectors, indices, db_slots, m, grouped_out, slots_out, offsets_out,
                       forest_out, roots_out);
}

// ------------------------------------------------------------------ the index after the recentre of one cluster (include/vdb.h
// vdb_ann_index_recentre_dev; the circuit is witness.hip's).  Values only; the old buffers are only read.  Nothing of the members
// changes: the grouped rows, the slots, the offsets and forest segments 0 .. K - 1 are copied device to device; segment K is the
// centroids' tree as the witness call left it (`updated`), row c of the centroids is the new centroid, the centroids' root is
// `updated`'s and the index root is hashed again: one launch (the sponge), no grouping, no forest level, no member leaf.
int ann_index_recentre_dev(const u256* grouped, const uint32_t* slots, const uint64_t* offsets, const u256* forest, const u256* roots, const u256* centroids,
                           const uint64_t* sizes, size_t K, size_t dim, size_t cluster, const u256* updated, const u256* new_centroid, u256* grouped_out,
                           uint32_t* slots_out, uint64_t* offsets_out, u256* forest_out, u256* roots_out, u256* centroids_out) {
  VDB_ARG(sizes, "null pointer");
  VDB_ARG(K > 1 && K <= VDB_ANN_MAX_CLUSTERS && cluster < K, "K below 2 (a centroids' tree of one leaf has no path), K above VDB_ANN_MAX_CLUSTERS or cluster >= K");
  VDB_ARG(dim > 0 && dim <= ((size_t)1 << 20), "dim outside [1, 2^20]");
  uint64_t n = 0, seg_k = 0, lp_k;
  uint32_t d;
  for (size_t s = 0; s < K; s++) {
    VDB_ARG(sizes[s] > 0 && sizes[s] <= VDB_ANN_MAX_VECTORS, "empty cluster or cluster too large");
    uint64_t lp;
    tree_shape(sizes[s], &lp, &d);
    n += sizes[s];
    seg_k += 2 * lp;
  }
  VDB_ARG(n <= VDB_ANN_MAX_VECTORS, "index too large: n at most VDB_ANN_MAX_VECTORS");
  tree_shape(K, &lp_k, &d);
  const PoseidonSpec* sp;
  TRY(poseidon_spec_dev(&sp, nullptr));
  hipStream_t s = ctx().stream;
  MkShape mw;
  mk_shape(1, K + 1, &mw);
  u256* states = (u256*)scratch_get(0, ((size_t)mw.nperm * PSD_T + 8) * sizeof(u256));
  if (!states) return VDB_ERR_OOM;
  const auto d2d = [&](void* dst, const void* src, size_t bytes) { return hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, s); };
  VDB_HIP(d2d(grouped_out, grouped, n * dim * sizeof(u256)));
  VDB_HIP(d2d(slots_out, slots, n * sizeof(uint32_t)));
  VDB_HIP(d2d(offsets_out, offsets, (K + 1) * sizeof(uint64_t)));
  VDB_HIP(d2d(forest_out, forest, seg_k * sizeof(u256)));
  VDB_HIP(d2d(forest_out + seg_k, updated, 2 * lp_k * sizeof(u256)));
  VDB_HIP(d2d(centroids_out, centroids, K * dim * sizeof(u256)));
  VDB_HIP(d2d(centroids_out + cluster * dim, new_centroid, dim * sizeof(u256)));
  VDB_HIP(d2d(roots_out, updated + 2 * lp_k - 2, sizeof(u256)));
  VDB_HIP(d2d(roots_out + 1, roots + 1, K * sizeof(u256)));
  TRY(mk_leaf_states(sp, roots_out, 1u, (uint32_t)(K + 1), mw.nperm, states, roots_out + K + 1, nullptr));
  VDB_HIP(hipStreamSynchronize(s));
  return VDB_OK;
}

// ------------------------------------------------------------------ the database tree of an index (include/vdb.h
// vdb_ann_index_db_tree_dev; the cover's circuit is witness.hip's).  Values only: no vector is hashed again, every leaf digest already
// lies in level 0 of its cluster's forest segment.  Lane g (a grouped row) finds its cluster by bisection in the offsets, copies its
// digest to levels_out[slots[g]] and counts the hit; a slot at or above n is skipped here and flagged by the second pass
__global__ __launch_bounds__(256) void k_annc_scatter(const u256* __restrict__ forest, const uint64_t* __restrict__ seg_off, const uint64_t* __restrict__ offsets,
                                                      const uint32_t* __restrict__ slots, uint32_t K, uint32_t n, u256* __restrict__ levels_out,
                                                      uint32_t* __restrict__ count) {
  const uint32_t g = blockIdx.x * 256 + threadIdx.x;
  if (g >= n) return;
  uint32_t lo = 0, hi = K;   // the cluster c with offsets[c] <= g < offsets[c + 1] (no cluster is empty)
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) / 2;
    if (offsets[mid] <= g) lo = mid; else hi = mid;
  }
  const uint32_t slot = slots[g];
  if (slot >= n) return;
  levels_out[slot] = forest[seg_off[lo] + (g - offsets[lo])];
  atomicAdd(count + slot, 1u);
}
// lane g: a slot entry at or above n, or a slot that was not hit exactly once: `slots` is no permutation of 0 .. n - 1
__global__ __launch_bounds__(256) void k_annc_slots_check(const uint32_t* __restrict__ slots, const uint32_t* __restrict__ count, uint32_t n,
                                                          uint32_t* __restrict__ flag) {
  const uint32_t g = blockIdx.x * 256 + threadIdx.x;
  if (g >= n) return;
  if (slots[g] >= n || count[g] != 1u) atomicOr(flag, 1u);
}
int ann_index_db_tree_dev(const u256* forest, const uint64_t* sizes, const uint32_t* slots, size_t K, size_t n, u256* levels_out) {
  static thread_local std::vector<uint64_t> tab;   // [seg_off K + 1 | offsets K + 1] (pageable source of an asynchronous upload)
  VDB_ARG(sizes, "null pointer");
  VDB_ARG(K > 0 && K <= VDB_ANN_MAX_CLUSTERS, "K = 0 or K above VDB_ANN_MAX_CLUSTERS");
  VDB_ARG(n > 0 && n <= VDB_ANN_MAX_VECTORS, "empty database or n above VDB_ANN_MAX_VECTORS");
  tab.assign(2 * (K + 1), 0);
  for (size_t c = 0; c < K; c++) {
    VDB_ARG(sizes[c] > 0 && sizes[c] <= n, "empty cluster or cluster sizes that do not sum to n");
    uint64_t lp_c;
    uint32_t d;
    tree_shape(sizes[c], &lp_c, &d);
    tab[c + 1] = tab[c] + 2 * lp_c;
    tab[K + 1 + c + 1] = tab[K + 1 + c] + sizes[c];
  }
  VDB_ARG(tab[2 * K + 1] == n, "cluster sizes that do not sum to n");
  const PoseidonSpec* sp;
  TRY(poseidon_spec_dev(&sp, nullptr));
  hipStream_t s = ctx().stream;
  uint64_t lp;
  uint32_t d;
  tree_shape(n, &lp, &d);
  uint8_t* w = (uint8_t*)scratch_get(7, 2 * (K + 1) * 8 + (n + 16) * 4);
  if (!w) return VDB_ERR_OOM;
  uint64_t* d_tab = (uint64_t*)w;
  uint32_t *d_count = (uint32_t*)(d_tab + 2 * (K + 1)), *d_flag = d_count + n;
  VDB_HIP(hipMemcpyAsync(d_tab, tab.data(), 2 * (K + 1) * 8, hipMemcpyHostToDevice, s));
  VDB_HIP(hipMemsetAsync(d_count, 0, (n + 1) * 4, s));
  VDB_HIP(hipMemsetAsync(levels_out, 0, 2 * lp * sizeof(u256), s));
  const unsigned grid = (unsigned)((n + 255) / 256);
  VDB_LAUNCH(k_annc_scatter, dim3(grid), dim3(256), forest, d_tab, d_tab + K + 1, slots, (uint32_t)K, (uint32_t)n, levels_out, d_count);
  VDB_LAUNCH(k_annc_slots_check, dim3(grid), dim3(256), slots, d_count, (uint32_t)n, d_flag);
  TRY(mk_levels_from_leaves(sp, levels_out, lp, nullptr));
  uint32_t flag = 0;
  VDB_HIP(hipMemcpyAsync(&flag, d_flag, 4, hipMemcpyDeviceToHost, s));
  VDB_HIP(hipStreamSynchronize(s));
  VDB_ARG(flag == 0, "slots is not a permutation of 0 .. n - 1: the database has slots no cluster holds, or one held twice");
  return VDB_OK;
}

// ------------------------------------------------------------------ the index after a batch of deletes (include/vdb.h
// vdb_ann_index_remove_dev; the batch's circuit is witness.hip's).  Values only; the old buffers are only read.
// A removal compacts the database: the result is the fresh build over its own grouped rows taken as the database, so every grouped
// row's slot is its own place.  One lane per word of the new grouped rows, then per slot entry: rows in front of cluster c stay, its
// surviving position p holds the original member origin[p] (p itself unless the move table says otherwise: at most m entries, scanned
// per lane), later rows move down by m
__global__ __launch_bounds__(256) void k_ann_rows_remove(const u256* __restrict__ grouped, const uint32_t* __restrict__ move_pos,
                                                         const uint32_t* __restrict__ move_src, uint32_t n_move, uint64_t off_c, uint64_t keep_c,
                                                         uint64_t m, uint64_t n_new, uint32_t D, u256* __restrict__ grouped_out,
                                                         uint32_t* __restrict__ slots_out) {
  const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x, n_words = n_new * D;
  if (t >= n_words + n_new) return;
  if (t >= n_words) {
    slots_out[t - n_words] = (uint32_t)(t - n_words);
    return;
  }
  const uint64_t r = t / D;
  const uint32_t wd = (uint32_t)(t % D);
  uint64_t from = r < off_c + keep_c ? r : r + m;
  if (r >= off_c && r < off_c + keep_c) {
    const uint32_t p = (uint32_t)(r - off_c);
    for (uint32_t i = 0; i < n_move; i++)
      if (move_pos[i] == p) {
        from = off_c + move_src[i];
        break;
      }
  }
  grouped_out[t] = grouped[from * D + wd];
}
// one lane per digest of the new forest: its segment by bisection in the new segment offsets; segment c is the updated tree cut to
// lp_new leaves (level l of the cut tree is the prefix of level l of the old one, the unused last entry 0), every other segment comes
// from where the old forest holds it (the segments behind c lie `delta` digests later there)
__global__ __launch_bounds__(256) void k_ann_forest_cut(const u256* __restrict__ forest, const u256* __restrict__ updated, const uint64_t* __restrict__ seg_off,
                                                        uint32_t n_seg, uint32_t c, uint64_t lp, uint64_t lp_new, uint64_t delta,
                                                        u256* __restrict__ forest_out) {
  const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= seg_off[n_seg]) return;
  uint32_t lo = 0, hi = n_seg;
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) / 2;
    if (seg_off[mid] <= t) lo = mid; else hi = mid;
  }
  if (lo != c) {
    forest_out[t] = forest[lo < c ? t : t + delta];
    return;
  }
  uint64_t e = t - seg_off[lo], width = lp_new;
  uint32_t l = 0;
  while (width && e >= width) {
    e -= width;
    width >>= 1;
    l++;
  }
  forest_out[t] = width ? updated[mku_level_off(lp, l) + e] : u256_zero();
}
// what the two remove entry points share: the batch against cluster c's fill and the offsets after it (VDB_ERR_ARG, nothing launched)
static int ann_remove_plan(const uint64_t* sizes, size_t K, size_t dim, size_t cluster, const uint64_t* slots, size_t m, AnndPlan* dp, AnndRemovePlan* p) {
  VDB_ARG(sizes && slots, "null pointer");
  VDB_ARG(K > 0 && K <= VDB_ANN_MAX_CLUSTERS && cluster < K, "K = 0, K above VDB_ANN_MAX_CLUSTERS or cluster >= K");
  VDB_ARG(dim > 0 && dim <= ((size_t)1 << 20), "dim outside [1, 2^20]");
  VDB_ARG(sizes[cluster] <= VDB_ANN_MAX_VECTORS, "cluster too large");
  const int rc = annd_expand(slots, m, sizes[cluster], MKU_MAX_UPDATES, dp, nullptr);
  VDB_ARG(rc != 1, "a batch holds 1 .. VDB_MERKLE_UPDATE_MAX_UPDATES / 2 deletes");
  VDB_ARG(rc != 2, "the batch would empty the cluster");
  VDB_ARG(rc == 0, "a slot at or above the cluster's fill at its turn");
  VDB_ARG(annd_remove_plan(sizes, K, cluster, m, dp->lp, dp->lp_new, p) == 0, "empty cluster");
  VDB_ARG(p->n_new + m <= VDB_ANN_MAX_VECTORS, "index too large: n at most VDB_ANN_MAX_VECTORS");
  return VDB_OK;
}
int ann_index_remove_dev(const u256* grouped, const u256* forest, const u256* roots, const uint64_t* sizes, size_t K, size_t dim, size_t cluster,
                         const u256* updated, const uint64_t* slots, size_t m, u256* grouped_out, uint32_t* slots_out, uint64_t* offsets_out,
                         u256* forest_out, u256* roots_out) {
  static thread_local AnndPlan dp;                // (pageable sources of asynchronous uploads: they outlive the call)
  static thread_local AnndRemovePlan p;
  static thread_local std::vector<uint32_t> tab;  // [move_pos | move_src]
  TRY(ann_remove_plan(sizes, K, dim, cluster, slots, m, &dp, &p));
  const PoseidonSpec* sp;
  TRY(poseidon_spec_dev(&sp, nullptr));
  hipStream_t s = ctx().stream;
  MkShape mw;
  mk_shape(1, K + 1, &mw);
  const size_t n_move = dp.move_pos.size();
  tab.resize(2 * n_move + 1);
  for (size_t i = 0; i < n_move; i++) tab[i] = (uint32_t)dp.move_pos[i], tab[n_move + i] = (uint32_t)dp.move_src[i];
  uint8_t* w = (uint8_t*)scratch_get(7, (K + 2) * 8 + (2 * n_move + 16) * 4);
  if (!w) return VDB_ERR_OOM;
  uint64_t* d_off = (uint64_t*)w;
  uint32_t* d_move = (uint32_t*)(d_off + K + 2);
  u256* states = (u256*)scratch_get(0, ((size_t)mw.nperm * PSD_T + 8) * sizeof(u256));
  if (!states) return VDB_ERR_OOM;
  VDB_HIP(hipMemcpyAsync(d_off, p.seg_off.data(), (K + 2) * 8, hipMemcpyHostToDevice, s));
  if (n_move) VDB_HIP(hipMemcpyAsync(d_move, tab.data(), 2 * n_move * 4, hipMemcpyHostToDevice, s));
  VDB_HIP(hipMemcpyAsync(offsets_out, p.offsets.data(), (K + 1) * 8, hipMemcpyHostToDevice, s));
  const uint64_t lanes = p.n_new * dim + p.n_new;
  VDB_LAUNCH(k_ann_rows_remove, dim3((unsigned)((lanes + 255) / 256)), dim3(256), grouped, d_move, d_move + n_move, (uint32_t)n_move, p.off_c, p.keep_c,
             (uint64_t)m, p.n_new, (uint32_t)dim, grouped_out, slots_out);
  VDB_LAUNCH(k_ann_forest_cut, dim3((unsigned)((p.seg_off[K + 1] + 255) / 256)), dim3(256), forest, updated, d_off, (uint32_t)(K + 1), (uint32_t)cluster,
             dp.lp, dp.lp_new, p.delta, forest_out);
  // the cut tree's root lies where level d - s of the old layout starts: k_ann_roots_apply reads it as the root of a one-leaf tree there
  VDB_LAUNCH(k_ann_roots_apply, dim3((unsigned)(K / 64 + 1)), dim3(64), roots, updated + mku_level_off(dp.lp, dp.depth - dp.shrink), (uint64_t)1, (uint32_t)K,
             (uint32_t)cluster, roots_out);
  TRY(mk_leaf_states(sp, roots_out, 1u, (uint32_t)(K + 1), mw.nperm, states, roots_out + K + 1, nullptr));
  VDB_HIP(hipStreamSynchronize(s));
  return VDB_OK;
}

// ------------------------------------------------------------------ the index after a batch of moves (include/vdb.h
// vdb_ann_index_move_dev; the batch's circuit is witness.hip's).  Values only; the old buffers are only read.  The database is not
// renumbered: every row keeps its database slot, the `slots` entries travel with their rows.
// One lane per word of the new grouped rows, then per slot entry: the lane finds its cluster s by bisection in the new offsets and its
// place p in it; the source row lies in the OLD offsets: cluster a's surviving position p holds its original member origin[p] (p itself
// unless the move table says otherwise, as k_ann_rows_remove), b's position n_b + j the member move j took out of a, every other row
// position p of its own cluster: the rows between a and b shift by m whichever of the two comes first
__global__ __launch_bounds__(256) void k_ann_rows_move(const u256* __restrict__ grouped, const uint32_t* __restrict__ slots, const uint64_t* __restrict__ off_new,
                                                       const uint64_t* __restrict__ off_old, const uint32_t* __restrict__ move_pos,
                                                       const uint32_t* __restrict__ move_src, uint32_t n_move, const uint32_t* __restrict__ removed_src,
                                                       uint32_t K, uint32_t a, uint32_t b, uint64_t n_b, uint64_t n, uint32_t D,
                                                       u256* __restrict__ grouped_out, uint32_t* __restrict__ slots_out) {
  const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x, n_words = n * D;
  if (t >= n_words + n) return;
  const bool is_slot = t >= n_words;
  const uint64_t r = is_slot ? t - n_words : t / D;
  uint32_t lo = 0, hi = K;   // the cluster s with off_new[s] <= r < off_new[s + 1] (no cluster is empty)
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) / 2;
    if (off_new[mid] <= r) lo = mid; else hi = mid;
  }
  const uint64_t p = r - off_new[lo];
  uint64_t from = off_old[lo] + p;
  if (lo == a) {
    for (uint32_t i = 0; i < n_move; i++)
      if (move_pos[i] == (uint32_t)p) {
        from = off_old[a] + move_src[i];
        break;
      }
  } else if (lo == b && p >= n_b) {
    from = off_old[a] + removed_src[p - n_b];
  }
  if (is_slot)
    slots_out[r] = slots[from];
  else
    grouped_out[t] = grouped[from * D + t % D];
}
// one lane per digest of the new forest: its segment by bisection in the new segment offsets; segment a is its updated tree cut to
// lp_new leaves (as k_ann_forest_cut), segment b its grown, updated tree, every other one comes from where the old forest holds it
__global__ __launch_bounds__(256) void k_ann_forest_splice(const u256* __restrict__ forest, const u256* __restrict__ updated_a, const u256* __restrict__ updated_b,
                                                           const uint64_t* __restrict__ seg_new, const uint64_t* __restrict__ seg_old, uint32_t n_seg,
                                                           uint32_t a, uint32_t b, uint64_t lp, uint64_t lp_new, u256* __restrict__ forest_out) {
  const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= seg_new[n_seg]) return;
  uint32_t lo = 0, hi = n_seg;
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) / 2;
    if (seg_new[mid] <= t) lo = mid; else hi = mid;
  }
  uint64_t e = t - seg_new[lo];
  if (lo == b) {
    forest_out[t] = updated_b[e];
    return;
  }
  if (lo != a) {
    forest_out[t] = forest[seg_old[lo] + e];
    return;
  }
  uint64_t width = lp_new;
  uint32_t l = 0;
  while (width && e >= width) {
    e -= width;
    width >>= 1;
    l++;
  }
  forest_out[t] = width ? updated_a[mku_level_off(lp, l) + e] : u256_zero();
}
// the K + 1 words of the index root: the old ones, words 1 + a and 1 + b the two new roots
__global__ __launch_bounds__(64) void k_ann_roots_move(const u256* __restrict__ roots, const u256* __restrict__ root_a, const u256* __restrict__ root_b, uint32_t K,
                                                       uint32_t a, uint32_t b, u256* __restrict__ roots_out) {
  const uint32_t s = blockIdx.x * 64 + threadIdx.x;
  if (s > K) return;
  roots_out[s] = s == 1 + a ? *root_a : s == 1 + b ? *root_b : roots[s];
}
// what the two move entry points share: the batch against the two clusters and the offsets after it (VDB_ERR_ARG, nothing launched)
static int ann_move_plan(const uint64_t* sizes, size_t K, size_t dim, size_t a, size_t b, int grow, const uint64_t* slots, size_t m, AnnMovePlan* mp,
                         AnnMoveIndexPlan* p) {
  VDB_ARG(sizes && slots, "null pointer");
  VDB_ARG(K >= 2 && K <= VDB_ANN_MAX_CLUSTERS && a < K && b < K && a != b, "K below 2, K above VDB_ANN_MAX_CLUSTERS, a cluster >= K or src == dst");
  VDB_ARG(dim > 0 && dim <= ((size_t)1 << 20), "dim outside [1, 2^20]");
  VDB_ARG(sizes[a] <= VDB_ANN_MAX_VECTORS && sizes[b] <= VDB_ANN_MAX_VECTORS, "cluster too large");
  const int rc = annmv_expand(slots, m, sizes[a], sizes[b], grow, MKU_MAX_UPDATES, mp, nullptr);
  VDB_ARG(rc != 1, "a batch holds 1 .. VDB_MERKLE_UPDATE_MAX_UPDATES / 2 moves");
  VDB_ARG(rc != 2, "the batch would empty the source cluster");
  VDB_ARG(rc != 3, "a slot at or above the source cluster's fill at its turn");
  VDB_ARG(rc != 4, "empty destination cluster");
  VDB_ARG(rc == 0, "grow is the smallest number of doublings after which the destination's tree holds its new members");
  VDB_ARG(annmv_index_plan(sizes, K, a, b, m, mp->d.lp_new, mp->glp_b, p) == 0, "empty cluster");
  VDB_ARG(p->n <= VDB_ANN_MAX_VECTORS, "index too large: n at most VDB_ANN_MAX_VECTORS");
  return VDB_OK;
}
int ann_index_move_dev(const u256* grouped, const uint32_t* slots_in, const u256* forest, const u256* roots, const uint64_t* sizes, size_t K, size_t dim, size_t a,
                       size_t b, unsigned grow, const u256* updated_a, const u256* updated_b, const uint64_t* slots, size_t m, u256* grouped_out,
                       uint32_t* slots_out, uint64_t* offsets_out, u256* forest_out, u256* roots_out) {
  static thread_local AnnMovePlan mp;                // (pageable sources of asynchronous uploads: they outlive the call)
  static thread_local AnnMoveIndexPlan p;
  static thread_local std::vector<uint64_t> tab64;   // [offsets K + 1 | old offsets K + 1 | seg_off K + 2 | old seg_off K + 2]
  static thread_local std::vector<uint32_t> tab32;   // [move_pos | move_src | removed_src m]
  VDB_ARG(grow <= 30, "more than 30 doublings");
  TRY(ann_move_plan(sizes, K, dim, a, b, (int)grow, slots, m, &mp, &p));
  const PoseidonSpec* sp;
  TRY(poseidon_spec_dev(&sp, nullptr));
  hipStream_t s = ctx().stream;
  MkShape mw;
  mk_shape(1, K + 1, &mw);
  const size_t n_move = mp.d.move_pos.size(), n64 = 4 * K + 6, n32 = 2 * n_move + m;
  tab64.clear();
  tab64.insert(tab64.end(), p.offsets.begin(), p.offsets.end());
  tab64.insert(tab64.end(), p.offsets_old.begin(), p.offsets_old.end());
  tab64.insert(tab64.end(), p.seg_off.begin(), p.seg_off.end());
  tab64.insert(tab64.end(), p.seg_off_old.begin(), p.seg_off_old.end());
  tab32.resize(n32);
  for (size_t i = 0; i < n_move; i++) tab32[i] = (uint32_t)mp.d.move_pos[i], tab32[n_move + i] = (uint32_t)mp.d.move_src[i];
  for (size_t j = 0; j < m; j++) tab32[2 * n_move + j] = (uint32_t)mp.d.removed_src[j];
  uint8_t* w = (uint8_t*)scratch_get(7, n64 * 8 + (n32 + 16) * 4);
  if (!w) return VDB_ERR_OOM;
  uint64_t *d_off = (uint64_t*)w, *d_off_old = d_off + K + 1, *d_seg = d_off_old + K + 1, *d_seg_old = d_seg + K + 2;
  uint32_t* d_move = (uint32_t*)(d_seg_old + K + 2);
  u256* states = (u256*)scratch_get(0, ((size_t)mw.nperm * PSD_T + 8) * sizeof(u256));
  if (!states) return VDB_ERR_OOM;
  VDB_HIP(hipMemcpyAsync(d_off, tab64.data(), n64 * 8, hipMemcpyHostToDevice, s));
  VDB_HIP(hipMemcpyAsync(d_move, tab32.data(), n32 * 4, hipMemcpyHostToDevice, s));
  VDB_HIP(hipMemcpyAsync(offsets_out, p.offsets.data(), (K + 1) * 8, hipMemcpyHostToDevice, s));
  const uint64_t lanes = p.n * dim + p.n;
  VDB_LAUNCH(k_ann_rows_move, dim3((unsigned)((lanes + 255) / 256)), dim3(256), grouped, slots_in, d_off, d_off_old, d_move, d_move + n_move, (uint32_t)n_move,
             d_move + 2 * n_move, (uint32_t)K, (uint32_t)a, (uint32_t)b, sizes[b], p.n, (uint32_t)dim, grouped_out, slots_out);
  VDB_LAUNCH(k_ann_forest_splice, dim3((unsigned)((p.seg_off[K + 1] + 255) / 256)), dim3(256), forest, updated_a, updated_b, d_seg, d_seg_old, (uint32_t)(K + 1),
             (uint32_t)a, (uint32_t)b, mp.d.lp, mp.d.lp_new, forest_out);
  // the cut tree's root lies where level d - s of a's old layout starts; b's at the end of its grown tree
  VDB_LAUNCH(k_ann_roots_move, dim3((unsigned)(K / 64 + 1)), dim3(64), roots, updated_a + mku_level_off(mp.d.lp, mp.d.depth - mp.d.shrink),
             updated_b + 2 * mp.glp_b - 2, (uint32_t)K, (uint32_t)a, (uint32_t)b, roots_out);
  TRY(mk_leaf_states(sp, roots_out, 1u, (uint32_t)(K + 1), mw.nperm, states, roots_out + K + 1, nullptr));
  VDB_HIP(hipStreamSynchronize(s));
  return VDB_OK;
}

// ------------------------------------------------------------------ the index after a linked write (include/vdb.h vdb_ann_index_write_dev;
// the batch's circuit is witness.hip's).  Both resident objects are kept: the index is ann_index_apply_dev's launches (ann_apply_run on the one plan), its appends at database
// slots n, n + 1, ... in append order, and the database tree is the one the witness call wrote its carried leaves back into, copied
// device to device as it stands: no vector and no node is hashed again.
// what the two entry points share (VDB_ERR_ARG, nothing launched): ann_apply_plan's, then the database's own shape
static int ann_write_plan(const uint64_t* sizes, size_t K, size_t dim, size_t cluster, unsigned grow_c, int grow_db, const uint64_t* indices, size_t m,
                          AnnuApplyPlan* p, uint64_t* glp_db, unsigned* g_db) {
  TRY(ann_apply_plan(sizes, K, dim, cluster, grow_c, indices, m, p));
  uint64_t lp;
  uint32_t d, gd;
  tree_shape(p->n_old, &lp, &d);
  tree_shape(p->n_new, glp_db, &gd);
  *g_db = gd - d;
  VDB_ARG(grow_db < 0 || (unsigned)grow_db == *g_db, "grow_db is the smallest number of doublings after which the database tree holds the appends");
  return VDB_OK;
}
int ann_index_write_dev(const u256* grouped, const uint32_t* slots, const u256* forest, const u256* roots, const uint64_t* sizes, size_t K, size_t dim,
                        size_t cluster, unsigned grow_c, unsigned grow_db, const u256* updated_c, const u256* updated_db, const u256* new_vectors,
                        const uint64_t* indices, size_t m, u256* grouped_out, uint32_t* slots_out, uint64_t* offsets_out, u256* forest_out, u256* roots_out,
                        u256* db_tree_out) {
  static thread_local AnnuApplyPlan p;
  uint64_t glp_db;
  unsigned g_db;
  VDB_ARG(grow_db <= 30, "more than 30 doublings");
  TRY(ann_write_plan(sizes, K, dim, cluster, grow_c, (int)grow_db, indices, m, &p, &glp_db, &g_db));
  VDB_HIP(hipMemcpyAsync(db_tree_out, updated_db, 2 * glp_db * sizeof(u256), hipMemcpyDeviceToDevice, ctx().stream));
  return ann_apply_run(p, grouped, slots, forest, roots, K, dim, cluster, updated_c, new_vectors, indices, nullptr, m, grouped_out, slots_out, offsets_out,
                       forest_out, roots_out);
}

}  // namespace vdb

using namespace vdb;

extern "C" {

// the root alone, from host vectors: the one tree builder into work space (scratch slots 0 and 1 only, so that the call also goes
// through while a deferred MSM holds slot 2)
int vdb_poseidon_merkle_root(const vdb_fr* vectors, size_t n, size_t dim, vdb_fr* root) {
  VDB_REQUIRE_INIT();
  VDB_ARG(vectors && root && n > 0, "null pointer or empty database");
  VDB_ARG(n <= ((size_t)1 << 30), "tree deeper than 30 levels");
  const PoseidonSpec* sp;
  TRY(poseidon_spec_dev(&sp, nullptr));
  MkShape ml;
  mk_shape(n, dim, &ml);
  const size_t n_words = n * dim;
  u256* din = (u256*)scratch_get(0, (n_words + n * ml.nperm * PSD_T + 8) * sizeof(u256));
  u256* levels = (u256*)scratch_get(1, 2 * ml.n_leaves_pow2 * sizeof(u256));
  if (!din || !levels) return VDB_ERR_OOM;
  VDB_HIP(hipMemcpyAsync(din, vectors, n_words * sizeof(u256), hipMemcpyHostToDevice, ctx().stream));
  uint64_t root_off;
  TRY(mk_tree_values(sp, din, n, dim, ml, din + n_words, levels, &root_off));
  VDB_HIP(hipMemcpyAsync(root, levels + root_off, sizeof(u256), hipMemcpyDeviceToHost, ctx().stream));
  VDB_HIP(hipStreamSynchronize(ctx().stream));
  return VDB_OK;
}

// the resident tree (include/vdb.h)
int vdb_merkle_tree_build_dev(const vdb_fr* vectors_dev, size_t n, size_t dim, vdb_fr* levels_dev) {
  VDB_REQUIRE_INIT();
  VDB_ARG(vectors_dev && levels_dev && n > 0 && dim > 0, "null pointer or empty database");
  VDB_ARG(n <= ((size_t)1 << 30), "tree deeper than 30 levels");
  return merkle_tree_build_dev(as_u256(vectors_dev), n, dim, as_u256(levels_dev));
}
int vdb_merkle_tree_grow_dev(const vdb_fr* levels_dev, size_t n, unsigned grow, vdb_fr* grown_dev) {
  VDB_REQUIRE_INIT();
  VDB_ARG(levels_dev && grown_dev, "null pointer");
  return merkle_tree_grow_dev(as_u256(levels_dev), n, grow, as_u256(grown_dev));
}

// the index of approximate-nearest-neighbour queries (include/vdb.h)
int vdb_ann_index_forest_size(const uint32_t* cluster_ids, size_t n, size_t K, uint64_t* digests, uint64_t* segment_offsets) {
  AnnForest f;
  TRY(ann_forest_plan(cluster_ids, n, K, &f));
  if (digests) *digests = f.seg_off[K + 1];
  if (segment_offsets) memcpy(segment_offsets, f.seg_off.data(), (K + 2) * sizeof(uint64_t));
  return VDB_OK;
}
int vdb_ann_index_build_dev(const vdb_fr* vectors_dev, const uint32_t* cluster_ids, const vdb_fr* centroids_dev, size_t n, size_t K, size_t dim,
                            vdb_fr* grouped_dev, uint32_t* slots_dev, uint64_t* offsets_dev, vdb_fr* forest_dev, vdb_fr* roots_dev) {
  VDB_REQUIRE_INIT();
  VDB_ARG(vectors_dev && cluster_ids && centroids_dev && grouped_dev && slots_dev && offsets_dev && forest_dev && roots_dev && dim > 0 &&
              dim <= ((size_t)1 << 20),
          "null pointer or dim outside [1, 2^20]");
  return ann_index_build_dev(as_u256(vectors_dev), cluster_ids, as_u256(centroids_dev), n, K, dim, as_u256(grouped_dev), slots_dev, offsets_dev,
                             as_u256(forest_dev), as_u256(roots_dev));
}
int vdb_ann_index_apply_size(const uint64_t* cluster_sizes, size_t K, size_t cluster, unsigned grow, const uint64_t* indices, size_t m, uint64_t* appends,
                             uint64_t* digests, uint64_t* segment_offsets) {
  AnnuApplyPlan p;
  TRY(ann_apply_plan(cluster_sizes, K, 1, cluster, grow, indices, m, &p));
  if (appends) *appends = p.appends;
  if (digests) *digests = p.seg_off[K + 1];
  if (segment_offsets) memcpy(segment_offsets, p.seg_off.data(), (K + 2) * sizeof(uint64_t));
  return VDB_OK;
}
int vdb_ann_index_apply_dev(const vdb_fr* grouped_dev, const uint32_t* slots_dev, const vdb_fr* forest_dev, const vdb_fr* roots_dev,
                            const uint64_t* cluster_sizes, size_t K, size_t dim, size_t cluster, unsigned grow, const vdb_fr* updated_levels_dev,
                            const vdb_fr* new_vectors_dev, const uint64_t* indices, const uint32_t* db_slots, size_t m, vdb_fr* grouped_out_dev,
                            uint32_t* slots_out_dev, uint64_t* offsets_out_dev, vdb_fr* forest_out_dev, vdb_fr* roots_out_dev) {
  VDB_REQUIRE_INIT();
  VDB_ARG(grouped_dev && slots_dev && forest_dev && roots_dev && updated_levels_dev && new_vectors_dev && grouped_out_dev && slots_out_dev &&
              offsets_out_dev && forest_out_dev && roots_out_dev,
          "null pointer");
  return ann_index_apply_dev(as_u256(grouped_dev), slots_dev, as_u256(forest_dev), as_u256(roots_dev), cluster_sizes, K, dim, cluster, grow,
                             as_u256(updated_levels_dev), as_u256(new_vectors_dev), indices, db_slots, m, as_u256(grouped_out_dev), slots_out_dev,
                             offsets_out_dev, as_u256(forest_out_dev), as_u256(roots_out_dev));
}

int vdb_ann_index_recentre_dev(const vdb_fr* grouped_dev, const uint32_t* slots_dev, const uint64_t* offsets_dev, const vdb_fr* forest_dev,
                               const vdb_fr* roots_dev, const vdb_fr* centroids_dev, const uint64_t* cluster_sizes, size_t K, size_t dim, size_t cluster,
                               const vdb_fr* updated_levels_dev, const vdb_fr* new_centroid_dev, vdb_fr* grouped_out_dev, uint32_t* slots_out_dev,
                               uint64_t* offsets_out_dev, vdb_fr* forest_out_dev, vdb_fr* roots_out_dev, vdb_fr* centroids_out_dev) {
  VDB_REQUIRE_INIT();
  VDB_ARG(grouped_dev && slots_dev && offsets_dev && forest_dev && roots_dev && centroids_dev && updated_levels_dev && new_centroid_dev && grouped_out_dev &&
              slots_out_dev && offsets_out_dev && forest_out_dev && roots_out_dev && centroids_out_dev,
          "null pointer");
  return ann_index_recentre_dev(as_u256(grouped_dev), slots_dev, offsets_dev, as_u256(forest_dev), as_u256(roots_dev), as_u256(centroids_dev), cluster_sizes, K,
                                dim, cluster, as_u256(updated_levels_dev), as_u256(new_centroid_dev), as_u256(grouped_out_dev), slots_out_dev, offsets_out_dev,
                                as_u256(forest_out_dev), as_u256(roots_out_dev), as_u256(centroids_out_dev));
}

int vdb_ann_index_db_tree_dev(const vdb_fr* forest_dev, const uint64_t* cluster_sizes, const uint32_t* slots_dev, size_t K, size_t n, vdb_fr* levels_out_dev) {
  VDB_REQUIRE_INIT();
  VDB_ARG(forest_dev && slots_dev && levels_out_dev, "null pointer");
  return ann_index_db_tree_dev(as_u256(forest_dev), cluster_sizes, slots_dev, K, n, as_u256(levels_out_dev));
}

int vdb_ann_index_remove_size(const uint64_t* cluster_sizes, size_t K, size_t cluster, const uint64_t* slots, size_t m, unsigned* shrink, uint64_t* digests,
                              uint64_t* segment_offsets) {
  AnndPlan dp;
  AnndRemovePlan p;
  TRY(ann_remove_plan(cluster_sizes, K, 1, cluster, slots, m, &dp, &p));
  if (shrink) *shrink = dp.shrink;
  if (digests) *digests = p.seg_off[K + 1];
  if (segment_offsets) memcpy(segment_offsets, p.seg_off.data(), (K + 2) * sizeof(uint64_t));
  return VDB_OK;
}
int vdb_ann_index_remove_dev(const vdb_fr* grouped_dev, const vdb_fr* forest_dev, const vdb_fr* roots_dev, const uint64_t* cluster_sizes, size_t K, size_t dim,
                             size_t cluster, const vdb_fr* updated_levels_dev, const uint64_t* slots, size_t m, vdb_fr* grouped_out_dev,
                             uint32_t* slots_out_dev, uint64_t* offsets_out_dev, vdb_fr* forest_out_dev, vdb_fr* roots_out_dev) {
  VDB_REQUIRE_INIT();
  VDB_ARG(grouped_dev && forest_dev && roots_dev && updated_levels_dev && grouped_out_dev && slots_out_dev && offsets_out_dev && forest_out_dev &&
              roots_out_dev,
          "null pointer");
  return ann_index_remove_dev(as_u256(grouped_dev), as_u256(forest_dev), as_u256(roots_dev), cluster_sizes, K, dim, cluster, as_u256(updated_levels_dev),
                              slots, m, as_u256(grouped_out_dev), slots_out_dev, offsets_out_dev, as_u256(forest_out_dev), as_u256(roots_out_dev));
}

int vdb_ann_index_move_size(const uint64_t* cluster_sizes, size_t K, size_t src, size_t dst, const uint64_t* slots, size_t m, unsigned* shrink, unsigned* grow,
                            uint64_t* digests, uint64_t* segment_offsets) {
  AnnMovePlan mp;
  AnnMoveIndexPlan p;
  TRY(ann_move_plan(cluster_sizes, K, 1, src, dst, -1, slots, m, &mp, &p));
  if (shrink) *shrink = mp.d.shrink;
  if (grow) *grow = mp.grow;
  if (digests) *digests = p.seg_off[K + 1];
  if (segment_offsets) memcpy(segment_offsets, p.seg_off.data(), (K + 2) * sizeof(uint64_t));
  return VDB_OK;
}
int vdb_ann_index_move_dev(const vdb_fr* grouped_dev, const uint32_t* slots_dev, const vdb_fr* forest_dev, const vdb_fr* roots_dev, const uint64_t* cluster_sizes,
                           size_t K, size_t dim, size_t src, size_t dst, unsigned grow, const vdb_fr* updated_src_dev, const vdb_fr* updated_dst_dev,
                           const uint64_t* slots, size_t m, vdb_fr* grouped_out_dev, uint32_t* slots_out_dev, uint64_t* offsets_out_dev, vdb_fr* forest_out_dev,
                           vdb_fr* roots_out_dev) {
  VDB_REQUIRE_INIT();
  VDB_ARG(grouped_dev && slots_dev && forest_dev && roots_dev && updated_src_dev && updated_dst_dev && grouped_out_dev && slots_out_dev && offsets_out_dev &&
              forest_out_dev && roots_out_dev,
          "null pointer");
  return ann_index_move_dev(as_u256(grouped_dev), slots_dev, as_u256(forest_dev), as_u256(roots_dev), cluster_sizes, K, dim, src, dst, grow,
                            as_u256(updated_src_dev), as_u256(updated_dst_dev), slots, m, as_u256(grouped_out_dev), slots_out_dev, offsets_out_dev,
                            as_u256(forest_out_dev), as_u256(roots_out_dev));
}

int vdb_ann_index_write_size(const uint64_t* cluster_sizes, size_t K, size_t cluster, const uint64_t* indices, size_t m, uint64_t* appends, unsigned* grow_c,
                             unsigned* grow_db, uint64_t* digests, uint64_t* segment_offsets, uint64_t* db_digests) {
  AnnuApplyPlan p;
  VDB_ARG(cluster_sizes && indices, "null pointer");
  VDB_ARG(K > 0 && K <= VDB_ANN_MAX_CLUSTERS && cluster < K, "K = 0, K above VDB_ANN_MAX_CLUSTERS or cluster >= K");
  VDB_ARG(cluster_sizes[cluster] > 0 && cluster_sizes[cluster] <= VDB_ANN_MAX_VECTORS && m > 0 && m <= MKU_MAX_UPDATES,
          "empty cluster, cluster too large or a batch outside 1 .. VDB_MERKLE_UPDATE_MAX_UPDATES");
  // g_c: the smallest number of doublings after which the cluster's tree holds its appends
  uint64_t lp, glp, app = 0, glp_db;
  uint32_t d, gd;
  unsigned g_db;
  VDB_ARG(annu_track_fill(indices, m, cluster_sizes[cluster], ~(uint64_t)0, &app, nullptr) == 0, "a write above the cluster's fill at its turn");
  tree_shape(cluster_sizes[cluster], &lp, &d);
  tree_shape(cluster_sizes[cluster] + app, &glp, &gd);
  TRY(ann_write_plan(cluster_sizes, K, 1, cluster, gd - d, -1, indices, m, &p, &glp_db, &g_db));
  if (appends) *appends = p.appends;
  if (grow_c) *grow_c = gd - d;
  if (grow_db) *grow_db = g_db;
  if (digests) *digests = p.seg_off[K + 1];
  if (segment_offsets) memcpy(segment_offsets, p.seg_off.data(), (K + 2) * sizeof(uint64_t));
  if (db_digests) *db_digests = 2 * glp_db;
  return VDB_OK;
}
int vdb_ann_index_write_dev(const vdb_fr* grouped_dev, const uint32_t* slots_dev, const vdb_fr* forest_dev, const vdb_fr* roots_dev,
                            const uint64_t* cluster_sizes, size_t K, size_t dim, size_t cluster, unsigned grow_c, unsigned grow_db,
                            const vdb_fr* updated_levels_dev, const vdb_fr* updated_db_levels_dev, const vdb_fr* new_vectors_dev, const uint64_t* indices,
                            size_t m, vdb_fr* grouped_out_dev, uint32_t* slots_out_dev, uint64_t* offsets_out_dev, vdb_fr* forest_out_dev,
                            vdb_fr* roots_out_dev, vdb_fr* db_tree_out_dev) {
  VDB_REQUIRE_INIT();
  VDB_ARG(grouped_dev && slots_dev && forest_dev && roots_dev && updated_levels_dev && updated_db_levels_dev && new_vectors_dev && grouped_out_dev &&
              slots_out_dev && offsets_out_dev && forest_out_dev && roots_out_dev && db_tree_out_dev,
          "null pointer");
  return ann_index_write_dev(as_u256(grouped_dev), slots_dev, as_u256(forest_dev), as_u256(roots_dev), cluster_sizes, K, dim, cluster, grow_c, grow_db,
                             as_u256(updated_levels_dev), as_u256(updated_db_levels_dev), as_u256(new_vectors_dev), indices, m, as_u256(grouped_out_dev),
                             slots_out_dev, offsets_out_dev, as_u256(forest_out_dev), as_u256(roots_out_dev), as_u256(db_tree_out_dev));
}

}  // extern "C"
