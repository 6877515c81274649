// The committed database as it lies on the device (resident.hip): the Poseidon Merkle tree over the vectors and the index of the
// approximate-nearest-neighbour queries, values only.  What the builders and the witness side (witness.hip, which traces the same tree
// cell by cell) both need is stated here once: the `levels` layout, the shape of a leaf's sponge and of the tree, the batch limit.
#pragma once
#include "ann_update_host.hpp"   // tree_shape: the padded leaf count and the depth of the tree over n leaves
#include "common.hpp"
#include "poseidon.hpp"

namespace vdb {

// The `levels` layout of a tree over lp (padded) leaves: level 0 = the lp leaf digests, then the levels one after the other
// (lp + lp / 2 + ... + 1 of the 2 lp entries, the last unused); level l starts at mku_level_off(lp, l), the root is entry 2 lp - 2
HD uint64_t mku_level_off(uint64_t lp, uint32_t l) { return 2 * (lp - (lp >> l)); }
// words that permutation p of the sponge over a leaf of D words absorbs
HD int leaf_absorbs(size_t D, uint32_t p) { return 2 * (size_t)p < D ? (int)(D - 2 * (size_t)p < 2 ? D - 2 * (size_t)p : 2) : 0; }
// updates in one batch, against the tree and against the index alike (include/vdb.h VDB_MERKLE_UPDATE_MAX_UPDATES)
#define MKU_MAX_UPDATES 4096

// the value part of merkle_commitment's layout over n vectors of `dim` words: the permutations of a leaf's sponge, the depth and the
// padded leaf count of the tree (the cell counts are the witness side's: MkLayout, witness.hip)
struct MkShape {
  uint32_t nperm, depth;
  uint64_t n_leaves_pow2;
};
static inline void mk_shape(size_t n, size_t dim, MkShape* o) {
  o->nperm = (uint32_t)((dim + 1) / 2 + (dim % 2 == 0 ? 1 : 0));
  tree_shape(n, &o->n_leaves_pow2, &o->depth);
}

// k_mk_leaf_states (the kernel's own arguments) on max(1, ceil(n / 64)) blocks of 64: a call's launch list does not depend on n
int mk_leaf_states(const PoseidonSpec* sp, const u256* vectors, uint32_t n, uint32_t D, uint32_t nperm, u256* states, u256* leaves,
                   const uint32_t* leaf_at);
int mk_tree_values(const PoseidonSpec* sp, const u256* vectors, size_t n, size_t dim, const MkShape& ml, u256* states, u256* levels,
                   uint64_t* root_off);
int mk_levels_from_leaves(const PoseidonSpec* sp, u256* levels, uint64_t lp, uint64_t* root_off);
int merkle_tree_build_dev(const u256* vectors, size_t n, size_t dim, u256* levels);
int merkle_tree_grow_dev(const u256* levels, size_t n, unsigned grow, u256* grown);
int ann_index_build_dev(const u256* db, const uint32_t* ids, const u256* centroids, size_t n, size_t K, size_t dim, u256* grouped, uint32_t* slots,
                        uint64_t* offsets, u256* forest, u256* roots);
int ann_index_apply_dev(const u256* grouped, const uint32_t* slots, const u256* forest, const u256* roots, const uint64_t* sizes, size_t K, size_t dim,
                        size_t cluster, unsigned grow, const u256* updated, const u256* new_vectors, const uint64_t* indices, const uint32_t* db_slots,
                        size_t m, u256* grouped_out, uint32_t* slots_out, uint64_t* offsets_out, u256* forest_out, u256* roots_out);
int ann_index_remove_dev(const u256* grouped, const u256* forest, const u256* roots, const uint64_t* sizes, size_t K, size_t dim, size_t cluster,
                         const u256* updated, const uint64_t* slots, size_t m, u256* grouped_out, uint32_t* slots_out, uint64_t* offsets_out,
                         u256* forest_out, u256* roots_out);
int ann_index_move_dev(const u256* grouped, const uint32_t* slots_in, const u256* forest, const u256* roots, const uint64_t* sizes, size_t K, size_t dim, size_t a,
                       size_t b, unsigned grow, const u256* updated_a, const u256* updated_b, const uint64_t* slots, size_t m, u256* grouped_out,
                       uint32_t* slots_out, uint64_t* offsets_out, u256* forest_out, u256* roots_out);
int ann_index_write_dev(const u256* grouped, const uint32_t* slots, const u256* forest, const u256* roots, const uint64_t* sizes, size_t K, size_t dim,
                        size_t cluster, unsigned grow_c, unsigned grow_db, const u256* updated_c, const u256* updated_db, const u256* new_vectors,
                        const uint64_t* indices, size_t m, u256* grouped_out, uint32_t* slots_out, uint64_t* offsets_out, u256* forest_out, u256* roots_out,
                        u256* db_tree_out);
int ann_index_db_tree_dev(const u256* forest, const uint64_t* sizes, const uint32_t* slots, size_t K, size_t n, u256* levels_out);

}  // namespace vdb
