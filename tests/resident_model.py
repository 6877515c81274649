"""The values-only layer of the committed database (resident.hip: vdb_merkle_tree_build_dev / _grow_dev, vdb_ann_index_build_dev / _apply_dev /
_remove_dev) as a model on whole arrays, for shapes far beyond what the cell-level models can trace: small helpers on top of
ann_model.index_model, merkle_update_model.build_tree / flat_levels, ann_update_model.updated_database / smallest_grow / track_fill and
ann_delete_model.simulate / compacted_database / shrink_of.  tests/test_resident_model_cpu.py holds them to those cell-level models.
Nothing here knows a launch shape, an offset table or a move table of the GPU side; launch_facts and the two *_facts functions restate
resident.hip's launch formulas only so that a test can assert, on the host, that its shape reaches the code it is there for."""
import numpy as np

import ann_delete_model as AD
import ann_model as AN
import ann_update_model as AU
import merkle_update_model as MU

MAX_UPDATES = 4096            # include/vdb.h VDB_MERKLE_UPDATE_MAX_UPDATES
MAX_CLUSTERS = 4096           # include/vdb.h VDB_ANN_MAX_CLUSTERS


def tree_over_leaves(O, leaf_digests, lp):
    """the tree in the device layout (2 lp, 4) over lp leaves, the first of them `leaf_digests`, the trailing slots 0: every level is
    O.poseidon_hash_many over the pairs of the level below"""
    leaf_digests = np.asarray(leaf_digests, dtype=np.uint64).reshape(-1, 4)
    assert lp >= 1 and lp & (lp - 1) == 0 and leaf_digests.shape[0] <= lp
    level = np.zeros((lp, 4), dtype=np.uint64)
    level[:leaf_digests.shape[0]] = leaf_digests
    levels = [level]
    while levels[-1].shape[0] > 1:
        levels.append(O.poseidon_hash_many(levels[-1].reshape(-1, 2, 4)))
    return np.concatenate(levels + [np.zeros((1, 4), dtype=np.uint64)])


def segments_of(forest):
    """the K + 2 digest offsets at which the trees of index_model's forest start"""
    return np.concatenate([[0], np.cumsum([t.shape[0] for t in forest])]).astype(np.uint64)


def as_index(ix):
    """index_model's dict in the form of api.ann_index_build's: the forest one array, and its segment offsets"""
    return dict(ix, forest=np.concatenate(ix["forest"]), segments=segments_of(ix["forest"]))


def applied_model(O, db, ids, cent, c, indices, new_vectors):
    """the batch of writes into cluster c -> (the index model over the updated database, the cluster's tree after the batch: the
    `updated_levels` of vdb_ann_index_apply_dev, the smallest number of doublings, the updated database and its ids)"""
    n_c = int((np.asarray(ids) == c).sum())
    grow = AU.smallest_grow(n_c, AU.track_fill(indices, n_c))
    db2, ids2 = AU.updated_database(db, ids, c, indices, new_vectors)
    members, _ = AN.select_cluster(db2, ids2, c)
    updated = tree_over_leaves(O, O.poseidon_hash_many(members), MU.padded(n_c)[0] << grow)
    return AN.index_model(O, db2, ids2, cent), updated, grow, db2, ids2


def removed_model(O, db, ids, cent, c, slots):
    """the batch of deletes from cluster c -> (the index model over the compacted database, the cluster's tree after the batch at its
    old size: the `updated_levels` of vdb_ann_index_remove_dev, the number of halvings, the compacted database and its ids)"""
    old, _ = AN.select_cluster(db, ids, c)
    n_c = old.shape[0]
    survivors, _ = AD.simulate(n_c, slots)
    updated = tree_over_leaves(O, O.poseidon_hash_many(old)[survivors], MU.padded(n_c)[0])
    db2, ids2 = AD.compacted_database(db, ids, c, slots)
    return AN.index_model(O, db2, ids2, cent), updated, AD.shrink_of(n_c, len(slots)), db2, ids2


# ------------------------------------------------------------------------------------------------ what a shape reaches (resident.hip's launches)
def _blocks(lanes, width):
    return (lanes + width - 1) // width


def launch_facts(ids, K, dim):
    """vdb_ann_index_build_dev over these ids: the 64-row tiles of k_ann_group and the live lanes of the last, the segments' padded leaf
    counts, the blocks of every launch, the segments with no node at level 0 and the longest run of them"""
    ids = np.asarray(ids)
    n = ids.shape[0]
    sizes = np.bincount(ids, minlength=K).tolist()
    lp = [MU.padded(s)[0] for s in sizes + [K]]
    depth = max(MU.padded(s)[1] for s in sizes + [K])
    level_nodes = [sum(x >> (l + 1) for x in lp) for l in range(depth)]
    nodeless = [x == 1 for x in lp]
    run = best = 0
    for x in nodeless:
        run = run + 1 if x else 0
        best = max(best, run)
    lead = next((i for i, x in enumerate(nodeless) if not x), len(nodeless))
    return dict(tiles=_blocks(n, 64), last_tile_live=n - 64 * (_blocks(n, 64) - 1), sizes=sizes, seg_lp=lp, depth=depth, segments=K + 1,
                cluster_depth=max(MU.padded(s)[1] for s in sizes), centroid_depth=MU.padded(K)[1], level_nodes=level_nodes,
                level_blocks=[_blocks(x, 64) for x in level_nodes], nodeless=sum(nodeless), nodeless_run=best, nodeless_lead=lead,
                leaf_blocks=max(1, _blocks(n, 64)), gather_blocks=_blocks(n * dim, 256), roots_blocks=K // 64 + 1,
                roots_last_live=K + 1 - 64 * (K // 64), digests=2 * sum(lp), nperm=(dim + 1) // 2 + (dim % 2 == 0),
                last_absorb=dim - 2 * ((dim - 1) // 2))


def apply_facts(sizes, c, dim, indices):
    """vdb_ann_index_apply_dev: appends, doublings, the digests by which the segments behind c move, the blocks of its three launches"""
    K, n_c = len(sizes), sizes[c]
    appends = AU.track_fill(indices, n_c)
    grow = AU.smallest_grow(n_c, appends)
    lp = [MU.padded(s)[0] for s in list(sizes) + [K]]
    delta = 2 * ((lp[c] << grow) - lp[c])
    n_new = sum(sizes) + appends
    return dict(appends=appends, grow=grow, delta=delta, rows_blocks=_blocks(n_new * dim + n_new, 256), forest_blocks=_blocks(2 * sum(lp) + delta, 256),
                roots_blocks=K // 64 + 1, digests=2 * sum(lp) + delta)


def remove_facts(sizes, c, dim, slots):
    """vdb_ann_index_remove_dev: halvings, the survivors that are not the original member of their place (the move table), the digests
    by which the segments behind c move, the blocks of its three launches"""
    K, n_c, m = len(sizes), sizes[c], len(slots)
    survivors, _ = AD.simulate(n_c, slots)
    lp = [MU.padded(s)[0] for s in list(sizes) + [K]]
    shrink = AD.shrink_of(n_c, m)
    delta = 2 * (lp[c] - (lp[c] >> shrink))
    n_new = sum(sizes) - m
    return dict(shrink=shrink, moved=sum(int(s != p) for p, s in enumerate(survivors)), delta=delta, rows_blocks=_blocks(n_new * dim + n_new, 256),
                forest_blocks=_blocks(2 * sum(lp) - delta, 256), roots_blocks=K // 64 + 1, digests=2 * sum(lp) - delta)
