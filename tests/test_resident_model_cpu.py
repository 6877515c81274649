"""tests/resident_model.py held to the cell-level models, which tests/test_ann_update_cpu.py and tests/test_ann_delete_cpu.py hold to the
oracle: the `updated_levels` the helpers hand to vdb_ann_index_apply_dev / _remove_dev are the trees that the path updates of
ann_update_model.update_model and ann_delete_model.path_ops_model leave behind, one update after the other; the expected index is the index
model over the updated or compacted database; and the tree of that index is the grown, or the cut, `updated_levels`."""
import numpy as np
import pytest

import ann_delete_model as AD
import ann_model as AN
import ann_update_model as AU
import merkle_ops_model as MO
import merkle_update_model as MU
import resident_model as RM
import test_ann_update_cpu as TU
from test_merkle_update_cpu import database

DIM = 3


def cut_levels(levels, lp, lp_new):
    """the tree `levels` over lp leaves cut to its first lp_new: level l keeps its first lp_new >> l digests"""
    rows, l = [], 0
    while lp_new >> l:
        off = 2 * (lp - (lp >> l))
        rows.append(levels[off:off + (lp_new >> l)])
        l += 1
    return np.concatenate(rows + [np.zeros((1, 4), dtype=np.uint64)])


def _delete_case(O, sizes, c, slots, seed=60):
    ids = AD.ids_of(sizes)
    K = len(sizes)
    db, cent = database(O, len(ids), DIM, seed), database(O, K, DIM, seed + 1)
    tree = MU.build_tree(O, AN.select_cluster(db, ids, c)[0])
    AD.path_ops_model(O, tree, slots)
    ix2, updated, shrink, db2, ids2 = RM.removed_model(O, db, ids, cent, c, slots)
    assert np.array_equal(updated, MU.flat_levels(tree)), "the tree the path updates leave"
    lp = MU.padded(sizes[c])[0]
    assert shrink == AD.shrink_of(sizes[c], len(slots)) and updated.shape[0] == 2 * lp
    assert np.array_equal(ix2["forest"][c], cut_levels(updated, lp, lp >> shrink)), "the fresh build's segment is the cut tree"
    assert np.array_equal(ix2["roots"][1 + c], updated[2 * (lp - (lp >> (MU.padded(sizes[c])[1] - shrink)))])
    want_db, want_ids = AD.compacted_database(db, ids, c, slots)
    assert np.array_equal(db2, want_db) and np.array_equal(ids2, want_ids)
    assert np.array_equal(ix2["slots"], np.arange(len(ids) - len(slots), dtype=np.uint32)), "a compacted database is its own grouping"
    return RM.remove_facts(list(sizes), c, DIM, slots)


@pytest.mark.parametrize("name", sorted(AD.SHAPES))
def test_removed_models_tree_is_what_the_path_updates_leave(O, name):
    _delete_case(O, *AD.SHAPES[name])


def test_removed_model_on_a_larger_cluster_with_repeated_slots_and_the_last_slot(O):
    """n_c = 37 of a 64-leaf tree: the last slot first (nothing moves), a slot deleted twice in a row, a slot whose carried leaf is
    itself a moved one, eight deletes in all: the tree halves once and survivors are not where they started"""
    facts = _delete_case(O, (3, 37, 2), 1, [36, 0, 0, 5, 5, 30, 12, 28])
    assert facts["shrink"] == 1 and facts["moved"] >= 4 and facts["delta"] == 64


@pytest.mark.parametrize("n_c", [5, 9])
def test_removed_model_at_the_sizes_next_to_a_power_of_two(O, n_c):
    facts = _delete_case(O, (2, n_c), 1, [n_c - 1, 0])
    assert facts["shrink"] == 1


@pytest.mark.parametrize("name", sorted(TU.CASES))
def test_applied_models_tree_is_what_the_path_updates_leave(O, name):
    ids, c, slots, grow = TU.CASES[name]
    m, db, ids, cent, new, ix, tree = TU.case(O, name)
    ix2, updated, g, db2, ids2 = RM.applied_model(O, db, ids, cent, c, slots, new)
    assert g == grow and np.array_equal(updated, MU.flat_levels(tree)), "the tree the path updates leave"
    assert np.array_equal(updated, ix2["forest"][c]) and np.array_equal(ix2["roots"][-1], m["public"][-1])
    small = ix["forest"][c]
    lp = small.shape[0] // 2
    assert np.array_equal(RM.tree_over_leaves(O, small[:lp], lp << grow), MU.flat_levels(MO.grow_tree(O, MU.build_tree(O, AN.select_cluster(db, ids, c)[0]), grow)))


def test_applied_model_on_a_batch_that_crosses_a_power_of_two(O):
    """n_c = 14 of a 16-leaf tree: a slot written twice, the padding filled, two appends past 16 (one doubling), and a replacement of a
    row appended by the same batch"""
    sizes, c, slots = (2, 14, 3), 1, [3, 14, 15, 3, 16, 13, 17, 16]
    ids = AD.ids_of(sizes)
    K = len(sizes)
    db, cent, new = database(O, len(ids), DIM, 70), database(O, K, DIM, 71), database(O, len(slots), DIM, 72)
    ix = AN.index_model(O, db, ids, cent)
    ix2, updated, grow, db2, ids2 = RM.applied_model(O, db, ids, cent, c, slots, new)
    facts = RM.apply_facts(list(sizes), c, DIM, slots)
    assert grow == 1 and (facts["appends"], facts["grow"], facts["delta"]) == (4, 1, 32)
    tree = MO.grow_tree(O, MU.build_tree(O, AN.select_cluster(db, ids, c)[0]), grow)
    m = AU.update_model(O, ix["roots"][:K + 1], c, tree, slots, new, grow)
    assert np.array_equal(updated, MU.flat_levels(tree)) and np.array_equal(updated, ix2["forest"][c])
    assert np.array_equal(ix2["roots"][-1], m["public"][-1]) and np.array_equal(ix2["roots"][1 + c], m["new_cluster_root"])
    assert np.array_equal(ix2["slots"][2:20], np.concatenate([np.arange(2, 16), np.arange(19, 23)])), "the appends' rows follow the cluster's"
    assert np.array_equal(ix2["grouped"][2 + 3], new[3]) and np.array_equal(ix2["grouped"][2 + 16], new[7]), "the last write to a slot wins"


def test_tree_over_leaves_is_the_fresh_build_and_the_grown_tree(O):
    for n, grow in ((1, 0), (1, 3), (5, 0), (6, 2), (8, 1)):
        db = database(O, n, DIM, 80 + n)
        tree = MU.build_tree(O, db)
        small = MU.flat_levels(tree)
        lp = MU.padded(n)[0]
        assert np.array_equal(RM.tree_over_leaves(O, O.poseidon_hash_many(db), lp), small)
        assert np.array_equal(RM.tree_over_leaves(O, small[:lp], lp << grow), MU.flat_levels(MO.grow_tree(O, tree, grow))), (n, grow)


def test_launch_facts_restate_the_forest_plan():
    """the host restatement of resident.hip's launch shapes against the library's own plan (vdb_ann_index_forest_size needs no device)"""
    import ctypes
    from halo2_vectordb_amd import _lib
    lib = _lib.load()
    ids = np.ascontiguousarray([0] * 9 + [1] + [2] * 70 + [3, 3], dtype=np.uint32)
    f = RM.launch_facts(ids, 4, 5)
    dig, seg = ctypes.c_uint64(), np.zeros(6, dtype=np.uint64)
    assert lib.vdb_ann_index_forest_size(ids.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(82), ctypes.c_size_t(4), ctypes.byref(dig),
                                         seg.ctypes.data_as(ctypes.c_void_p)) == 0
    assert f["seg_lp"] == [16, 1, 128, 2, 4] and dig.value == f["digests"] == 302 and seg.tolist() == [0, 32, 34, 290, 294, 302]
    assert (f["tiles"], f["last_tile_live"], f["depth"], f["level_nodes"][:3], f["nodeless"], f["nodeless_run"], f["nodeless_lead"]) == (2, 18, 7, [75, 37, 18], 1, 1, 0)
    assert (f["nperm"], f["last_absorb"], f["roots_blocks"], f["roots_last_live"], f["gather_blocks"]) == (3, 1, 1, 5, 2)
    assert RM.launch_facts(ids, 4, 4)["nperm"] == 3 and RM.launch_facts(ids, 4, 4)["last_absorb"] == 2
