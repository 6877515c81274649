"""The index update circuit without a GPU (circuit_sym.trace_ann_update / build_ann_update; tests/ann_update_model.py): the model's new index
root is the index model's over the updated database, the traced and the built map agree, and the single-cell alteration sweep leaves one
kind of cell free: the inverse witness of the is_zero whose operand is zero (indicator c's)."""
import ctypes

import numpy as np
import pytest

import alteration_model as AM
import ann_model as AN
import ann_update_model as AU
import merkle_ops_model as MO
import merkle_update_model as MU
import topk_model as TM
from halo2_vectordb_amd import circuit_sym as CS
from test_alteration_cpu import both_forms
from test_batch_query_cpu import same_map
from test_merkle_update_cpu import database, fetchers

DIM = 3
# name: (ids, c, slots written, grow)
CASES = {
    "replacement": ([0, 1, 1, 2, 2, 2], 2, [1], 0),
    "append_into_padding": ([0, 1, 1, 2, 2, 2], 2, [3], 0),
    "append_needs_grow": ([0, 1, 1, 2, 2, 2], 1, [2], 1),
    "one_member_cluster": ([0, 1, 1, 2, 2, 2], 0, [1], 1),
    "two_writes_to_one_slot": ([0, 1, 1, 2, 2, 2], 2, [0, 3, 0], 0),
    "replace_append_append_grow": ([0, 0, 1, 2, 2, 2], 0, [0, 2, 3], 1),
}


def case(O, name, seed=5):
    """-> (model, db, ids, centroids, new vectors, the index model before the batch, the cluster's tree after it)"""
    ids, c, slots, grow = CASES[name]
    ids = np.asarray(ids)
    K = int(ids.max()) + 1
    db, cent, new = database(O, len(ids), DIM, seed), database(O, K, DIM, seed + 1), database(O, len(slots), DIM, seed + 2)
    ix = AN.index_model(O, db, ids, cent)
    tree = MO.grow_tree(O, MU.build_tree(O, AN.select_cluster(db, ids, c)[0]), grow)
    m = AU.update_model(O, ix["roots"][:K + 1], c, tree, slots, new, grow)
    return m, db, ids, cent, new, ix, tree


@pytest.mark.parametrize("name", sorted(CASES))
def test_new_index_root_is_the_index_models_over_the_updated_database(O, name):
    ids, c, slots, grow = CASES[name]
    m, db, ids, cent, new, ix, tree = case(O, name)
    K = cent.shape[0]
    assert grow == AU.smallest_grow(int((ids == c).sum()), AU.track_fill(slots, int((ids == c).sum())))
    db2, ids2 = AU.updated_database(db, ids, c, slots, new)
    ix2 = AN.index_model(O, db2, ids2, cent)
    assert np.array_equal(m["public"][0], ix["roots"][-1]) and np.array_equal(m["public"][-1], ix2["roots"][-1])
    assert np.array_equal(m["new_cluster_root"], ix2["roots"][1 + c])
    assert TM.to_ints(m["public"][1:2]) == [c] and m["public"].shape[0] == 3 * len(slots) + 3
    assert np.array_equal(MU.flat_levels(tree), ix2["forest"][c]), "the tree the batch leaves is the fresh build's segment"
    assert TM.to_limbs(m["outs"]).tobytes() == ix2["roots"][1:1 + K].tobytes()
    lay = CS.ann_update_layout(K, len(slots), DIM, len(tree) - 1, grow)
    assert m["advice"].shape[0] == lay["total"] and all(m["regions"][k] == lay[k] for k in m["regions"])


def test_a_write_above_the_fill_is_refused_by_the_model():
    with pytest.raises(AssertionError):
        AU.track_fill([4], 3)
    assert AU.track_fill([3, 4, 0], 3) == 2


@pytest.mark.parametrize("K,c", [(1, 0), (3, 0), (3, 2)])
@pytest.mark.parametrize("grow", [0, 1])
def test_traced_and_built_maps_agree_and_only_the_zero_operands_inverse_is_free(O, K, c, grow):
    ids = np.asarray([0, 0, 0] if K == 1 else [0, 0, 1, 2, 2, 2][: 6])
    n_c = int((ids == c).sum())
    slots = [0, n_c] if grow == 0 and MU.padded(n_c)[0] > n_c else ([0] if grow == 0 else [n_c - 1, n_c])
    if grow and MU.padded(n_c)[0] > n_c:
        slots = [n_c, n_c + 1]                               # fill the padding, then the append that needs the doubling
    db, cent, new = database(O, len(ids), DIM, 9), database(O, K, DIM, 10), database(O, len(slots), DIM, 11)
    ix = AN.index_model(O, db, ids, cent)
    tree = MO.grow_tree(O, MU.build_tree(O, AN.select_cluster(db, ids, c)[0]), grow)
    m = AU.update_model(O, ix["roots"][:K + 1], c, tree, slots, new, grow)
    depth, k = len(tree) - 1, len(slots)
    ff, fv, vals = fetchers(m)
    traced = CS.trace_ann_update(K, k, DIM, depth, ff, fv, grow=grow)
    built = CS.build_ann_update(K, k, DIM, depth, ff, fv, grow=grow)
    same_map(traced[0], built[0])
    assert traced[1] == built[1] and len(built[1]) == 3 * k + 3 and traced[2] == built[2]
    bm, bpub, info = built
    assert bm.n_cells == m["advice"].shape[0]
    rep = bm.check_witness(vals, [], flags=m["flags"])
    assert not any(rep.values()), rep
    assert [vals[x] for x in bpub] == TM.to_ints(m["public"])
    assert [vals[x] for x in info["indicators"]] == m["indicators"] and vals[info["picked"]] == m["picked"]
    assert [vals[x] for x in info["outs"]] == m["outs"] and bm.copy_of[info["old_root"]] == info["picked"]
    # the sweep: (a) .. (d) of test_alteration_cpu on both forms; one free cell, indicator c's inverse witness
    both_forms(f"ann update K {K} c {c} grow {grow}", (traced[0], traced[1]), (built[0], built[1]), vals, [], 8, m["flags"])
    free = AM.unnoticed(bm, vals, np.asarray([], dtype=object), [int(x) for x in bpub])
    lay = info["layout"]
    inv_c = lay["indicator"] + (8 + 12 * (c - 1) + 4 if c else 0) + 2
    assert free == [inv_c] and AM.explain(bm, vals, inv_c) == AM.IS_ZERO_INVERSE
    # tampering is noticed: a cluster root, the centroids' root, an indicator, an out_j, the update block's old root
    inst = [vals[x] for x in bpub]
    for cell in (lay["roots"] + c, lay["centroids_root"], info["indicators"][c], info["outs"][K - 1], info["old_root"], lay["c"]):
        alt = vals.copy()
        alt[cell] = (alt[cell] + 1) % CS.R
        assert AM.violations(AM.recount(bm, alt, np.asarray([], dtype=object), 8, [int(x) for x in bpub], inst)) >= 1, cell


def test_build_merkle_update_is_place_merkle_update_at_base_zero(O):
    """the plain update map is unchanged by being expressed through place_merkle_update"""
    from test_merkle_ops_cpu import kernel_like_flags, ops_case
    m, tree, _ = ops_case(O, 3, 3, [9, 2, 15], [0, 1, 1], 2)
    m["flags"] = kernel_like_flags(m)
    ff, fv, vals = fetchers(m)
    traced = CS.trace_merkle_update(3, 3, len(tree) - 1, ff, fv, kinds=[0, 1, 1], grow=2)
    built = CS.build_merkle_update(3, 3, len(tree) - 1, ff, fv, kinds=[0, 1, 1], grow=2)
    same_map(traced[0], built[0])
    assert traced[1] == built[1]


def test_layout_refuses_an_index_without_clusters():
    with pytest.raises(ValueError):
        CS.ann_update_layout(0, 1, 3, 2)


def test_library_exports_the_index_update_entry_points():
    from halo2_vectordb_amd import _lib
    lib = _lib.load()
    for name in ("vdb_wit_ann_update_size", "vdb_wit_ann_update", "vdb_wit_ann_update_dev", "vdb_ann_index_apply_size", "vdb_ann_index_apply_dev"):
        assert hasattr(lib, name), name
    cells, n_in, ub = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
    # the size call needs no device; it is circuit_sym's layout
    for K, n_c, dim, m, grow in ((3, 3, 3, 2, 0), (1, 1, 4, 1, 1), (5, 2, 2, 3, 2)):
        assert lib.vdb_wit_ann_update_size(K, n_c, dim, m, grow, ctypes.byref(cells), ctypes.byref(n_in), ctypes.byref(ub)) == 0
        lay = CS.ann_update_layout(K, m, dim, MU.padded(n_c)[1] + grow, grow)
        assert (cells.value, n_in.value, ub.value) == (lay["total"], lay["n_in"], lay["update"])
    for K, n_c, m, grow in ((0, 3, 1, 0), (4097, 3, 1, 0), (3, 1, 1, 0), (3, 3, 0, 0)):
        assert lib.vdb_wit_ann_update_size(K, n_c, 3, m, grow, ctypes.byref(cells), ctypes.byref(n_in), ctypes.byref(ub)) == -3
    # the apply plan: appends, digests and segment offsets of the next index, and its refusals
    sizes = np.asarray([2, 1, 3], dtype=np.uint64)
    app, dig, seg = ctypes.c_uint64(), ctypes.c_uint64(), np.zeros(5, dtype=np.uint64)
    idx = np.asarray([0, 2, 3], dtype=np.uint64)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    assert lib.vdb_ann_index_apply_size(p(sizes), 3, 0, 1, p(idx), 3, ctypes.byref(app), ctypes.byref(dig), p(seg)) == 0
    assert app.value == 2 and seg.tolist() == [0, 8, 10, 18, 26] and dig.value == 26
    assert lib.vdb_ann_index_apply_size(p(sizes), 3, 0, 0, p(idx), 3, None, None, None) == -3       # the appends need one doubling
    assert lib.vdb_ann_index_apply_size(p(sizes), 3, 0, 2, p(idx), 3, None, None, None) == -3       # ... and not two
    hole = np.asarray([3], dtype=np.uint64)
    assert lib.vdb_ann_index_apply_size(p(sizes), 3, 0, 1, p(hole), 1, None, None, None) == -3      # a hole
    assert lib.vdb_ann_index_apply_size(p(sizes), 3, 3, 0, p(idx), 3, None, None, None) == -3       # c >= K
