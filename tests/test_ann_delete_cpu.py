"""The index delete circuit without a GPU (circuit_sym.trace_ann_delete / build_ann_delete; tests/ann_delete_model.py): the model's new
index root is the index model's over the compacted database, the traced and the built map agree, and the single-cell alteration sweep
leaves one kind of cell free: the inverse witness of the is_zero whose operand is zero (indicator c's).  The carried leaf and S_0 are
plain witness cells, and both are noticed."""
import ctypes

import numpy as np
import pytest

import alteration_model as AM
import ann_delete_model as AD
import ann_model as AN
import merkle_update_model as MU
import topk_model as TM
from halo2_vectordb_amd import circuit_sym as CS
from test_alteration_cpu import both_forms
from test_batch_query_cpu import same_map
from test_merkle_update_cpu import database, fetchers

DIM = 3


def case(O, sizes, c, slots, seed=5):
    """-> (model, db, ids, centroids, the index model before the batch, the cluster's tree after it at its old size)"""
    ids = AD.ids_of(sizes)
    K = len(sizes)
    db, cent = database(O, len(ids), DIM, seed), database(O, K, DIM, seed + 1)
    ix = AN.index_model(O, db, ids, cent)
    tree = MU.build_tree(O, AN.select_cluster(db, ids, c)[0])
    m = AD.delete_model(O, ix["roots"][:K + 1], c, tree, slots)
    return m, db, ids, cent, ix, tree


@pytest.mark.parametrize("name", sorted(AD.SHAPES))
def test_new_index_root_is_the_index_models_over_the_compacted_database(O, name):
    sizes, c, slots = AD.SHAPES[name]
    m, db, ids, cent, ix, tree = case(O, sizes, c, slots)
    K, n_c, k = len(sizes), sizes[c], len(slots)
    db2, ids2 = AD.compacted_database(db, ids, c, slots)
    ix2 = AN.index_model(O, db2, ids2, cent)
    assert np.array_equal(m["public"][0], ix["roots"][-1]) and np.array_equal(m["public"][-1], ix2["roots"][-1])
    assert np.array_equal(m["new_cluster_root"], ix2["roots"][1 + c])
    assert np.array_equal(MU.flat_levels(m["cut_tree"]), ix2["forest"][c]), "the tree the batch leaves, cut, is the fresh build's segment"
    assert m["s"] == {"shrink": 1, "last_repeat": 2, "flat": 0, "to_one": 1, "k1": 1}[name]
    if m["s"]:
        assert np.array_equal(m["shrink_top"], m["update"]["public"][-1]), "S_s is the update block's final root: the dropped half is empty"
    # public: [root_old | c | slot, removed leaf, last, moved leaf | root_new], last_j = n_c - 1 - j, the moved leaf is what sat there
    pub = m["public"]
    assert pub.shape[0] == 4 * k + 3 and TM.to_ints(pub[1:2]) == [c]
    members = list(ix["forest"][c][:n_c])
    for j, s in enumerate(slots):
        assert TM.to_ints(pub[2 + 4 * j: 3 + 4 * j]) == [s] and TM.to_ints(pub[4 + 4 * j: 5 + 4 * j]) == [n_c - 1 - j]
        assert np.array_equal(pub[3 + 4 * j], members[s]) and np.array_equal(pub[5 + 4 * j], members[-1])
        members[s] = members[-1]
        members.pop()
    lay = CS.ann_delete_layout(K, k, DIM, len(tree) - 1, m["s"])
    assert m["advice"].shape[0] == lay["total"] and all(m["regions"][r] == lay[r] for r in m["regions"])
    assert CS.ann_delete_shrink(n_c, k) == (len(tree) - 1, m["s"])


def test_the_model_refuses_emptying_a_cluster_and_a_slot_at_or_above_the_fill():
    for n_c, slots in ((2, [0, 0]), (3, [3]), (3, [0, 2]), (3, [])):
        with pytest.raises(AssertionError):
            AD.simulate(n_c, slots)
    assert AD.simulate(5, [4, 0, 0]) == ([2, 1], [4, 3, 2])
    assert AD.simulate(5, [1]) == ([0, 4, 2, 3], [4])


def _shapes_and_clusters():
    out = []
    for name in sorted(AD.SHAPES):
        sizes, c, slots = AD.SHAPES[name]
        out.append((name, c))
        for other in (0, len(sizes) - 1):
            # the same batch against another cluster of the same size, where the shape has one
            if other != c and sizes[other] == sizes[c]:
                out.append((name, other))
    return out


@pytest.mark.parametrize("name,c", _shapes_and_clusters() + [("flat_c2", 2), ("shrink_c2", 2)])
def test_traced_and_built_maps_agree_and_only_the_zero_operands_inverse_is_free(O, name, c):
    extra = {"flat_c2": ((2, 3, 4), 2, [1]), "shrink_c2": ((2, 3, 5), 2, [1])}      # c = K - 1 at s = 0 and s = 1
    sizes, _, slots = extra[name] if name in extra else AD.SHAPES[name]
    m, db, ids, cent, ix, tree = case(O, sizes, c, slots, seed=9)
    K, depth, k, sh = len(sizes), len(tree) - 1, len(slots), m["s"]
    ff, fv, vals = fetchers(m)
    traced = CS.trace_ann_delete(K, k, DIM, depth, ff, fv, shrink=sh)
    built = CS.build_ann_delete(K, k, DIM, depth, ff, fv, shrink=sh)
    same_map(traced[0], built[0])
    assert traced[1] == built[1] and len(built[1]) == 4 * k + 3
    assert {x: traced[2][x] for x in traced[2] if x != "layout"} == {x: built[2][x] for x in built[2] if x != "layout"}
    bm, bpub, info = built
    assert bm.n_cells == m["advice"].shape[0]
    rep = bm.check_witness(vals, [], flags=m["flags"])
    assert not any(rep.values()), rep
    assert [vals[x] for x in bpub] == TM.to_ints(m["public"])
    assert [vals[x] for x in info["indicators"]] == m["indicators"] and vals[info["picked"]] == m["picked"]
    assert [vals[x] for x in info["outs"]] == m["outs"] and bm.copy_of[info["old_root"]] == info["picked"]
    u = m["update"]
    assert info["carried"] == [m["regions"]["update"] + x for x in u["carried"]]
    assert all(bm.copy_of[a] == b for a, b in zip(info["carried"], info["moved_old"]))
    assert all(bm.const_idx[x] < 0 and not m["flags"][x] for x in info["carried"]), "a carried leaf is a witness, not a constant"
    if sh:
        assert info["s0"] == m["regions"]["shrink"] and bm.copy_of[info["shrink_top"]] == info["new_root"]
        assert bm.const_idx[info["s0"]] < 0 and bm.consts[bm.const_idx[info["z0"]]] == 0
    else:
        assert info["s0"] is None and m["regions"]["shrink"] == m["regions"]["new_roots"]
    # the sweep: (a) .. (d) of test_alteration_cpu on both forms; one free cell, indicator c's inverse witness
    both_forms(f"ann delete {name} c {c}", (traced[0], traced[1]), (built[0], built[1]), vals, [], 8, m["flags"])
    free = AM.unnoticed(bm, vals, np.asarray([], dtype=object), [int(x) for x in bpub])
    lay = info["layout"]
    inv_c = lay["indicator"] + (8 + 12 * (c - 1) + 4 if c else 0) + 2
    assert free == [inv_c] and AM.explain(bm, vals, inv_c) == AM.IS_ZERO_INVERSE
    # tampering is noticed: every carried leaf, S_0, Z_0, a cluster root, an out_j
    inst = [vals[x] for x in bpub]
    cells = list(info["carried"]) + [lay["roots"] + c, info["outs"][K - 1]] + ([info["s0"], info["z0"], info["shrink_top"]] if sh else [])
    for cell in cells:
        alt = vals.copy()
        alt[cell] = (alt[cell] + 1) % CS.R
        assert AM.violations(AM.recount(bm, alt, np.asarray([], dtype=object), 8, [int(x) for x in bpub], inst)) >= 1, cell


@pytest.mark.parametrize("K", [1, 3])
@pytest.mark.parametrize("shrink", [0, 1])
def test_update_and_delete_share_one_frame(O, K, shrink):
    """Blocks A - D and F - G of the two circuits are the same cells: the layouts agree up to the inner block and, behind it, after
    subtracting its cells; so do the maps' entries, F - G translated by the same amount.  The one operand of each select of F that
    copies the new cluster root is the circuit's own, and is excluded."""
    import ann_update_model as AU
    depth, k = 3, 1
    sizes = ((6, 2, 3), (5, 2, 3))[shrink][:K]               # 6 -> 5 keeps the tree's size, 5 -> 4 halves it
    md, db, ids, cent, ix, tree = case(O, sizes, 0, [1], seed=9)
    assert md["s"] == shrink and len(tree) - 1 == depth
    mu = AU.update_model(O, ix["roots"][:K + 1], 0, MU.build_tree(O, AN.select_cluster(db, ids, 0)[0]), [1], database(O, 1, DIM, 11), 0)
    lu, ld = CS.ann_update_layout(K, k, DIM, depth, 0), CS.ann_delete_layout(K, k, DIM, depth, shrink)
    head = ("c", "centroids_root", "roots", "n_in", "indicator", "select", "sponge_old", "update", "sponge")
    assert all(lu[x] == ld[x] for x in head)
    inner_u, inner_d = lu["update_layout"]["total"], ld["update_layout"]["total"] + ld["shrink_cells"]
    assert ld["shrink_cells"] == (2 + depth * 4506 if shrink else 0) and inner_d > inner_u
    assert all(lu[x] - inner_u == ld[x] - inner_d for x in ("new_roots", "sponge_new", "total"))
    n_head, n_tail = lu["update"], lu["total"] - lu["new_roots"]
    a_operand = 8 * np.arange(K) + 3                         # select: [a - b, 1, b, a, b, sel, a - b, out]
    keep = np.setdiff1d(np.arange(n_tail), a_operand)
    fu, fd = fetchers(mu), fetchers(md)
    for form_u, form_d in ((CS.trace_ann_update, CS.trace_ann_delete), (CS.build_ann_update, CS.build_ann_delete)):
        (cu, _, iu), (cd, _, idl) = form_u(K, k, DIM, depth, fu[0], fu[1], grow=0), form_d(K, k, DIM, depth, fd[0], fd[1], shrink=shrink)
        entries = []
        for cm, lay, info in ((cu, lu, iu), (cd, ld, idl)):
            cells = np.concatenate([np.arange(n_head), lay["new_roots"] + np.arange(n_tail)])
            src = cm.copy_of[cells]
            new_root = info["s0"] if shrink and cm is cd else info["new_root"]
            assert np.all(src[n_head + a_operand] == new_root), "F's `a` copies the new cluster root"
            inner = (src >= lay["update"]) & (src < lay["new_roots"])
            assert np.flatnonzero(inner).tolist() == (n_head + a_operand).tolist(), "nothing else of the frame reads the inner block"
            src = np.where(src >= lay["new_roots"], src - lay["new_roots"] + n_head, src)       # into the frame's own numbering
            const = np.where(cm.const_idx[cells] >= 0, np.asarray(cm.consts + [0], dtype=object)[cm.const_idx[cells]], -1)
            entries.append([x[np.concatenate([np.arange(n_head), n_head + keep])] for x in (src, const, cm.asserted[cells], cm.gate[cells])])
        for x, y, name in zip(entries[0], entries[1], ("copy_of", "const", "asserted", "gate")):
            assert np.array_equal(x, y), (form_u.__name__, name)


def test_plain_update_maps_refuse_the_carried_kind():
    with pytest.raises(ValueError):
        CS.merkle_update_layout(2, DIM, 2, kinds=[2, 1])
    assert CS.merkle_update_layout(2, DIM, 2, kinds=[2, 1], carried=True)["total"] == CS.merkle_update_layout(2, DIM, 2, kinds=[1, 1])["total"]
    with pytest.raises(ValueError):
        CS.ann_delete_layout(0, 1, DIM, 2)
    with pytest.raises(ValueError):
        CS.ann_delete_shrink(3, 3)


def test_library_exports_the_index_delete_entry_points():
    from halo2_vectordb_amd import _lib
    lib = _lib.load()
    for name in ("vdb_wit_ann_delete_size", "vdb_wit_ann_delete", "vdb_wit_ann_delete_dev", "vdb_ann_index_remove_size", "vdb_ann_index_remove_dev"):
        assert hasattr(lib, name), name
    cells, n_in, ub, sb, s = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint()
    # the size call needs no device; it is circuit_sym's layout, and s is computed, not passed
    for K, n_c, dim, m in ((3, 5, 3, 1), (3, 5, 3, 3), (3, 4, 3, 1), (3, 2, 3, 1), (1, 3, 3, 1), (5, 9, 4, 8), (2, 1000, 128, 8)):
        assert lib.vdb_wit_ann_delete_size(K, n_c, dim, m, ctypes.byref(cells), ctypes.byref(n_in), ctypes.byref(ub), ctypes.byref(sb), ctypes.byref(s)) == 0
        depth, sh = CS.ann_delete_shrink(n_c, m)
        lay = CS.ann_delete_layout(K, m, dim, depth, sh)
        assert (cells.value, n_in.value, ub.value, sb.value, s.value) == (lay["total"], lay["n_in"], lay["update"], lay["shrink"], sh)
        assert lay["shrink_cells"] == (2 + (depth - 1 + sh) * 4506 if sh else 0)
        # a delete costs 2 (1 + 9,048 d + 1 + 3 (d - 1)) cells of block E' behind its 2 (1 + 2 d) inputs
        assert lay["update_layout"]["total"] == m * (2 * (1 + 2 * depth) + 2 * (1 + 9048 * depth + 1 + 3 * (depth - 1)))
    for K, n_c, m in ((0, 3, 1), (4097, 3, 1), (3, 3, 0), (3, 3, 3), (3, 1, 1), (3, 5000, 2049)):
        assert lib.vdb_wit_ann_delete_size(K, n_c, 3, m, ctypes.byref(cells), ctypes.byref(n_in), ctypes.byref(ub), ctypes.byref(sb), ctypes.byref(s)) == -3
    # the remove plan: halvings, digests and segment offsets of the next index, and its refusals
    sizes = np.asarray([5, 2, 3], dtype=np.uint64)
    dig, seg = ctypes.c_uint64(), np.zeros(5, dtype=np.uint64)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    for c, slots, want_s, want_seg in ((0, [1], 1, [0, 8, 12, 20, 28]), (0, [4, 0, 0], 2, [0, 4, 8, 16, 24]), (1, [0], 1, [0, 16, 18, 26, 34]),
                                       (2, [2], 1, [0, 16, 20, 24, 32])):
        idx = np.asarray(slots, dtype=np.uint64)
        assert lib.vdb_ann_index_remove_size(p(sizes), 3, c, p(idx), len(slots), ctypes.byref(s), ctypes.byref(dig), p(seg)) == 0
        assert s.value == want_s and seg.tolist() == want_seg and dig.value == want_seg[-1]
    for c, slots in ((0, [5]), (0, [0, 4]), (1, [0, 0]), (3, [0]), (0, [])):
        idx = np.asarray(slots + [0], dtype=np.uint64)
        assert lib.vdb_ann_index_remove_size(p(sizes), 3, c, p(idx), len(slots), None, None, None) == -3
