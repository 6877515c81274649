"""The index move circuit without a GPU (circuit_sym.trace_ann_move / build_ann_move; tests/ann_move_model.py): the model's new index
root is the index model's over the same database with the moved rows' ids set to b, the database tree is untouched, the blocks are the
delete's and the update's cell for cell, the traced and the built map agree, and the single-cell alteration sweep leaves one kind of
cell free: the inverse witness of the is_zero whose operand is zero, one per indicator block.  The carried leaves, S_0, Z_0 and every
mid_j are noticed; a leaf pulled from nowhere breaks exactly the move copy; a == b satisfies the map."""
import ctypes

import numpy as np
import pytest

import alteration_model as AM
import ann_delete_model as AD
import ann_model as AN
import ann_move_model as AV
import ann_update_model as AU
import merkle_ops_model as MO
import merkle_update_model as MU
import topk_model as TM
from halo2_vectordb_amd import circuit_sym as CS
from test_alteration_cpu import both_forms
from test_batch_query_cpu import same_map
from test_merkle_update_cpu import database, fetchers

DIM = 3
_CASES = {}


def case(O, name, seed=5):
    """-> dict(model, db, ids, cent, ix: the index model before the batch, tree_a / tree_b0: the two trees before it (b's grown)),
    computed once per shape and shared (nothing alters it)"""
    if (name, seed) not in _CASES:
        sizes, a, b, slots = AV.SHAPES[name]
        ids = AD.ids_of(sizes)
        K = len(sizes)
        db, cent = database(O, len(ids), DIM, seed), database(O, K, DIM, seed + 1)
        ix = AN.index_model(O, db, ids, cent)
        d_a, s, d_b, g = AV.shape_of(sizes[a], sizes[b], len(slots))
        tree_a = MU.build_tree(O, AN.select_cluster(db, ids, a)[0])
        tree_b = MO.grow_tree(O, MU.build_tree(O, AN.select_cluster(db, ids, b)[0]), g)
        before = ([[x.copy() for x in lv] for lv in tree_a], [[x.copy() for x in lv] for lv in tree_b])
        m = AV.move_model(O, ix["roots"][:K + 1], a, b, tree_a, tree_b, slots)
        _CASES[name, seed] = dict(model=m, db=db, ids=ids, cent=cent, ix=ix, tree_a0=before[0], tree_b0=before[1], tree_a=tree_a, tree_b=tree_b,
                                  shape=(d_a, s, d_b, g))
    return _CASES[name, seed]


def maps(O, name, seed=9):
    c = case(O, name, seed)
    if "maps" not in c:
        sizes, a, b, slots = AV.SHAPES[name]
        ff, fv, vals = fetchers(c["model"])
        d_a, s, d_b, g = c["shape"]
        c["maps"] = (CS.trace_ann_move(len(sizes), len(slots), d_a, s, d_b, g, ff, fv), CS.build_ann_move(len(sizes), len(slots), d_a, s, d_b, g, ff, fv),
                     vals)
    return c["maps"]


@pytest.mark.parametrize("name", sorted(AV.SHAPES))
def test_new_index_root_is_the_index_models_and_the_database_is_untouched(O, name):
    sizes, a, b, slots = AV.SHAPES[name]
    c = case(O, name)
    m, db, ids, ix = c["model"], c["db"], c["ids"], c["ix"]
    K, n_a, n_b, k = len(sizes), sizes[a], sizes[b], len(slots)
    assert (m["s"], m["g"]) == {"shrink_grow": (1, 1), "flat": (0, 0), "repeat": (2, 2), "to_one": (1, 1), "backwards": (1, 1)}[name]
    assert c["shape"] == (len(c["tree_a"]) - 1, m["s"], len(c["tree_b"]) - 1, m["g"])
    grouped2, ids2, slots2 = AV.moved_grouping(db, ids, a, b, slots)
    ix2 = AN.index_model(O, grouped2, ids2, c["cent"])
    assert np.array_equal(m["public"][0], ix["roots"][-1]) and np.array_equal(m["public"][-1], ix2["roots"][-1])
    assert np.array_equal(m["new_root_a"], ix2["roots"][1 + a]) and np.array_equal(m["new_root_b"], ix2["roots"][1 + b])
    assert np.array_equal(MU.flat_levels(m["cut_tree"]), ix2["forest"][a]), "a's tree, cut, is the fresh build's segment"
    assert np.array_equal(MU.flat_levels(m["tree_b"]), ix2["forest"][b]), "b's grown tree after the batch is the fresh build's segment"
    if m["s"]:
        assert np.array_equal(m["shrink_top"], m["delete"]["public"][-1]), "S_s is E''s final root: the dropped half is empty"
    # the database: every row keeps its slot, so the tree over the rows in slot order is the one before the batch
    assert sorted(slots2.tolist()) == list(range(len(ids))) and np.array_equal(db[slots2], grouped2)
    leaves2 = np.concatenate([ix2["forest"][k_][:n] for k_, n in enumerate(np.bincount(ids2))])
    by_slot = np.zeros_like(leaves2)
    by_slot[slots2] = leaves2
    assert np.array_equal(by_slot, np.stack(MU.build_tree(O, db)[0][:len(ids)])), "the database tree's leaves are unchanged"
    moved_slots = [int(x) for x in np.flatnonzero(np.asarray(ids) != _scatter(ids2, slots2))]
    assert len(moved_slots) == k and all(_scatter(ids2, slots2)[x] == b and ids[x] == a for x in moved_slots)
    # public: [root_old | a | b | slot, leaf, last, moved leaf, dest, dest old leaf | root_new]
    pub = m["public"]
    assert pub.shape[0] == 6 * k + 4 and TM.to_ints(pub[1:3]) == [a, b]
    members = list(ix["forest"][a][:n_a])
    for j, s in enumerate(slots):
        per = pub[3 + 6 * j: 9 + 6 * j]
        assert TM.to_ints(per[[0, 2, 4]]) == [s, n_a - 1 - j, n_b + j] and not per[5].any()
        assert np.array_equal(per[1], members[s]) and np.array_equal(per[3], members[-1])
        assert np.array_equal(m["tree_b"][0][n_b + j], members[s]), "what arrived in b is what left a"
        members[s] = members[-1]
        members.pop()
    lay = CS.ann_move_layout(K, k, *c["shape"])
    assert m["advice"].shape[0] == lay["total"] and all(m["regions"][r] == lay[r] for r in m["regions"])
    assert CS.ann_move_shape(n_a, n_b, k) == c["shape"]


def _scatter(vals, slots):
    out = np.zeros(len(vals), dtype=np.int64)
    out[slots] = vals
    return out


def test_the_model_refuses_what_the_library_refuses():
    for n_a, n_b, slots in ((2, 3, [0, 0]), (3, 3, [3]), (3, 3, [0, 2]), (3, 3, [])):
        with pytest.raises(AssertionError):
            AV.simulate(n_a, n_b, slots)
    assert AV.simulate(5, 2, [4, 0, 0]) == ([2, 1], [("b", 0), ("b", 1), ("a", 4), ("a", 0), ("a", 3)], [4, 3, 2])
    with pytest.raises(ValueError):
        CS.ann_move_layout(1, 1, 2, 0, 2, 0)
    with pytest.raises(ValueError):
        CS.ann_move_shape(3, 0, 1)
    with pytest.raises(ValueError):
        CS.ann_move_shape(3, 2, 3)


@pytest.mark.parametrize("name", sorted(AV.SHAPES))
def test_blocks_are_the_deletes_and_the_updates_cell_for_cell(O, name):
    """E' and S are ann_delete_model's on the same tree; E_b is ann_update_model's block E over appends of the moved VECTORS apart from
    the carried cells: every cell outside the leaf sponges (the inputs behind the vectors, the growth block, every level and index)."""
    sizes, a, b, slots = AV.SHAPES[name]
    c = case(O, name)
    m, ix, K, k = c["model"], c["ix"], len(sizes), len(slots)
    reg = m["regions"]
    tree = [[x.copy() for x in lv] for lv in c["tree_a0"]]
    md = AD.delete_model(O, ix["roots"][:K + 1], a, tree, slots)
    n = reg["mid"] - reg["update"]
    rd = md["regions"]
    assert rd["new_roots"] - rd["update"] == n
    for key in ("advice", "flags"):
        assert np.array_equal(m[key][reg["update"]:reg["mid"]], md[key][rd["update"]:rd["new_roots"]]), key
    assert m["s"] == md["s"] and reg["shrink"] - reg["update"] == rd["shrink"] - rd["update"]
    # the appended vectors: the members of a the moves take, in move order
    mem_a = AN.select_cluster(c["db"], c["ids"], a)[0]
    taken = np.stack([mem_a[i] for w, i in AV.simulate(sizes[a], sizes[b], slots)[1] if w == "a"])
    tree_b = [[x.copy() for x in lv] for lv in c["tree_b0"]]
    roots_mid = ix["roots"][:K + 1].copy()
    roots_mid[1 + a] = m["new_root_a"]
    mu = AU.update_model(O, roots_mid, b, tree_b, [sizes[b] + j for j in range(k)], taken, m["g"])
    uu, ub = mu["update"], m["append"]
    assert np.array_equal(uu["public"], ub["public"]), "the same old root, slots, old leaves, NEW LEAVES and new root"
    n_vec = k * DIM
    assert uu["n_in"] - n_vec == ub["n_in"] and np.array_equal(uu["advice"][n_vec:uu["n_in"]], ub["advice"][:ub["n_in"]])
    flags_u, flags_b = mu["flags"][mu["regions"]["update"]:mu["regions"]["new_roots"]], m["flags"][reg["update_b"]:reg["new_roots"]]
    g0u, g0b = uu["n_in"], ub["n_in"]
    glen = uu["regions"][0]["block"] - g0u
    assert glen == ub["regions"][0]["block"] - g0b == (1 + (c["shape"][2] - 1 + m["g"]) * 4506 if m["g"] else 0)
    assert np.array_equal(uu["advice"][g0u:g0u + glen], ub["advice"][g0b:g0b + glen]) and np.array_equal(flags_u[g0u:g0u + glen], flags_b[g0b:g0b + glen])
    for j in range(k):
        lo_u, lo_b = uu["regions"][j]["levels"][0], ub["regions"][j]["levels"][0]
        end_u = uu["regions"][j + 1]["block"] if j + 1 < k else uu["advice"].shape[0]
        end_b = ub["regions"][j + 1]["block"] if j + 1 < k else ub["advice"].shape[0]
        assert end_u - lo_u == end_b - lo_b and lo_b - ub["regions"][j]["block"] == 1
        assert np.array_equal(uu["advice"][lo_u:end_u], ub["advice"][lo_b:end_b]) and np.array_equal(flags_u[lo_u:end_u], flags_b[lo_b:end_b])
        assert np.array_equal(ub["advice"][ub["carried"][j]], ub["public"][3 + 3 * j]) and not flags_b[ub["carried"][j]]
    # and the frame: the move's F_b - G are the update's F - G over mid (the same cells, the map aside)
    tail = m["advice"].shape[0] - reg["new_roots"]
    assert np.array_equal(m["advice"][reg["new_roots"]:], mu["advice"][mu["regions"]["new_roots"]:]) and tail == mu["advice"].shape[0] - mu["regions"]["new_roots"]
    assert np.array_equal(m["public"][-1], mu["public"][-1])


@pytest.mark.parametrize("name", sorted(AV.SHAPES))
def test_traced_and_built_maps_agree_and_accept_the_model(O, name):
    sizes, a, b, slots = AV.SHAPES[name]
    c = case(O, name, seed=9)
    m, K, k = c["model"], len(sizes), len(slots)
    traced, built, vals = maps(O, name)
    same_map(traced[0], built[0])
    assert traced[1] == built[1] and len(built[1]) == 6 * k + 4
    assert {x: traced[2][x] for x in traced[2] if x != "layout"} == {x: built[2][x] for x in built[2] if x != "layout"}
    bm, bpub, info = built
    assert bm.n_cells == m["advice"].shape[0]
    rep = bm.check_witness(vals, [], flags=m["flags"])
    assert not any(rep.values()), rep
    assert [vals[x] for x in bpub] == TM.to_ints(m["public"])
    assert [vals[x] for x in info["indicators"]] == m["indicators"] and vals[info["picked"]] == m["picked"]
    assert [vals[x] for x in info["indicators_b"]] == m["indicators_b"] and vals[info["picked_b"]] == m["picked_b"]
    assert [vals[x] for x in info["mids"]] == m["mids"] and [vals[x] for x in info["outs"]] == m["outs"]
    assert bm.copy_of[info["old_root"]] == info["picked"] and bm.copy_of[info["old_root_b"]] == info["picked_b"]
    reg = m["regions"]
    assert info["carried"] == [reg["update"] + x for x in m["delete"]["carried"]]
    assert info["arrived"] == [reg["update_b"] + x for x in m["append"]["carried"]]
    assert all(bm.copy_of[x] == y for x, y in zip(info["carried"], info["moved_old"]))
    assert all(bm.copy_of[x] == y for x, y in zip(info["arrived"], info["removed"])), "the move: what arrived in b is what left a"
    assert all(bm.const_idx[x] < 0 and not m["flags"][x] for x in info["carried"] + info["arrived"]), "a carried leaf is a witness, not a constant"
    if m["s"]:
        assert info["s0"] == reg["shrink"] and bm.copy_of[info["shrink_top"]] == info["new_root"]
        assert bm.const_idx[info["s0"]] < 0 and bm.consts[bm.const_idx[info["z0"]]] == 0
    else:
        assert info["s0"] is None and reg["shrink"] == reg["mid"]
    # F_a's and F_b's `a` operands copy the new roots: S_0 (E''s final root at s = 0), E_b's final root
    new_a = info["s0"] if m["s"] else info["new_root"]
    lay = info["layout"]
    assert all(bm.copy_of[lay["mid"] + 8 * j + 3] == new_a and bm.copy_of[lay["new_roots"] + 8 * j + 3] == info["new_root_b"] for j in range(K))


def _inverse_cells(lay, a, b):
    inv = lambda at, c: at + (8 + 12 * (c - 1) + 4 if c else 0) + 2
    return sorted([inv(lay["indicator"], a), inv(lay["indicator_b"], b)])


@pytest.mark.parametrize("name", ["shrink_grow", "repeat"])
def test_every_cell_altered_alone_only_the_two_zero_operand_inverses_are_free(O, name):
    sizes, a, b, slots = AV.SHAPES[name]
    c = case(O, name, seed=9)
    m, K = c["model"], len(sizes)
    traced, built, vals = maps(O, name)
    bm, bpub, info = built
    both_forms(f"ann move {name}", (traced[0], traced[1]), (built[0], built[1]), vals, [], 8, m["flags"])
    free = AM.unnoticed(bm, vals, np.asarray([], dtype=object), [int(x) for x in bpub])
    lay = info["layout"]
    assert free == _inverse_cells(lay, a, b) and all(AM.explain(bm, vals, x) == AM.IS_ZERO_INVERSE for x in free)
    # tampering is noticed: every carried leaf of both blocks, S_0, Z_0, S_s, every mid_j, a cluster root, an out_j
    inst = [vals[x] for x in bpub]
    cells = list(info["carried"]) + list(info["arrived"]) + list(info["removed"]) + list(info["mids"]) + [lay["roots"] + a, lay["roots"] + b, info["outs"][K - 1]]
    cells += [info["s0"], info["z0"], info["shrink_top"]] if m["s"] else []
    for cell in cells:
        alt = vals.copy()
        alt[cell] = (alt[cell] + 1) % CS.R
        assert AM.violations(AM.recount(bm, alt, np.asarray([], dtype=object), 8, [int(x) for x in bpub], inst)) >= 1, cell


@pytest.mark.parametrize("name", ["shrink_grow", "backwards"])
def test_a_leaf_pulled_from_nowhere_breaks_exactly_the_move_copy(O, name):
    """A witness whose E_b is honest about ANOTHER leaf (its path, its roots, F_b and G recomputed over it) satisfies every gate and
    every other copy: only the tie between the carried leaf of E_b's update j and the removed leaf of E''s update 2 j fails."""
    sizes, a, b, slots = AV.SHAPES[name]
    c = case(O, name, seed=9)
    K, k = len(sizes), len(slots)
    ix = c["ix"]
    tree_a, tree_b = [[x.copy() for x in lv] for lv in c["tree_a0"]], [[x.copy() for x in lv] for lv in c["tree_b0"]]
    real = AV.append_model
    other = database(O, 1, DIM, 77)
    forged = O.poseidon_hash_many(other)[0]

    def forging(O_, levels, indices, leaves, grow):
        return real(O_, levels, indices, [forged] + list(leaves[1:]), grow)

    AV.append_model = forging
    try:
        m = AV.move_model(O, ix["roots"][:K + 1], a, b, tree_a, tree_b, slots)
    finally:
        AV.append_model = real
    _, built, _ = maps(O, name)
    bm, bpub, info = built
    vals = np.asarray(TM.to_ints(m["advice"]), dtype=object)
    none, pub = np.asarray([], dtype=object), [int(x) for x in bpub]
    rep = AM.recount(bm, vals, none, 8, pub, [vals[x] for x in pub])
    assert AM.violations(rep) == 1 and rep["copies_unequal"] == 1 and rep["first_copy"] == info["arrived"][0], rep
    assert vals[info["arrived"][0]] != vals[info["removed"][0]] and all(vals[x] == vals[y] for x, y in zip(info["arrived"][1:], info["removed"][1:]))
    fixed = vals.copy()
    fixed[info["arrived"][0]] = vals[info["removed"][0]]
    rep = AM.recount(bm, fixed, none, 8, pub, [vals[x] for x in pub])
    assert rep["copies_unequal"] >= 1 and rep["first_copy"] > info["arrived"][0], "with the tie honoured the forged path's own copies of the leaf break"


@pytest.mark.parametrize("sizes,a,slots", [((5, 4, 3), 0, [1]), ((6, 2), 0, [2, 0])])
def test_a_witness_built_sequentially_with_src_equal_to_dst_satisfies_the_map(O, sizes, a, slots):
    """Why the circuit needs no a != b gate: b's root is selected from mid, the roots after the removal, so with a == b block E_b runs
    on the tree E' and S leave and the map is satisfied; the statement proved is then 'these members left a and came back at its end'."""
    ids = AD.ids_of(sizes)
    K, k = len(sizes), len(slots)
    db, cent = database(O, len(ids), DIM, 3), database(O, K, DIM, 4)
    ix = AN.index_model(O, db, ids, cent)
    tree_a = MU.build_tree(O, AN.select_cluster(db, ids, a)[0])
    m = AV.move_model(O, ix["roots"][:K + 1], a, a, tree_a, None, slots, same_cluster=True)
    d_a, s = CS.ann_delete_shrink(sizes[a], k)
    ff, fv, vals = fetchers(m)
    bm, bpub, info = CS.build_ann_move(K, k, d_a, s, d_a, m["g"], ff, fv)
    assert m["g"] == s and bm.n_cells == m["advice"].shape[0]
    rep = bm.check_witness(vals, [], flags=m["flags"])
    assert not any(rep.values()), rep
    assert [vals[x] for x in bpub] == TM.to_ints(m["public"]) and TM.to_ints(m["public"][1:3]) == [a, a]
    # the cluster holds the same multiset of leaves as before
    before = sorted(TM.to_ints(np.stack(MU.build_tree(O, AN.select_cluster(db, ids, a)[0])[0][:sizes[a]])))
    assert sorted(TM.to_ints(np.stack(m["tree_b"][0][:sizes[a]]))) == before


def test_library_exports_the_index_move_entry_points():
    from halo2_vectordb_amd import _lib
    lib = _lib.load()
    for name in ("vdb_wit_ann_move_size", "vdb_wit_ann_move", "vdb_wit_ann_move_dev", "vdb_ann_index_move_size", "vdb_ann_index_move_dev"):
        assert hasattr(lib, name), name
    u64 = ctypes.c_uint64
    cells, n_in, db_, sb, ab, s, g = u64(), u64(), u64(), u64(), u64(), ctypes.c_uint(), ctypes.c_uint()
    size = lambda K, n_a, n_b, m: lib.vdb_wit_ann_move_size(K, n_a, n_b, m, ctypes.byref(cells), ctypes.byref(n_in), ctypes.byref(db_), ctypes.byref(sb),
                                                            ctypes.byref(ab), ctypes.byref(s), ctypes.byref(g))
    # the size call needs no device; it is circuit_sym's layout, and s and g are computed, not passed
    for K, n_a, n_b, m in ((3, 5, 4, 1), (3, 4, 3, 1), (2, 5, 2, 3), (2, 2, 1, 1), (3, 5, 3, 2), (32, 32, 32, 8), (2, 130, 3, 67)):
        assert size(K, n_a, n_b, m) == 0
        d_a, sh, d_b, gr = CS.ann_move_shape(n_a, n_b, m)
        lay = CS.ann_move_layout(K, m, d_a, sh, d_b, gr)
        assert (cells.value, n_in.value, db_.value, sb.value, ab.value, s.value, g.value) == (lay["total"], K + 3, lay["update"], lay["shrink"],
                                                                                             lay["update_b"], sh, gr)
    for K, n_a, n_b, m in ((1, 3, 3, 1), (4097, 3, 3, 1), (3, 3, 3, 0), (3, 3, 3, 3), (3, 1, 3, 1), (3, 5000, 3, 2049), (3, 3, 0, 1)):
        assert size(K, n_a, n_b, m) == -3
    # the index plan: s, g, digests and segment offsets of the next index, and its refusals
    sizes = np.asarray([5, 4, 3], dtype=np.uint64)
    dig, seg = u64(), np.zeros(5, dtype=np.uint64)
    p = lambda x: x.ctypes.data_as(ctypes.c_void_p)
    for a, b, slots, want in ((0, 1, [1], (1, 1, [0, 8, 24, 32, 40])), (2, 0, [0, 1], (2, 0, [0, 16, 24, 26, 34])), (1, 2, [0], (0, 0, [0, 16, 24, 32, 40]))):
        idx = np.asarray(slots, dtype=np.uint64)
        assert lib.vdb_ann_index_move_size(p(sizes), 3, a, b, p(idx), len(slots), ctypes.byref(s), ctypes.byref(g), ctypes.byref(dig), p(seg)) == 0
        assert (s.value, g.value, seg.tolist()) == want and dig.value == want[2][-1]
    for a, b, slots in ((0, 0, [1]), (0, 3, [1]), (3, 0, [1]), (0, 1, [5]), (0, 1, [0, 4]), (2, 0, [0, 0, 0]), (0, 1, [])):
        idx = np.asarray(slots + [0], dtype=np.uint64)
        assert lib.vdb_ann_index_move_size(p(sizes), 3, a, b, p(idx), len(slots), None, None, None, None) == -3
