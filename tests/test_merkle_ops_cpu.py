"""Deletes and tree growth in the Merkle update circuit, without a GPU.  tests/merkle_ops_model.py is the checker of the GPU streams:
here a plain batch of it is merkle_update_model's stream byte for byte, its roots are the oracle's poseidon_merkle_root of the
database after the deletes and after growth, its empty-subtree digests are the roots of all-padding trees, the traced and the
block-built constraint maps (circuit_sym.trace_merkle_update / build_merkle_update with kinds and grow) agree and accept its witness,
the single-cell alteration sweep leaves no cell free, and the library exports the entry points."""
import ctypes
import os

import numpy as np
import pytest

import merkle_ops_model as MO
import merkle_update_model as MU
import topk_model as TM
from halo2_vectordb_amd import circuit_sym as CS
from test_alteration_cpu import both_forms
from test_batch_query_cpu import same_map
from test_merkle_update_cpu import database, fetchers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def kernel_like_flags(m):
    """the flag bytes the kernels write for the model's stream: its gate bits, the constant bit on the load_constant cells and on the
    constant cells of every permutation (as tests/test_merkle_update_cpu.py::kernel_like_flags reads them off the values)"""
    from halo2_vectordb_amd import copymap as CM
    flags = m["selectors"].astype(np.uint8).copy()
    vals = TM.to_ints(m["advice"])
    for c in m["constants"]:
        assert vals[c] == 0
        flags[c] |= 2
    for at, n_in in m["perms"]:
        size = CM.perm_cells(n_in)
        t = CM._Tracer(None)
        t.next_is_const = lambda: vals[at + len(t.src)] == 0 and vals[at + len(t.src) + 3] == vals[at + len(t.src) + 1] * vals[at + len(t.src) + 2] % CS.R
        CM._trace_permutation(t, n_in)
        assert len(t.src) == size and np.array_equal(np.asarray(t.gate, dtype=np.uint8), flags[at:at + size] & 1)
        flags[at:at + size] |= np.asarray(t.cst, dtype=np.uint8) << 1
    return flags


def ops_case(O, n, dim, indices, kinds, grow, seed=7):
    """-> (model, the grown tree after the batch, the grown tree before it)"""
    db = database(O, n, dim, seed)
    tree = MO.grow_tree(O, MU.build_tree(O, db), grow)
    before = [[x.copy() for x in lv] for lv in tree]
    kinds = [0] * len(indices) if kinds is None else kinds
    new = database(O, max(kinds.count(0), 1), dim, seed + 1)[: kinds.count(0)]
    return MO.ops_model(O, tree, indices, kinds, new, grow), tree, before


# ---------------------------------------------------------------------------------------------------------------- what it computes
@pytest.mark.parametrize("n,dim,indices", [(6, 4, [2, 5, 2, 7]), (2, 3, [1, 0]), (5, 5, [4])])
def test_a_plain_batch_is_the_update_models_stream(O, n, dim, indices):
    db, new = database(O, n, dim, 3), database(O, len(indices), dim, 4)
    ta, tb = MU.build_tree(O, db), MU.build_tree(O, db)
    a = MU.update_model(O, ta, indices, new, plan_k=12)
    b = MO.ops_model(O, tb, indices, None, new, 0, plan_k=12)
    for key in ("advice", "selectors", "public", "break_points"):
        assert np.asarray(a[key]).tobytes() == np.asarray(b[key]).tobytes(), key
    assert a["n_in"] == b["n_in"] and b["constants"] == [] and b["growth"] is None
    assert np.array_equal(MU.flat_levels(ta), MU.flat_levels(tb))
    assert [r["block"] for r in a["regions"]] == [r["block"] for r in b["regions"]]


def test_deleting_the_tail_leaves_the_commitment_of_the_head(O):
    n, dim = 6, 3
    db = database(O, n, dim, 11)
    tree = MU.build_tree(O, db)
    m = MO.ops_model(O, tree, [5, 4], [1, 1], db[:0], 0)
    head = np.stack([MU.build_tree(O, db[:4])[0][i] if i < 4 else MU.ZERO for i in range(8)])
    want = [list(head)]
    while len(want[-1]) > 1:
        prev = want[-1]
        want.append(list(O.poseidon_hash_many(np.stack([np.stack([prev[2 * i], prev[2 * i + 1]]) for i in range(len(prev) // 2)]))))
    assert np.array_equal(MU.flat_levels(tree), MU.flat_levels(want)), "the first four vectors in the same lp = 8 tree"
    # ... whose left half is the oracle's commitment of the four (lp = 4) and whose right half is the empty subtree of height 2
    z, _ = MO.empty_digests(O, 3)
    assert np.array_equal(want[2][0], O.poseidon_merkle_root(db[:4])) and np.array_equal(want[2][1], z[2])
    assert np.array_equal(m["public"][-1], want[3][0]) and np.array_equal(m["public"][0], O.poseidon_merkle_root(db))
    assert np.array_equal(m["public"][3], MU.ZERO) and np.array_equal(m["public"][6], MU.ZERO) and not np.array_equal(m["public"][2], MU.ZERO)
    assert len(m["constants"]) == 2 and m["advice"].shape[0] == CS.merkle_update_layout(2, dim, 3, [1, 1])["total"]


def test_growth_then_insert_is_the_oracles_root_of_five(O):
    n, dim = 4, 4
    db, new = database(O, n, dim, 12), database(O, 1, dim, 13)
    small = MU.build_tree(O, db)
    tree = MO.grow_tree(O, small, 1)
    assert len(tree[0]) == 8 and np.array_equal(tree[2][0], O.poseidon_merkle_root(db)) and len(small[0]) == 4
    m = MO.ops_model(O, tree, [4], [0], new, 1)
    five = np.concatenate([db, new])
    assert np.array_equal(m["public"][-1], O.poseidon_merkle_root(five))
    assert np.array_equal(m["public"][0], O.poseidon_merkle_root(db)), "the public old root is R_0"
    assert np.array_equal(MU.flat_levels(tree), MU.flat_levels(MU.build_tree(O, five)))
    lay = CS.merkle_update_layout(1, dim, 3, [0], 1)
    assert m["advice"].shape[0] == lay["total"] and m["n_in"] == lay["n_in"] and lay["grow_cells"] == (3 - 1 + 1) * 4506 + 1
    assert m["growth"]["r0"] == lay["r0"] and m["growth"]["z0"] == lay["z0"] and m["regions"][0]["block"] == lay["block"][0]


def test_empty_digests_are_the_roots_of_all_padding_subtrees(O):
    z, _ = MO.empty_digests(O, 4)
    assert np.array_equal(z[0], MU.ZERO)
    # a tree over one vector padded to 2^l leaves: every subtree beside the first leaf's path is all padding
    for l in range(1, 4):
        tree = MU.build_tree(O, database(O, (1 << l) // 2 + 1, 3, l))
        grown = MO.grow_tree(O, tree, 1)
        assert np.array_equal(grown[l][1], z[l]) and all(np.array_equal(x, MU.ZERO) for x in grown[0][len(tree[0]):])
    # Z_l itself: build_tree's levels over leaves that are all zero
    lv = [MU.ZERO.copy() for _ in range(8)]
    for l in range(1, 4):
        lv = list(O.poseidon_hash_many(np.stack([np.stack([lv[2 * i], lv[2 * i + 1]]) for i in range(len(lv) // 2)])))
        assert all(np.array_equal(x, z[l]) for x in lv), l


def test_updates_of_one_batch_see_each_other_deletes_included(O):
    m, tree, _ = ops_case(O, 5, 3, [2, 2, 3, 7, 2], [0, 1, 1, 1, 0], 0)
    pub = m["public"]
    assert np.array_equal(pub[2 + 3], pub[3]), "the delete's old leaf is the leaf the write before it left"
    assert np.array_equal(pub[3 + 3], MU.ZERO) and np.array_equal(pub[2 + 9], MU.ZERO) and np.array_equal(pub[3 + 9], MU.ZERO), "0 -> 0 is legal"
    assert np.array_equal(pub[2 + 12], MU.ZERO) and not np.array_equal(pub[3 + 12], MU.ZERO)


# ---------------------------------------------------------------------------------------------------------------- the constraint maps
MAPS = {
    "mixed": (5, 3, [2, 2, 3, 7], [0, 1, 0, 1], 0),
    "all_deletes": (3, 4, [1, 0, 1], [1, 1, 1], 0),
    "grow2_mixed": (3, 3, [9, 2, 15], [0, 1, 1], 2),
    "one_leaf_grow1": (1, 4, [1, 0], [0, 1], 1),
    "grow1_all_writes": (2, 3, [3], [0], 1),
}


@pytest.mark.parametrize("name", sorted(MAPS))
def test_traced_and_built_maps_agree_and_every_cell_is_bound(O, name):
    n, dim, indices, kinds, grow = MAPS[name]
    m, tree, _ = ops_case(O, n, dim, indices, kinds, grow)
    depth, k = len(tree) - 1, len(indices)
    m["flags"] = kernel_like_flags(m)
    ff, fv, vals = fetchers(m)
    traced = CS.trace_merkle_update(k, dim, depth, ff, fv, kinds=kinds, grow=grow)
    built = CS.build_merkle_update(k, dim, depth, ff, fv, kinds=kinds, grow=grow)
    same_map(traced[0], built[0])
    assert traced[1] == built[1] and len(built[1]) == 3 * k + 2
    bm, bpub = built
    assert bm.n_cells == m["advice"].shape[0]
    rep = bm.check_witness(vals, [], flags=m["flags"])
    assert not any(rep.values()), rep
    assert [vals[c] for c in bpub] == TM.to_ints(m["public"])
    # the constants are fixed-column constants; R_grow -> the top of update 0's old path is a copy
    for c in m["constants"]:
        assert bm.const_idx[c] >= 0 and int(bm.consts[bm.const_idx[c]]) == 0
    for j, kd in enumerate(kinds):
        assert (m["regions"][j]["new_leaf"] is not None) == bool(kd)
        if kd:
            assert bpub[3 + 3 * j] == m["regions"][j]["new_leaf"]
    if grow:
        g = m["growth"]
        assert bpub[0] == g["r0"] and bm.const_idx[g["z0"]] >= 0
        first = m["regions"][0]["block"]
        tops = [c for c in np.flatnonzero(bm.copy_of != np.arange(bm.n_cells)) if c >= first and g["z0"] < bm.copy_of[c] < first]
        assert len(tops) == 1 and tops[0] < m["regions"][0]["index"] and bm.copy_of[tops[0]] >= g["r"][-1], "one tie, from the last R hash"
    # the sweep: no is_zero in this circuit, so nothing is free; it raises on a cell that is tied to nothing
    both_forms(f"merkle ops {name}", traced, built, vals, [], 8, m["flags"])
    import alteration_model as AM
    assert AM.unnoticed(bm, vals, np.asarray([], dtype=object), [int(c) for c in bpub]) == []
    inst = [vals[c] for c in bpub]

    def noticed(cell):
        alt = vals.copy()
        alt[cell] = (alt[cell] + 1) % CS.R
        return AM.violations(AM.recount(bm, alt, np.asarray([], dtype=object), 8, [int(c) for c in bpub], inst)) >= 1

    for c in m["constants"]:
        assert noticed(c), ("a load_constant cell", c)
    if grow:
        g = m["growth"]
        assert noticed(g["r0"]) and noticed(g["z0"])
        for at in g["r"]:                                     # R_{i+1}: the one cell of the hash that a later cell copies
            later = np.flatnonzero((bm.copy_of >= at) & (bm.copy_of < at + 4506) & (np.arange(bm.n_cells) >= at + 4506))
            digest = {int(bm.copy_of[c]) for c in later}
            assert len(digest) == 1 and noticed(digest.pop()), at


def test_layout_refuses_what_the_circuit_has_no_shape_for():
    for kw in (dict(kinds=[0]), dict(kinds=[0, 2]), dict(grow=-1), dict(grow=4)):
        with pytest.raises(ValueError):
            CS.merkle_update_layout(2, 4, 3, **kw)
    plain, same = CS.merkle_update_layout(3, 5, 4), CS.merkle_update_layout(3, 5, 4, [0, 0, 0], 0)
    assert plain == same and plain["block"] == [plain["n_in"] + j * plain["per_update"] for j in range(3)] and plain["r0"] is None
    lay = CS.merkle_update_layout(64, 128, 14, [1] * 64, 1)
    assert lay["total"] == lay["n_in"] + (14 - 1 + 1) * 4506 + 1 + 64 * (1 + 14 * 9048 + 40) and lay["n_in"] == 64 * (1 + 28) + 1


# ---------------------------------------------------------------------------------------------------------------- the ABI
def test_library_exports_the_ops_entry_points():
    lib_path = os.path.join(ROOT, "halo2_vectordb_amd", "libvdb_hip.so")
    if not os.path.exists(lib_path):
        import __graft_entry__ as g
        g.build()
    lib = ctypes.CDLL(lib_path)
    names = ("vdb_merkle_tree_grow_dev", "vdb_wit_merkle_update_ops_size", "vdb_wit_merkle_update_ops", "vdb_wit_merkle_update_ops_dev")
    header = open(os.path.join(ROOT, "include", "vdb.h")).read()
    from halo2_vectordb_amd import _lib, api
    for name in names:
        assert hasattr(lib, name), name
        assert f"int {name}(" in header and name in _lib._SIGNATURES, name
    assert callable(api.merkle_tree_grow)
    # the size entry needs no device: the shape and its limits
    lib.vdb_wit_merkle_update_ops_size.argtypes = [ctypes.c_size_t] * 3 + [ctypes.c_void_p, ctypes.c_uint] + [ctypes.c_void_p] * 2
    cells, n_in = ctypes.c_uint64(), ctypes.c_uint64()

    def size(n, dim, kinds, grow):
        k = (ctypes.c_uint8 * max(len(kinds), 1))(*kinds)
        return lib.vdb_wit_merkle_update_ops_size(n, dim, len(kinds), k, grow, ctypes.byref(cells), ctypes.byref(n_in))

    for n, dim, kinds, grow in ((16384, 128, [0] * 64, 0), (16384, 128, [1] * 64, 1), (5, 3, [0, 1, 0, 1, 1, 0, 1], 2), (1, 4, [0, 1], 1)):
        depth = max(n - 1, 0).bit_length() + grow
        lay = CS.merkle_update_layout(len(kinds), dim, depth, kinds, grow)
        assert size(n, dim, kinds, grow) == 0 and (cells.value, n_in.value) == (lay["total"], lay["n_in"]), (n, dim, kinds, grow)
    assert lib.vdb_wit_merkle_update_ops_size(16384, 128, 64, None, 0, ctypes.byref(cells), ctypes.byref(n_in)) == 0
    assert cells.value == 64 * (128 + 1 + 28) + 64 * (146634 + 14 * 9048 + 40), "no kinds: a plain batch"
    for n, dim, kinds, grow in ((8, 4, [0, 2], 0), (8, 4, [0], 28), (1, 4, [0], 0), (8, 4, [], 0), (8, 4, [1] * 4097, 0), (1 << 30, 4, [1], 1)):
        assert size(n, dim, kinds, grow) == -3, (n, dim, len(kinds), grow)
