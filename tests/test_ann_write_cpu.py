"""The linked write without a GPU (circuit_sym.trace_ann_write / build_ann_write; tests/ann_write_model.py): the four public roots are the
oracle's and the index model's before and after the batch, blocks A - D, E, F, G are build_ann_update's cell for cell, the two new ties
hold and break alone, a database slot with an equal digest is as good as the member's own, the only free cell is the update's, and a
cover of the old pair of roots followed by the write gives a pair the cover model accepts."""
import ctypes

import numpy as np
import pytest

import alteration_model as AM
import ann_cover_model as CM
import ann_model as AN
import ann_update_model as AU
import ann_write_model as AW
import merkle_ops_model as MO
import merkle_update_model as MU
import topk_model as TM
from halo2_vectordb_amd import circuit_sym as CS
from test_alteration_cpu import both_forms
from test_ann_cover_cpu import built as cover_built, clean as cover_clean
from test_batch_query_cpu import FIELDS, same_map
from test_merkle_update_cpu import database, fetchers

DIM = 3
GROWS = {"flat": (0, 0), "both_grow": (1, 1), "cluster_grows": (1, 0), "db_grows": (0, 1), "append_then_replace": (0, 0), "one_cluster": (0, 0)}
_CASES = {}


def trees(O, db, ids, c, g_c, g_db):
    """(the cluster's tree and the database tree, both grown, as lists per level; the cluster's database slots)"""
    rows, slots = AN.select_cluster(db, ids, c)
    return MO.grow_tree(O, MU.build_tree(O, rows), g_c), MO.grow_tree(O, MU.build_tree(O, db), g_db), [int(x) for x in slots]


def case(O, name, seed=5, duplicate=None):
    """-> dict(model, db, ids, cent, new, ix: the index model before the batch, tree / tree_db: the two trees after it, db_idx, shape),
    computed once per shape and shared (nothing alters it).  duplicate = (i, j): row j of the database is made a copy of row i"""
    key = (name, seed, duplicate)
    if key not in _CASES:
        sizes, c, slots = AW.SHAPES[name]
        ids, K = AW.interleaved_ids(sizes), len(sizes)
        db, cent, new = database(O, len(ids), DIM, seed), database(O, K, DIM, seed + 1), database(O, len(slots), DIM, seed + 2)
        if duplicate:
            db[duplicate[1]] = db[duplicate[0]]
        ix = AN.index_model(O, db, ids, cent)
        members = [int(x) for x in AN.select_cluster(db, ids, c)[1]]
        db_idx, appends = AW.db_indices(members, slots, len(ids))
        shape = AW.shape_of(sizes[c], len(ids), appends)
        tree, tree_db, _ = trees(O, db, ids, c, shape[1], shape[3])
        m = AW.write_model(O, ix["roots"][:K + 1], c, tree, tree_db, slots, db_idx, new, shape[1], shape[3])
        _CASES[key] = dict(model=m, db=db, ids=ids, cent=cent, new=new, ix=ix, tree=tree, tree_db=tree_db, db_idx=db_idx, appends=appends, shape=shape,
                           members=members)
    return _CASES[key]


def maps(O, name, **kw):
    c = case(O, name, **kw)
    if "maps" not in c:
        sizes, _, slots = AW.SHAPES[name]
        ff, fv, vals = fetchers(c["model"])
        d_c, g_c, d_db, g_db = c["shape"]
        args = (len(sizes), len(slots), DIM, d_c, ff, fv)
        c["maps"] = (CS.trace_ann_write(*args, grow=g_c, depth_db=d_db, grow_db=g_db), CS.build_ann_write(*args, grow=g_c, depth_db=d_db, grow_db=g_db), vals)
    return c["maps"]


def recount(bm, bpub, vals):
    none, pub = np.asarray([], dtype=object), [int(x) for x in bpub]
    return AM.recount(bm, vals, none, 8, pub, [vals[x] for x in pub])


def covered(O, db, ids, cent, b=None, sizes=None):
    """the cover model over the database `db` and the index grouping `ids` (b: the clusters' leaves in grouped order, where they are not
    the stable grouping of the database's), checked clean on the host-built cover map -> its public pair"""
    K = cent.shape[0]
    a = O.poseidon_hash_many(db)
    sizes = tuple(int(x) for x in np.bincount(ids, minlength=K)) if sizes is None else sizes
    b = np.ascontiguousarray(a[np.argsort(ids, kind="stable")]) if b is None else b
    m = CM.cover_model(O, a, b, sizes, O.poseidon_merkle_root(cent))
    cm, public, info, vals = cover_built(m, sizes)
    cover_clean(cm, vals, m, public)
    return m["public"]


@pytest.mark.parametrize("name", sorted(AW.SHAPES))
def test_the_four_roots_are_the_oracles_and_the_index_models(O, name):
    sizes, c, slots = AW.SHAPES[name]
    cs = case(O, name)
    m, db, ids, ix, K, k = cs["model"], cs["db"], cs["ids"], cs["ix"], len(sizes), len(slots)
    assert (cs["shape"][1], cs["shape"][3]) == GROWS[name]
    assert cs["shape"] == (len(cs["tree"]) - 1, AU.smallest_grow(sizes[c], cs["appends"]), len(cs["tree_db"]) - 1, AU.smallest_grow(len(ids), cs["appends"]))
    db2, ids2 = AU.updated_database(db, ids, c, slots, cs["new"])
    ix2 = AN.index_model(O, db2, ids2, cs["cent"])
    pub = m["public"]
    assert pub.shape[0] == 4 * k + 5 and TM.to_ints(pub[2:3]) == [c]
    assert np.array_equal(pub[0], O.poseidon_merkle_root(db)) and np.array_equal(pub[-2], O.poseidon_merkle_root(db2))
    assert np.array_equal(pub[1], ix["roots"][-1]) and np.array_equal(pub[-1], ix2["roots"][-1])
    assert np.array_equal(m["new_cluster_root"], ix2["roots"][1 + c])
    assert np.array_equal(MU.flat_levels(cs["tree"]), ix2["forest"][c]), "the cluster's tree after the batch is the fresh build's segment"
    assert np.array_equal(MU.flat_levels(cs["tree_db"]), MU.flat_levels(MU.build_tree(O, db2))), "the database tree after the batch is the fresh build's"
    # per write: [idx, db_idx, old leaf, new leaf]; the new leaf is the row's digest, both trees hold it where the write put it
    digests = O.poseidon_hash_many(cs["new"])
    members = [db[x] for x in cs["members"]]
    for j, s in enumerate(slots):
        per = pub[3 + 4 * j: 7 + 4 * j]
        assert TM.to_ints(per[:2]) == [s, cs["db_idx"][j]] and np.array_equal(per[3], digests[j])
        if s == len(members):
            assert not per[2].any() and cs["db_idx"][j] == len(ids) + (len(members) - sizes[c])
            members.append(None)
        else:
            assert np.array_equal(per[2], O.poseidon_hash_many(members[s][None])[0])
        members[s] = cs["new"][j]
    assert np.array_equal(m["update_db"]["public"][1::3][:k], TM.to_limbs(cs["db_idx"])) and np.array_equal(m["update_db"]["public"][3::3], digests)
    if name == "flat":
        assert cs["db_idx"] == [2] and slots == [1], "a replacement whose database slot is not its cluster slot"
    if name == "append_then_replace":
        assert cs["db_idx"] == [5, 5, 3, 3], "the appended member's database slot comes from the batch"
    lay = CS.ann_write_layout(K, k, DIM, *cs["shape"])
    assert m["advice"].shape[0] == lay["total"] and all(m["regions"][r] == lay[r] for r in m["regions"])


@pytest.mark.parametrize("name", sorted(AW.SHAPES))
def test_traced_and_built_maps_agree_and_accept_the_model(O, name):
    sizes, c, slots = AW.SHAPES[name]
    cs = case(O, name, seed=9)
    m, K, k = cs["model"], len(sizes), len(slots)
    traced, built, vals = maps(O, name, seed=9)
    same_map(traced[0], built[0])
    assert traced[1] == built[1] and len(built[1]) == 4 * k + 5
    assert {x: traced[2][x] for x in traced[2] if x != "layout"} == {x: built[2][x] for x in built[2] if x != "layout"}
    bm, bpub, info = built
    assert bm.n_cells == m["advice"].shape[0]
    rep = bm.check_witness(vals, [], flags=m["flags"])
    assert not any(rep.values()), rep                        # every gate, copy and constant
    assert AM.violations(recount(bm, bpub, vals)) == 0
    assert [vals[x] for x in bpub] == TM.to_ints(m["public"])
    assert [vals[x] for x in info["indicators"]] == m["indicators"] and vals[info["picked"]] == m["picked"]
    assert [vals[x] for x in info["outs"]] == m["outs"] and bm.copy_of[info["old_root"]] == info["picked"]
    # the two new ties, and what they tie
    reg = m["regions"]
    assert info["carried"] == [reg["update_db"] + x for x in m["update_db"]["carried"]]
    assert all(bm.copy_of[x] == y for x, y in zip(info["carried"], info["new_leaves"])), "the database gains the digest the cluster gains"
    assert all(bm.copy_of[x] == y for x, y in zip(info["old_leaves_db"], info["old_leaves"])), "and loses the digest the cluster loses"
    assert all(bm.const_idx[x] < 0 and not m["flags"][x] for x in info["carried"]), "a carried leaf is a witness, not a constant"
    assert all(reg["update"] <= x < reg["update_db"] for x in info["new_leaves"] + info["old_leaves"])
    assert [vals[x] for x in info["new_leaves"]] == TM.to_ints(O.poseidon_hash_many(cs["new"]))
    # the public database roots are E_db's own, the new cluster root F selects is E's
    assert (bpub[0], bpub[-2]) == (info["old_root_db"], info["new_root_db"]) and reg["update_db"] <= info["old_root_db"] < info["new_root_db"] < reg["new_roots"]
    lay = info["layout"]
    assert all(bm.copy_of[lay["new_roots"] + 8 * j + 3] == info["new_root"] for j in range(K)) and info["new_root"] < reg["update_db"]


@pytest.mark.parametrize("name", sorted(AW.SHAPES))
def test_blocks_a_to_e_f_and_g_are_build_ann_updates_cell_for_cell(O, name):
    """the map of the linked write, E_db cut out, IS the map of the plain update at the same arguments: the same copies, constants and
    gates, a cell behind E_db standing for the cell that many places earlier; so are the streams' values and flag bytes"""
    sizes, c, slots = AW.SHAPES[name]
    cs = case(O, name, seed=9)
    m, K, k = cs["model"], len(sizes), len(slots)
    d_c, g_c, d_db, g_db = cs["shape"]
    tree = trees(O, cs["db"], cs["ids"], c, g_c, g_db)[0]
    mu = AU.update_model(O, cs["ix"]["roots"][:K + 1], c, tree, slots, cs["new"], g_c)
    ff, fv, _ = fetchers(mu)
    um, upub, uinfo = CS.build_ann_update(K, k, DIM, d_c, ff, fv, grow=g_c)
    wm, wpub, winfo = maps(O, name, seed=9)[1]
    lo, hi = m["regions"]["update_db"], m["regions"]["new_roots"]
    assert lo == mu["regions"]["new_roots"] and wm.n_cells - um.n_cells == hi - lo == CS.merkle_update_layout(k, 1, d_db, [2] * k, g_db, carried=True)["total"]
    keep = np.concatenate([np.arange(lo), np.arange(hi, wm.n_cells)])
    for key in ("advice", "flags"):
        assert np.array_equal(m[key][keep], mu[key]), key
    back = lambda x: np.where(x >= hi, x - (hi - lo), x)     # a cell of the write's map as the update's map numbers it
    for f in FIELDS:
        x, y = getattr(wm, f), getattr(um, f)
        if f == "lookup_src":
            assert len(x) == len(y) == 0
            continue
        x = x[keep]
        if f == "copy_of":
            assert not ((x >= lo) & (x < hi)).any(), "nothing outside E_db copies a cell of E_db"
            x = back(x)
        if f == "const_idx":
            x = np.where(x >= 0, np.asarray(wm.consts + [0], dtype=object)[x], -1)
            y = np.where(y >= 0, np.asarray(um.consts + [0], dtype=object)[y], -1)
        assert np.array_equal(x, y), f
    # the public row: the update's values in the update's order, with db_idx and the two database roots put in
    assert [int(back(np.asarray(x))) for x in [wpub[1], wpub[2]] + [wpub[3 + 4 * j + i] for j in range(k) for i in (0, 2, 3)] + [wpub[-1]]] == [int(x) for x in upub]
    # what E_db copies from outside itself: E's new leaves and old leaves, nothing else
    inside = wm.copy_of[lo:hi]
    outside = sorted(int(x) for x in inside[(inside < lo)])
    assert outside == sorted(winfo["new_leaves"] + winfo["old_leaves"])


@pytest.mark.parametrize("name", ["flat", "both_grow"])
def test_another_digest_carried_breaks_exactly_the_carried_tie(O, name):
    """a witness whose E_db is honest about ANOTHER leaf (its path and its roots computed over it) satisfies every gate and every other
    copy: only the tie between E_db's carried leaf and E's new leaf fails"""
    sizes, c, slots = AW.SHAPES[name]
    cs = case(O, name, seed=9)
    K = len(sizes)
    d_c, g_c, d_db, g_db = cs["shape"]
    tree, tree_db, _ = trees(O, cs["db"], cs["ids"], c, g_c, g_db)
    forged = O.poseidon_hash_many(database(O, 1, DIM, 77))
    m = AW.write_model(O, cs["ix"]["roots"][:K + 1], c, tree, tree_db, slots, cs["db_idx"], cs["new"], g_c, g_db, carried=list(forged))
    bm, bpub, info = maps(O, name, seed=9)[1]
    vals = np.asarray(TM.to_ints(m["advice"]), dtype=object)
    rep = recount(bm, bpub, vals)
    assert AM.violations(rep) == 1 and rep["copies_unequal"] == 1 and rep["first_copy"] == info["carried"][0], rep
    assert vals[info["carried"][0]] != vals[info["new_leaves"][0]] and vals[info["old_leaves_db"][0]] == vals[info["old_leaves"][0]]
    assert not np.array_equal(m["public"][-2], cs["model"]["public"][-2]) and np.array_equal(m["public"][-1], cs["model"]["public"][-1])


def test_a_database_slot_with_another_digest_breaks_exactly_the_old_leaf_tie(O):
    """E_db honest at database slot 3 where the member lives at slot 2: every gate and every other copy holds, the old leaves differ"""
    sizes, c, slots = AW.SHAPES["flat"]
    cs = case(O, "flat", seed=9)
    K = len(sizes)
    tree, tree_db, _ = trees(O, cs["db"], cs["ids"], c, 0, 0)
    m = AW.write_model(O, cs["ix"]["roots"][:K + 1], c, tree, tree_db, slots, [3], cs["new"])
    bm, bpub, info = maps(O, "flat", seed=9)[1]
    vals = np.asarray(TM.to_ints(m["advice"]), dtype=object)
    rep = recount(bm, bpub, vals)
    assert AM.violations(rep) == 1 and rep["copies_unequal"] == 1 and rep["first_copy"] == info["old_leaves_db"][0], rep
    assert vals[info["carried"][0]] == vals[info["new_leaves"][0]]


def test_a_database_slot_with_an_equal_digest_is_as_good_and_the_new_pair_is_covered(O):
    """rows 2 and 3 of the database are equal; the member at cluster slot 1 lives at database slot 2.  A write that names slot 3 satisfies
    the map: both trees lose the same digest and gain the same digest, and the cover of the new pair of roots holds, because equal
    digests are interchangeable in a multiset"""
    sizes, c, slots = AW.SHAPES["flat"]
    cs = case(O, "flat", seed=9, duplicate=(2, 3))
    db, ids, cent, K = cs["db"], cs["ids"], cs["cent"], len(sizes)
    assert cs["db_idx"] == [2] and np.array_equal(db[2], db[3]) and ids[2] != ids[3]
    before = covered(O, db, ids, cent)
    assert np.array_equal(before, cs["model"]["public"][:2])
    tree, tree_db, _ = trees(O, db, ids, c, 0, 0)
    m = AW.write_model(O, cs["ix"]["roots"][:K + 1], c, tree, tree_db, slots, [3], cs["new"])
    ff, fv, vals = fetchers(m)
    bm, bpub, info = CS.build_ann_write(K, 1, DIM, cs["shape"][0], ff, fv, grow=0, depth_db=cs["shape"][2], grow_db=0)
    rep = bm.check_witness(vals, [], flags=m["flags"])
    assert not any(rep.values()), rep
    assert AM.violations(recount(bm, bpub, vals)) == 0
    assert np.array_equal(m["public"][-1], cs["model"]["public"][-1]) and not np.array_equal(m["public"][-2], cs["model"]["public"][-2])
    # the database the roots now commit: row 3 replaced, row 2 as it was; the index: cluster 0 = rows (0, new, 4), cluster 1 = rows (1, old 2)
    db2 = db.copy()
    db2[3] = cs["new"][0]
    a2 = O.poseidon_hash_many(db2)
    h_new = O.poseidon_hash_many(cs["new"])[0]
    b2 = np.stack([a2[0], h_new, a2[4], a2[1], a2[2]])
    after = covered(O, db2, ids, cent, b=b2, sizes=tuple(sizes))
    assert np.array_equal(after, m["public"][-2:])


@pytest.mark.parametrize("name", ["flat", "both_grow"])
def test_every_cell_altered_alone_only_the_updates_inverse_is_free(O, name):
    sizes, c, slots = AW.SHAPES[name]
    cs = case(O, name, seed=9)
    m, K = cs["model"], len(sizes)
    traced, built, vals = maps(O, name, seed=9)
    bm, bpub, info = built
    both_forms(f"ann write {name}", (traced[0], traced[1]), (built[0], built[1]), vals, [], 8, m["flags"])
    free = AM.unnoticed(bm, vals, np.asarray([], dtype=object), [int(x) for x in bpub])
    lay = info["layout"]
    inv_c = lay["indicator"] + (8 + 12 * (c - 1) + 4 if c else 0) + 2
    assert free == [inv_c] and AM.explain(bm, vals, inv_c) == AM.IS_ZERO_INVERSE, "E_db adds no free cell"
    inst = [vals[x] for x in bpub]
    cells = info["carried"] + info["new_leaves"] + info["old_leaves"] + info["old_leaves_db"] + [info["old_root_db"], info["new_root_db"], info["new_root"]]
    cells += [lay["update_db"] + lay["update_db_layout"]["r0"], lay["update_db"] + lay["update_db_layout"]["z0"]] if lay["update_db_layout"]["grow"] else []
    for cell in cells:
        alt = vals.copy()
        alt[cell] = (alt[cell] + 1) % CS.R
        assert AM.violations(AM.recount(bm, alt, np.asarray([], dtype=object), 8, [int(x) for x in bpub], inst)) >= 1, cell


@pytest.mark.parametrize("name", ["both_grow", "append_then_replace"])
def test_chain_cover_then_write_gives_a_covered_pair(O, name):
    """cover(database_root_old, index_root_old) and the write give cover(database_root_new, index_root_new), with n and n_c raised by
    the number of appends"""
    sizes, c, slots = AW.SHAPES[name]
    cs = case(O, name)
    m, db, ids, cent = cs["model"], cs["db"], cs["ids"], cs["cent"]
    assert np.array_equal(covered(O, db, ids, cent), m["public"][:2])
    # the write itself, on the map the library's builder makes: the model's stream satisfies it and its public cells hold the two pairs
    bm, bpub, _ = maps(O, name)[1]
    vals = maps(O, name)[2]
    assert not any(bm.check_witness(vals, [], flags=m["flags"]).values()) and AM.violations(recount(bm, bpub, vals)) == 0
    assert [vals[x] for x in (bpub[0], bpub[1], bpub[-2], bpub[-1])] == TM.to_ints(np.concatenate([m["public"][:2], m["public"][-2:]]))
    db2, ids2 = AU.updated_database(db, ids, c, slots, cs["new"])
    assert len(ids2) == len(ids) + cs["appends"] and int((ids2 == c).sum()) == sizes[c] + cs["appends"] and cs["appends"] == 1
    assert np.array_equal(covered(O, db2, ids2, cent), m["public"][-2:])


def test_the_model_and_the_layout_refuse_what_the_library_refuses():
    with pytest.raises(AssertionError):
        AW.db_indices([0, 1], [3], 4)
    assert AW.db_indices([3, 1], [2, 2, 0], 4) == ([4, 4, 3], 1)
    with pytest.raises(ValueError):
        CS.ann_write_layout(0, 1, 3, 2, 0, 2, 0)
    with pytest.raises(ValueError):
        CS.ann_write_layout(2, 1, 3, 2, 0, 0, 0)


def cell_limit_dim(lib, K, n_c, m):
    """the largest dim at which the plain index update of m replacements still fits VDB_MERKLE_UPDATE_MAX_CELLS = 2^34 cells (by bisection
    over vdb_wit_ann_update_size, which needs no device) -> (dim, the update's cells there)"""
    cells = ctypes.c_uint64()
    fits = lambda dim: lib.vdb_wit_ann_update_size(K, n_c, dim, m, 0, ctypes.byref(cells), None, None) == 0
    lo, hi = 1, 1 << 20
    assert fits(lo) and not fits(hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if fits(mid) else (lo, mid)
    assert fits(lo)
    return lo, cells.value


def test_the_cell_limit_counts_e_and_e_db_together_and_a_batch_above_the_update_limit_is_refused():
    """2^34 cells: at the largest dim at which the plain update of 16 replacements fits, E alone fits and E + E_db does not (a step of
    dim adds at most 16 permutations, 35,808 cells; E_db has 16 x 3 levels of 9,048); some dims below, the linked write fits too"""
    from halo2_vectordb_amd import _lib
    lib = _lib.load()
    K, n_c, n_db, m = 2, 4, 8, 16
    dim, up_cells = cell_limit_dim(lib, K, n_c, m)
    cells = ctypes.c_uint64()
    size = lambda d, mm=m: lib.vdb_wit_ann_write_size(K, n_c, n_db, d, mm, 0, ctypes.byref(cells), None, None, None, None, None)
    e_db = CS.merkle_update_layout(m, 1, 3, [2] * m, 0, carried=True)["total"]
    assert up_cells <= 1 << 34 < up_cells + e_db and (1 << 34) - up_cells < 16 * 2238
    assert size(dim) == -3, "E fits, E + E_db does not"
    assert size(dim - 64) == 0 and (1 << 34) - 64 * 16 * 2238 < cells.value <= 1 << 34
    assert size(1 << 20) == -3 and size((1 << 20) + 1) == -3
    # section 4h's limit on the batch: VDB_MERKLE_UPDATE_MAX_UPDATES = 4,096 updates
    assert size(3, 4096) == 0 and size(3, 4097) == -3


def test_the_librarys_database_slots_are_the_models(O):
    """vdb_ann_write_db_indices (annw_expand on the cluster's recorded slots: what AnnWriteHotPath uses) against the model's brute force"""
    from halo2_vectordb_amd import api
    from halo2_vectordb_amd._lib import VdbError
    for name, (sizes, c, slots) in AW.SHAPES.items():
        ids = AW.interleaved_ids(sizes)
        members = [int(x) for x in np.flatnonzero(ids == c)]
        got, app = api.ann_write_db_indices(members, slots, len(ids))
        assert (got.tolist(), app) == AW.db_indices(members, slots, len(ids)), name
    assert api.ann_write_db_indices([3, 1], [2, 2, 0], 4)[0].tolist() == [4, 4, 3]
    for members, slots, n_db in (([0, 1], [3], 4), ([0, 4], [0], 4), ([0, 1], [0], 0), ([0, 1, 2], [0], 2), ([0, 1], [], 4)):
        with pytest.raises(VdbError) as e:
            api.ann_write_db_indices(members, slots, n_db)
        assert e.value.code == -3, (members, slots, n_db)


def test_library_exports_the_linked_write_entry_points():
    from halo2_vectordb_amd import _lib
    lib = _lib.load()
    for name in ("vdb_wit_ann_write_size", "vdb_wit_ann_write", "vdb_wit_ann_write_dev", "vdb_ann_index_write_size", "vdb_ann_index_write_dev",
                 "vdb_ann_write_db_indices"):
        assert hasattr(lib, name), name
    u64 = ctypes.c_uint64
    cells, n_in, ub, udb, gc, gdb = u64(), u64(), u64(), u64(), ctypes.c_uint(), ctypes.c_uint()
    size = lambda K, n_c, n_db, dim, m, app: lib.vdb_wit_ann_write_size(K, n_c, n_db, dim, m, app, ctypes.byref(cells), ctypes.byref(n_in), ctypes.byref(ub),
                                                                        ctypes.byref(udb), ctypes.byref(gc), ctypes.byref(gdb))
    # the size call needs no device; it is circuit_sym's layout, and g_c and g_db are computed, not passed
    for K, n_c, n_db, dim, m, app in ((2, 3, 5, 3, 1, 0), (2, 2, 4, 3, 1, 1), (2, 2, 5, 3, 2, 1), (2, 3, 4, 3, 1, 1), (1, 3, 3, 3, 2, 1), (32, 32, 1024, 128, 8, 4),
                                      (2, 3, 100, 3, 67, 67)):
        assert size(K, n_c, n_db, dim, m, app) == 0
        d_c, g_c, d_db, g_db = AW.shape_of(n_c, n_db, app)
        lay = CS.ann_write_layout(K, m, dim, d_c, g_c, d_db, g_db)
        assert (cells.value, n_in.value, ub.value, udb.value, gc.value, gdb.value) == (lay["total"], K + 2, lay["update"], lay["update_db"], g_c, g_db)
        up = u64()
        assert lib.vdb_wit_ann_update_size(K, n_c, dim, m, g_c, ctypes.byref(up), None, None) == 0
        assert cells.value - up.value == lay["update_db_layout"]["total"], "E_db on top of the plain update's circuit"
    # K = 0, cluster >= K is not a size matter; an empty database, a cluster larger than its database, more appends than writes, no write,
    # an empty cluster, a one-leaf tree without a path
    for K, n_c, n_db, dim, m, app in ((0, 3, 5, 3, 1, 0), (4097, 3, 5, 3, 1, 0), (2, 3, 0, 3, 1, 0), (2, 6, 5, 3, 1, 0), (2, 3, 5, 3, 1, 2), (2, 3, 5, 3, 0, 0),
                                      (2, 0, 5, 3, 1, 0), (2, 1, 5, 3, 1, 0), (2, 3, 5, 0, 1, 0)):
        assert size(K, n_c, n_db, dim, m, app) == -3, (K, n_c, n_db, dim, m, app)
    # the index plan: the appends, g_c, g_db, the digests and segment offsets of the next index, the digests of its database tree
    sizes = np.asarray([2, 3], dtype=np.uint64)
    app, dig, dbd, seg = u64(), u64(), u64(), np.zeros(4, dtype=np.uint64)
    p = lambda x: x.ctypes.data_as(ctypes.c_void_p)
    for c, slots, want in ((0, [2, 0], (1, 1, 0, [0, 8, 16, 20], 16)), (1, [3, 3, 1, 1], (1, 0, 0, [0, 4, 12, 16], 16)), (0, [2, 3, 4], (3, 2, 0, [0, 16, 24, 28], 16)),
                           (1, [3, 4, 5, 6], (4, 1, 1, [0, 4, 20, 24], 32))):
        idx = np.asarray(slots, dtype=np.uint64)
        assert lib.vdb_ann_index_write_size(p(sizes), 2, c, p(idx), len(slots), ctypes.byref(app), ctypes.byref(gc), ctypes.byref(gdb), ctypes.byref(dig), p(seg),
                                            ctypes.byref(dbd)) == 0
        assert (app.value, gc.value, gdb.value, seg.tolist(), dbd.value) == want and dig.value == want[3][-1]
    for c, slots in ((2, [0]), (0, [3]), (0, [2, 4]), (0, [])):
        idx = np.asarray(slots + [0], dtype=np.uint64)
        assert lib.vdb_ann_index_write_size(p(sizes), 2, c, p(idx), len(slots), None, None, None, None, None, None) == -3
