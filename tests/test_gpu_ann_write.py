"""Linked writes on the GPU (pipeline.AnnWriteHotPath, AnnIndex.written; vdb_wit_ann_write*, vdb_ann_index_write_dev).  The streams are
tests/ann_write_model.py's bit for bit (tests/test_ann_write_cpu.py holds that model against the oracle, the index model and the cover
model first); host and device forms, three rank windows cut inside E_db's growth block, at a carried cell, between E and E_db and
between E_db and F, the launch list, refused arguments, the device-placed map, the whole proof, changed instances, cells tampered in
HBM, another index's database tree, the written index against a fresh build over the updated database with its database tree, the
chain cover - write - cover on the device, the other hot paths on the written index, and a batch beyond one workgroup."""
import ctypes

import numpy as np
import pytest

import ann_model as AN
import ann_update_model as AU
import ann_write_model as AW
import merkle_ops_model as MO
import merkle_update_model as MU
import topk_model as TM
from test_gpu_ann_delete import _resident
from test_gpu_ann_update import _same_index
from test_gpu_batch_query import _dev
from test_gpu_rounds import TAU
from test_gpu_sweep import _check_window, _windowed

pytestmark = pytest.mark.gpu
P, L, DIM = 48, 12, 3
PROVED = "both_grow"


@pytest.fixture(scope="module")
def api():
    from halo2_vectordb_amd import api as a
    a.init(0)
    return a


def _rows(seed, n, dim):
    return np.random.default_rng(seed).integers(0, 219, size=(n, dim)).astype(np.float64)


_MODELS = {}


def _case(O, name, seed=70, slots=None, sizes=None, c=None, block_flags=True):
    """-> dict(f64 rows, quantized rows, the index model before the batch, the two trees before the batch (device layout, not grown and
    grown), the model and the trees after the batch); computed once per case and left unchanged"""
    key = (name, None if slots is None else tuple(slots), sizes, c)
    if key not in _MODELS:
        sizes0, c0, slots0 = AW.SHAPES[name]
        sizes, slots, c = sizes0 if sizes is None else sizes, slots0 if slots is None else slots, c0 if c is None else c
        ids, K = AW.interleaved_ids(sizes), len(sizes)
        f = dict(db=_rows(seed, len(ids), DIM), cent=_rows(seed + 1, K, DIM), new=_rows(seed + 2, len(slots), DIM))
        db, cent, new = O.quantize(f["db"], P), O.quantize(f["cent"], P), O.quantize(f["new"], P)
        ix = AN.index_model(O, db, ids, cent)
        rows_c, members = AN.select_cluster(db, ids, c)
        db_idx, appends = AW.db_indices(members, slots, len(ids))
        d_c, g_c, d_db, g_db = AW.shape_of(sizes[c], len(ids), appends)
        tree_c0, tree_db0 = MU.build_tree(O, rows_c), MU.build_tree(O, db)
        tree, tree_db = MO.grow_tree(O, tree_c0, g_c), MO.grow_tree(O, tree_db0, g_db)
        before = dict(c=MU.flat_levels(tree), db=MU.flat_levels(tree_db), c0=MU.flat_levels(tree_c0), db0=MU.flat_levels(tree_db0))
        m = AW.write_model(O, ix["roots"][:K + 1], c, tree, tree_db, slots, db_idx, new, g_c, g_db, plan_k=13, block_flags=block_flags)
        db2, ids2 = AU.updated_database(db, ids, c, slots, new)
        _MODELS[key] = dict(f=f, db=db, cent=cent, new=new, ids=ids, K=K, dim=DIM, c=c, slots=list(slots), db_idx=db_idx, appends=appends, ix=ix, before=before,
                            m=m, tree=tree, tree_db=tree_db, n_c=int(sizes[c]), n_db=len(ids), shape=(d_c, g_c, d_db, g_db), db2=db2, ids2=ids2)
    return _MODELS[key]


def _write_dev(api, s, levels_db=None, profile=False):
    """vdb_wit_ann_write_dev into poisoned buffers -> (stream, flags, public, the cluster's levels after, the database's[, launches per
    kernel of a second run])"""
    from halo2_vectordb_amd._lib import check
    lib = api.init()
    m, K = len(s["slots"]), s["K"]
    d_c, g_c, d_db, g_db = s["shape"]
    cells = s["m"]["advice"].shape[0]
    idx, dbi = np.ascontiguousarray(s["slots"], dtype=np.uint64), np.ascontiguousarray(s["db_idx"], dtype=np.uint64)
    levels_c, levels_db = s["before"]["c"], s["before"]["db"] if levels_db is None else levels_db
    up = []
    try:
        d_lc, d_ld, d_roots, d_new = _dev(api, up, levels_c), _dev(api, up, levels_db), _dev(api, up, s["ix"]["roots"][:K + 1]), _dev(api, up, s["new"])
        d_adv, d_sel, d_pub = api.DeviceBuffer(cells * 32), api.DeviceBuffer(cells), api.DeviceBuffer((4 * m + 5) * 32)
        up += [d_adv, d_sel, d_pub]
        check(lib.vdb_memset_dev(d_adv.ptr, 0xA5, ctypes.c_size_t(cells * 32)))
        check(lib.vdb_memset_dev(d_sel.ptr, 0xFF, ctypes.c_size_t(cells)))
        run = lambda: check(lib.vdb_wit_ann_write_dev(d_lc.ptr, d_ld.ptr, d_roots.ptr, K, s["c"], s["n_c"], s["n_db"], s["dim"], g_c, g_db, d_new.ptr, api._p(idx),
                                                      api._p(dbi), m, d_adv.ptr, d_sel.ptr, d_pub.ptr))
        run()
        api.sync()
        out = [d_adv.download((cells, 4)), d_sel.download((cells,), dtype=np.uint8), d_pub.download((4 * m + 5, 4)), d_lc.download(levels_c.shape),
               d_ld.download(levels_db.shape)]
        if profile:
            d_lc.upload(levels_c)
            d_ld.upload(levels_db)
            api.profile_begin(deferred=True)
            run()
            api.sync()
            out.append({name: int(v["launches"]) for name, v in api.profile_end().items()})
        return out
    finally:
        for b in up:
            b.free()


# ---------------------------------------------------------------------------------------------------------------- streams and trees
@pytest.mark.parametrize("name", sorted(AW.SHAPES))
def test_entry_points_write_the_models_stream_and_leave_the_models_trees(api, O, name):
    s = _case(O, name)
    m, K, k = s["m"], s["K"], len(s["slots"])
    stream, flags, pub, lc, ld = _write_dev(api, s)
    assert stream.shape == m["advice"].shape
    bad = np.flatnonzero((stream != m["advice"]).any(axis=1))
    assert bad.size == 0, f"first differing advice cells {bad[:5]} of {stream.shape[0]} (blocks {m['regions']})"
    assert np.array_equal(flags & 1, m["selectors"]) and not (flags & ~np.uint8(3)).any()
    # the flag bytes: outside the two update blocks the model's (a selection's leading zero is not flagged by the generator, as in the
    # query circuit); E's are those of the block emitted alone, cell for cell; inside E_db the gate bits above, every level's bytes those
    # of a level of E (one template), one flag pattern for every node hash of the growth block, and the single cells below
    d_c, g_c, d_db, g_db = s["shape"]
    r, u, udb = m["regions"], m["update"], m["update_db"]
    alone = api.wit_merkle_update(s["before"]["c"], s["n_c"], s["new"], s["slots"], selectors=True, grow=g_c)
    assert np.array_equal(flags[r["update"]:r["update_db"]], alone["flags"]) and np.array_equal(stream[r["update"]:r["update_db"]], alone["stream"])
    assert np.array_equal(lc, alone["levels"])
    outside = np.ones(flags.shape[0], dtype=bool)
    outside[r["update"]:r["new_roots"]] = False
    assert np.array_equal(flags[outside], m["flags"][outside]) and not flags[:K + 2].any()
    level_cells = 4 + 16 + 4506 + 16 + 4506                  # assert_bit, two selects, H old, two selects, H new
    e0 = r["update"] + u["regions"][0]["levels"][0]
    for reg in udb["regions"]:
        assert len(reg["levels"]) == d_db
        for lv in reg["levels"]:
            assert np.array_equal(flags[r["update_db"] + lv:r["update_db"] + lv + level_cells], flags[e0:e0 + level_cells]), lv
    if g_db:
        hashes = [r["update_db"] + x for x in udb["growth"]["z"] + udb["growth"]["r"]]
        assert len(hashes) == d_db - 1 + g_db and all(np.array_equal(flags[h:h + 4506], flags[e0 + 20:e0 + 20 + 4506]) for h in hashes)
        assert flags[r["update_db"] + udb["growth"]["r0"]] == 0 and flags[r["update_db"] + udb["growth"]["z0"]] == 2
    assert not flags[r["update_db"]:r["update_db"] + udb["n_in"]].any(), "E_db's assigned witnesses"
    assert not flags[[r["update_db"] + x for x in udb["carried"]]].any(), "a carried leaf is a plain witness cell"
    assert (flags[[r["update_db"] + x for x in udb["constants"]]] == 2).all()
    assert np.array_equal(pub, m["public"]) and pub.shape[0] == 4 * k + 5
    assert np.array_equal(lc, MU.flat_levels(s["tree"])) and np.array_equal(ld, MU.flat_levels(s["tree_db"]))
    assert np.array_equal(ld, api.merkle_tree_build(s["db2"])), "the database tree the call leaves is the fresh build over the updated rows"
    host = api.wit_ann_write(s["before"]["c"], s["before"]["db"], s["ix"]["roots"][:K + 1], s["c"], s["n_c"], s["n_db"], s["new"], s["slots"], s["db_idx"],
                             selectors=True)
    assert np.array_equal(host["stream"], stream) and np.array_equal(host["flags"], flags) and np.array_equal(host["public"], pub)
    assert np.array_equal(host["levels_c"], lc) and np.array_equal(host["levels_db"], ld) and host["input_cells"] == K + 2
    assert (host["update_base"], host["update_db_base"], host["grow_c"], host["grow_db"]) == (r["update"], r["update_db"], g_c, g_db)
    own, app = api.ann_write_db_indices(AN.select_cluster(s["db"], s["ids"], s["c"])[1], s["slots"], s["n_db"])
    assert own.tolist() == s["db_idx"] and app == s["appends"]
    # the trees as the library grows them are the model's
    assert np.array_equal(api.merkle_tree_grow(s["before"]["c0"], s["n_c"], g_c), s["before"]["c"])
    assert np.array_equal(api.merkle_tree_grow(s["before"]["db0"], s["n_db"], g_db), s["before"]["db"])


def test_three_windowed_calls_write_the_bytes_of_one(api, O):
    from halo2_vectordb_amd._lib import check
    lib = api.init()
    s = _case(O, "both_grow")
    m, K = s["m"], s["K"]
    want, pub, r, udb = m["advice"], m["public"], m["regions"], m["update_db"]
    d_c, g_c, d_db, g_db = s["shape"]
    assert (g_c, g_db) == (1, 1)
    cells = want.shape[0]
    lk = np.zeros((0, 4), dtype=np.uint64)
    idx, dbi = np.ascontiguousarray(s["slots"], dtype=np.uint64), np.ascontiguousarray(s["db_idx"], dtype=np.uint64)
    up = []
    try:
        d_roots, d_new, d_pub = _dev(api, up, s["ix"]["roots"][:K + 1]), _dev(api, up, s["new"]), _dev(api, up, np.zeros_like(pub))
        carried = r["update_db"] + udb["carried"][0]
        # between E and E_db | inside a hash of E_db's growth block; at the carried cell | between E_db and F; behind the carried cell |
        # inside a level of E_db; inside E's leaf sponge | inside R_0 / Z_0 of E_db
        for cuts in ((r["update_db"], r["update_db"] + udb["growth"]["r"][0] + 40), (carried, r["new_roots"]),
                     (carried + 1, r["update_db"] + udb["regions"][0]["levels"][1] + 25), (r["update"] + m["update"]["n_in"] + 9500, r["update_db"] + udb["n_in"])):
            edges, parts = (0,) + cuts + (cells,), []
            assert list(edges) == sorted(set(edges))
            for lo, hi in zip(edges[:-1], edges[1:]):
                window = (lo, hi, 0, 0)
                d_lc, d_ld = _dev(api, up, s["before"]["c"]), _dev(api, up, s["before"]["db"])     # every call starts from the trees before the batch
                run = lambda d_adv, d_lk: check(lib.vdb_wit_ann_write_dev(d_lc.ptr, d_ld.ptr, d_roots.ptr, K, s["c"], s["n_c"], s["n_db"], DIM, g_c, g_db, d_new.ptr,
                                                                          api._p(idx), api._p(dbi), len(idx), d_adv.ptr, None, d_pub.ptr))
                g_adv, _ = _windowed(api, lib, check, want, lk, window, run)
                _check_window(want, lk, g_adv, lk, window, (cuts, window))
                assert np.array_equal(d_pub.download(pub.shape), pub), (cuts, window)
                assert np.array_equal(d_lc.download(s["before"]["c"].shape), MU.flat_levels(s["tree"])), (cuts, window)
                assert np.array_equal(d_ld.download(s["before"]["db"].shape), MU.flat_levels(s["tree_db"])), (cuts, window)
                parts.append(g_adv[lo:hi])
            assert len(parts) == 3 and np.array_equal(np.concatenate(parts), want), cuts
    finally:
        for b in up:
            b.free()


def test_launch_list_depends_on_neither_K_nor_m_and_refused_arguments_launch_nothing(api, O):
    from halo2_vectordb_amd._lib import check
    lib = api.init()
    counts = {}
    # both trees double and d_c + d_db = 6 in all four: K = 1, sizes (4,): 4 -> 5 | 4 -> 5 (d 3, 3); K = 3, sizes (2, 3, 3): 2 -> 3 | 8 -> 9 (d 2, 4)
    counts["K1_m1"] = _write_dev(api, _case(O, "both_grow", sizes=(4,), slots=[4]), profile=True)[5]
    counts["K1_m3"] = _write_dev(api, _case(O, "both_grow", sizes=(4,), slots=[4, 0, 4]), profile=True)[5]
    counts["K3_m1"] = _write_dev(api, _case(O, "both_grow", sizes=(2, 3, 3), slots=[2]), profile=True)[5]
    counts["K3_m3"] = _write_dev(api, _case(O, "both_grow", sizes=(2, 3, 3), slots=[2, 0, 2]), profile=True)[5]
    counts["K2_m1"] = _write_dev(api, _case(O, "both_grow"), profile=True)[5]                                        # 2 -> 3 | 4 -> 5: d_c 2, d_db 3
    counts["flat"] = _write_dev(api, _case(O, "flat"), profile=True)[5]                                              # d_c 2, d_db 3, no growth
    assert counts["K1_m1"] == counts["K1_m3"] == counts["K3_m1"] == counts["K3_m3"], counts
    want = dict(k_annu_header=1, k_annu_indicator=1, k_nv_select=1, k_mk_leaf_states=4, k_mk_leaf_trace=4, k_mku_touchers=2, k_mku_level=6,
                k_mku_grow_trace=2, k_mku_writeback=2, k_mku_inputs=2, k_mku_level_trace=2, k_mku_index=2, k_annu_new_roots=1, k_annw_public=1, k_inv_fixup=1)
    assert counts["K1_m1"] == want, counts
    assert counts["K2_m1"] == dict(want, k_mku_level=5), counts
    flat = dict(want, k_mku_level=5)
    del flat["k_mku_grow_trace"]
    assert counts["flat"] == flat, counts
    # refusals (K, c, n_c, n_db, g_c, g_db, idx, db_idx).  The update's: c >= K, K = 0, K too large, a slot above the fill at its turn, a
    # slot outside the grown tree, no write, depth 0, d + g > 30.  The write's own: an empty database, a cluster larger than its database,
    # an append that does not go to the database's fill (beyond it, and onto an occupied slot), a replacement at or beyond the fill, a
    # write to a member the batch appended at another slot than that member's, a g_db that is too small and one that is too large
    s = _case(O, "both_grow")
    old = api.ann_index_build(s["db"], s["ids"], s["cent"])
    up = []
    try:
        d_lc, d_ld, d_roots, d_new = _dev(api, up, s["before"]["c"]), _dev(api, up, s["before"]["db"]), _dev(api, up, s["ix"]["roots"][:3]), _dev(api, up, s["new"])
        d_out = api.DeviceBuffer(1 << 16)
        up.append(d_out)
        check(lib.vdb_memset_dev(d_out.ptr, 0xA5, ctypes.c_size_t(1 << 16)))
        api.sync()
        api.profile_begin(deferred=True)
        for K, c, n_c, n_db, g_c, g_db, idx, dbi in ((2, 2, 2, 4, 1, 1, [2], [4]), (0, 0, 2, 4, 1, 1, [2], [4]), (4097, 0, 2, 4, 1, 1, [2], [4]),
                                                     (2, 0, 2, 4, 1, 1, [3], [4]), (2, 0, 2, 4, 0, 1, [2], [4]), (2, 0, 2, 4, 1, 1, [], []),
                                                     (2, 0, 1, 4, 0, 0, [0], [0]), (2, 0, 2, 4, 30, 1, [2], [4]),
                                                     (2, 0, 2, 0, 1, 0, [2], [0]), (2, 0, 5, 4, 0, 1, [5], [4]), (2, 0, 2, 4, 1, 1, [2], [5]),
                                                     (2, 0, 2, 4, 1, 1, [2], [3]), (2, 0, 2, 4, 0, 0, [1], [4]), (2, 0, 2, 4, 0, 0, [1], [7]),
                                                     (2, 0, 2, 4, 1, 1, [2, 2], [4, 1]), (2, 0, 2, 4, 1, 0, [2], [4]), (2, 0, 2, 4, 1, 2, [2], [4])):
            uidx, udbi = np.ascontiguousarray(idx + [0], dtype=np.uint64), np.ascontiguousarray(dbi + [0], dtype=np.uint64)
            with pytest.raises(api.VdbError) as e:
                check(lib.vdb_wit_ann_write_dev(d_lc.ptr, d_ld.ptr, d_roots.ptr, K, c, n_c, n_db, DIM, g_c, g_db, d_new.ptr, api._p(uidx), api._p(udbi), len(idx),
                                                d_out.ptr, None, d_out.at(1 << 15)))
            assert e.value.code == -3, (K, c, n_c, n_db, g_c, g_db, idx, dbi)
        # the two limits.  2^34 cells: 16 replacements at the largest dim at which the plain update still fits, so E alone fits and E + E_db
        # does not (tests/test_ann_write_cpu.py finds the dim and holds the size calls to it); the plain call's own layout accepts the
        # shape.  And section 4h's batch limit: 4,097 writes.  Both are refused before any pointer is used
        from test_ann_write_cpu import cell_limit_dim
        big, _ = cell_limit_dim(lib, 2, 4, 16)
        assert lib.vdb_wit_ann_update_size(2, 4, big, 16, 0, None, None, None) == 0
        for dim, k in ((big, 16), (DIM, 4097)):
            zeros = np.zeros(k + 1, dtype=np.uint64)
            with pytest.raises(api.VdbError) as e:
                check(lib.vdb_wit_ann_write_dev(d_lc.ptr, d_ld.ptr, d_roots.ptr, 2, 0, 4, 8, dim, 0, 0, d_new.ptr, api._p(zeros), api._p(zeros), k, d_out.ptr, None,
                                                d_out.at(1 << 15)))
            assert e.value.code == -3, (dim, k)
        # the index after the batch: a hole, growths that are not the smallest
        for slots, g_c, g_db in (([3], None, None), ([2], 0, None), ([2], 2, None), ([2], None, 0), ([2], None, 2), ([0], 1, None), ([0], None, 1)):
            with pytest.raises(api.VdbError) as e:
                api.ann_index_write(old, 0, MU.flat_levels(s["tree"]), MU.flat_levels(s["tree_db"]), s["new"][:1], slots, grow_c=g_c, grow_db=g_db)
            assert e.value.code == -3, (slots, g_c, g_db)
        api.sync()
        assert api.profile_end() == {}
        assert (d_out.download((1 << 16,), dtype=np.uint8) == 0xA5).all()
        assert np.array_equal(d_lc.download(s["before"]["c"].shape), s["before"]["c"]) and np.array_equal(d_ld.download(s["before"]["db"].shape), s["before"]["db"])
    finally:
        for b in up:
            b.free()


def test_a_batch_beyond_one_workgroup_of_the_public_row(api, O):
    """67 replacements into a cluster of two: 4 m + 5 = 273 public values, more than the 256 lanes of one workgroup of k_annw_public, and
    more than 64 updates in both update blocks; every slot is written many times.  Streams, public row and trees against the model"""
    slots = [int(x) for x in np.random.default_rng(3).integers(0, 2, 67)]
    s = _case(O, "flat", sizes=(2, 2), slots=slots, block_flags=False)
    m = s["m"]
    assert s["shape"] == (1, 0, 2, 0) and s["appends"] == 0 and set(s["db_idx"]) == {0, 2}
    stream, flags, pub, lc, ld = _write_dev(api, s)
    assert np.array_equal(stream, m["advice"]) and np.array_equal(flags & 1, m["selectors"]) and not (flags & ~np.uint8(3)).any()
    assert pub.shape[0] == 273 and np.array_equal(pub, m["public"])
    assert np.array_equal(lc, MU.flat_levels(s["tree"])) and np.array_equal(ld, MU.flat_levels(s["tree_db"]))
    assert np.array_equal(ld, api.merkle_tree_build(s["db2"]))


# ---------------------------------------------------------------------------------------------------------------- the map and the proof
def _index_and_hot_path(s, k=13, **kw):
    from halo2_vectordb_amd.pipeline import AnnIndex, AnnWriteHotPath
    index = AnnIndex(len(s["ids"]), s["dim"], s["K"], s["f"]["db"], s["ids"], s["f"]["cent"], P=P, L=13)
    return index, AnnWriteHotPath(index, s["c"], (s["slots"], s["f"]["new"]), k=k, tau=TAU, **kw)


@pytest.mark.parametrize("name", ["both_grow", "append_then_replace"])
def test_device_placed_map_is_the_host_builders(api, O, name):
    from halo2_vectordb_amd.rounds import ProverRounds
    index, hp = _index_and_hot_path(_case(O, name))
    maps = {}
    try:
        hp.setup()
        for on_dev in (True, False):
            pr = ProverRounds(hp)
            pr.map_on_device = on_dev
            d_flags = hp.keygen_flags()
            cm = pr.circuit_map(d_flags)
            d_flags.free()
            maps[on_dev] = (np.array(cm.copy_of), np.array(cm.const_idx), np.asarray(cm.gate).copy(), [int(v) for v in cm.consts], np.array(cm.lookup_src),
                            np.array(cm.asserted), pr.public_cells)
            if on_dev:
                cm.free()
        d, h = maps[True], maps[False]
        assert d[6] == h[6] and len(h[6]) == 4 * hp.m + 5
        for i in (0, 2, 4, 5):
            assert np.array_equal(d[i], h[i]), i
        val = lambda x: np.where(x[1] >= 0, np.asarray(x[3] + [0], dtype=object)[np.maximum(x[1], -1)], -1)
        assert np.array_equal(val(d), val(h))
    finally:
        hp.free()
        index.free()


@pytest.fixture(scope="module")
def proved(api, O):
    """one AnnWriteHotPath with its keys and its proof, shared by the tests below"""
    from halo2_vectordb_amd.rounds import ProverRounds
    s = _case(O, PROVED)
    index, hp = _index_and_hot_path(s)
    hp.setup()
    pr = ProverRounds(hp).keygen()
    hp._witness()
    api.sync()
    stream = hp.d_stream.download((hp.n_cells, 4))
    out = pr.prove(None, seed=23)
    yield dict(s=s, index=index, hp=hp, pr=pr, out=out, stream=stream)
    pr.free()
    hp.free()
    index.free()


def test_hot_path_proves_the_models_batch_and_changed_instances_are_rejected(api, O, proved):
    from halo2_vectordb_amd import verifier
    s, hp, pr, out = proved["s"], proved["hp"], proved["pr"], proved["out"]
    m, k = s["m"], len(s["slots"])
    assert hp.n_cells == m["advice"].shape[0] and hp.n_in == s["K"] + 2 and hp.n_lookup == 0 and np.array_equal(hp.bp, m["break_points"])
    assert (hp.depth, hp.grow, hp.depth_db, hp.grow_db) == s["shape"] and hp.n_input_rows() == k and hp.appends == s["appends"]
    assert (hp.update_base, hp.update_db_base) == (m["regions"]["update"], m["regions"]["update_db"]) and hp.db_indices.tolist() == s["db_idx"]
    assert pr.keygen_report.violations() == 0, pr.keygen_report.as_dict()
    assert pr.mock_check().violations() == 0
    assert np.array_equal(proved["stream"], m["advice"])
    res = hp.results()
    assert np.array_equal(np.concatenate([np.stack(res[:3]), np.stack(res[3:7], axis=1).reshape(-1, 4), np.stack(res[7:])]), m["public"])
    assert np.array_equal(res[1], proved["index"].roots()[-1])
    lp_db = api.merkle_levels(s["n_db"])[0]
    assert np.array_equal(res[0], proved["index"].database_tree().download((2 * lp_db, 4))[-2]), "database_root_old is the index's database tree's"
    assert TM.to_ints(res[3]) == s["slots"] and TM.to_ints(res[4]) == s["db_idx"] and not res[5][0].any()
    assert np.array_equal(hp.d_levels.download((2 * hp.lp, 4)), MU.flat_levels(s["tree"]))
    assert np.array_equal(hp.d_levels_db.download((2 * hp.lp_db, 4)), MU.flat_levels(s["tree_db"]))
    want = TM.to_ints(m["public"])
    assert out["instances"] == want and len(want) == 4 * k + 5
    vk = verifier.VerifyingKey.from_prover(pr, out["opened"])
    assert verifier.verify(out["proof"], want, vk)
    for at in range(len(want)):                                  # the four roots, c, idx, db_idx and both leaves
        wrong = list(want)
        wrong[at] = (wrong[at] + 1) % O.R_MOD
        assert not verifier.verify(out["proof"], wrong, vk), at


def test_cells_tampered_in_hbm_fail_the_mock_stage(api, O, proved):
    from halo2_vectordb_amd import circuit_sym as CS
    s, hp, pr = proved["s"], proved["hp"], proved["pr"]
    hp._witness()
    api.sync()
    stream = hp.d_stream.download((hp.n_cells, 4))
    assert np.array_equal(stream, proved["stream"])
    lay = CS.ann_write_layout(s["K"], hp.m, DIM, hp.depth, hp.grow, hp.depth_db, hp.grow_db)
    u, udb = lay["update_layout"], lay["update_db_layout"]
    one = O.fr_from_ints([1])
    d_flags = api.DeviceBuffer(hp.n_cells)
    try:
        d_flags.upload(np.asarray(pr.circuit.gate).astype(np.uint8))
        assert pr.mock_check(d_flags).violations() == 0              # the witness as it lies in HBM, not emitted again
        carried = [lay["update_db"] + udb["block"][j] for j in range(hp.m)]
        old_db = [lay["update_db"] + udb["old_leaf"] + j for j in range(hp.m)]
        old_c = [lay["update"] + u["old_leaf"] + j for j in range(hp.m)]
        # every carried leaf and old-leaf cell of E_db, E's old leaves, R_0 of E_db, the new cluster root's select
        for cell in carried + old_db + old_c + [lay["update_db"] + udb["r0"], lay["new_roots"] + 8 * s["c"] + 7]:
            hp.d_stream.upload(O.fr_add(stream[cell:cell + 1], one), offset=cell * 32)
            rep = pr.mock_check(d_flags)
            hp.d_stream.upload(np.ascontiguousarray(stream[cell:cell + 1]), offset=cell * 32)
            assert rep.violations() >= 1, (cell, rep.as_dict())
        assert pr.mock_check(d_flags).violations() == 0
    finally:
        d_flags.free()


def test_another_indexs_database_tree_breaks_the_old_leaf_tie_alone(api, O):
    """a replacement against the database tree of an index over OTHER rows: every gate holds (the trees of a shape are interchangeable),
    the one copy that fails ties E_db's old leaf to E's; and a database slot that is not the member's, over the right tree, the same"""
    from halo2_vectordb_amd import circuit_sym as CS
    from halo2_vectordb_amd.pipeline import AnnIndex
    from halo2_vectordb_amd.rounds import ProverRounds
    s = _case(O, "flat")
    other = AnnIndex(len(s["ids"]), DIM, s["K"], _rows(96, len(s["ids"]), DIM), s["ids"], s["f"]["cent"], P=P, L=13)
    d_c, g_c, d_db, g_db = s["shape"]
    lay = CS.ann_write_layout(s["K"], 1, DIM, d_c, g_c, d_db, g_db)
    tie = (lay["update_db"] + lay["update_db_layout"]["old_leaf"], lay["update"] + lay["update_layout"]["old_leaf"])
    try:
        for kw in (dict(), dict(levels_db=other.database_tree()), dict(db_indices=[3])):
            index, hp = _index_and_hot_path(s, **kw)
            pr = ProverRounds(hp.setup()).keygen()
            try:
                rep = pr.keygen_report
                if not kw:
                    assert rep.violations() == 0, rep.as_dict()
                else:
                    assert rep.violations() == rep.copies_unequal == 1 and (int(rep.first_copy), int(pr.circuit.copy_of[rep.first_copy])) == tie, rep.as_dict()
                    with pytest.raises(ValueError):              # written() adopts the proof's tree: not one that is not the database's
                        index.written(hp)
                with pytest.raises(ValueError):
                    other.written(hp)                            # nor a hot path built on another index
            finally:
                pr.free()
                hp.free()
                index.free()
    finally:
        other.free()


# ---------------------------------------------------------------------------------------------------------------- the resident index
@pytest.mark.parametrize("name", sorted(AW.SHAPES))
def test_written_index_is_a_fresh_build_over_the_updated_database_with_its_database_tree(api, O, name):
    s = _case(O, name)
    K, c = s["K"], s["c"]
    old = api.ann_index_build(s["db"], s["ids"], s["cent"])
    got = api.ann_index_write(old, c, MU.flat_levels(s["tree"]), MU.flat_levels(s["tree_db"]), s["new"], s["slots"])
    _same_index(got, api.ann_index_build(s["db2"], s["ids2"], s["cent"]), K)
    assert np.array_equal(got["roots"][-1], s["m"]["public"][-1]), "the written index's root is the circuit's public index_root_new"
    assert np.array_equal(got["db_tree"], api.merkle_tree_build(s["db2"])) and np.array_equal(got["db_tree"][-2], s["m"]["public"][-2])
    assert np.array_equal(got["db_tree"], api.ann_index_db_tree(got["forest"], np.bincount(s["ids2"]), got["slots"])), "what database_tree() would have built"
    d_c, g_c, d_db, g_db = s["shape"]
    assert api.ann_index_write_layout(np.bincount(s["ids"]), c, s["slots"])[:3] == (s["appends"], g_c, g_db)


def test_written_keeps_both_objects_resident_and_the_chain_of_covers_holds(api, O, proved):
    """written(hp) against a fresh build, its database tree against merkle_tree_build and MerkleHotPath's root; AnnCoverHotPath is
    Mock-clean on the built index and on written(hp) and publishes the pairs of roots the write published"""
    from halo2_vectordb_amd.pipeline import AnnCoverHotPath, MerkleHotPath
    from halo2_vectordb_amd.rounds import ProverRounds
    s, hp, index = proved["s"], proved["hp"], proved["index"]
    K, dim = s["K"], s["dim"]
    made = []
    try:
        before = [b.download((b.nbytes,), dtype=np.uint8) for b in (index.d_grouped, index.d_slots, index.d_offsets, index.d_forest, index.d_roots)]
        hp._witness()
        api.sync()
        res = hp.results()
        ix2 = index.written(hp)
        made.append(ix2)
        _same_index(_resident(ix2, K, dim), api.ann_index_build(s["db2"], s["ids2"], s["cent"]), K)
        assert np.array_equal(ix2.qvec, s["db2"]) and np.array_equal(ix2.cluster_ids, s["ids2"]) and ix2.n == len(s["ids2"])
        made_tree = ix2.d_db_tree
        assert made_tree is not None and ix2.database_tree() is made_tree, "the tree is the proof's: database_tree() builds nothing"
        lp2 = api.merkle_levels(ix2.n)[0]
        tree2 = ix2.database_tree().download((2 * lp2, 4))
        assert np.array_equal(tree2, api.merkle_tree_build(s["db2"])) and np.array_equal(tree2[-2], res[7])
        mk = MerkleHotPath(n=ix2.n, dim=dim, k=13, P=P, tau=TAU, vectors=api.dequantize(s["db2"], P)).setup()
        made.append(mk)
        mk._witness()
        api.sync()
        assert np.array_equal(np.asarray(mk.results()).reshape(-1, 4)[-1], res[7]), "the root MerkleHotPath publishes for the updated rows"
        for ix, pair in ((index, res[:2]), (ix2, res[7:])):
            cover = AnnCoverHotPath(ix, k=12, L=L, tau=TAU).setup()
            made.append(cover)
            pr = ProverRounds(cover).keygen()
            made.append(pr)
            assert pr.keygen_report.violations() == 0, pr.keygen_report.as_dict()
            cover._witness()
            api.sync()
            assert np.array_equal(np.stack(cover.results()[:2]), np.stack(pair)), "the cover publishes the pair of roots the write published"
        after = [b.download((b.nbytes,), dtype=np.uint8) for b in (index.d_grouped, index.d_slots, index.d_offsets, index.d_forest, index.d_roots)]
        assert all(np.array_equal(x, y) for x, y in zip(before, after)), "the old index's buffers are only read"
    finally:
        for x in reversed(made):
            x.free()


def test_the_other_hot_paths_and_a_second_linked_write_run_on_the_written_index(api, O, proved):
    """one small call of each on written(hp): a query, a read, a plain update, a move and a second linked write, which starts from the
    pair of roots the first one published"""
    from halo2_vectordb_amd.pipeline import AnnMoveHotPath, AnnQueryHotPath, AnnUpdateHotPath, AnnWriteHotPath, ReadHotPath
    s, hp = proved["s"], proved["hp"]
    c, dim = s["c"], s["dim"]
    made = []
    try:
        hp._witness()
        api.sync()
        res = hp.results()
        ix2 = proved["index"].written(hp)
        made.append(ix2)
        n_c2 = int(ix2.sizes[c])
        assert n_c2 == s["n_c"] + s["appends"]
        q = AnnQueryHotPath(ix2, s["f"]["cent"][c] + 0.25, cluster=c, k=13, P=P, L=L, tau=TAU).setup()
        made.append(q)
        q._witness()
        api.sync()
        assert np.array_equal(q.results()[3], res[8])
        rd = ReadHotPath(n=n_c2, dim=dim, m=1, k=13, P=P, tau=TAU, vectors=api.dequantize(ix2.members(c), P), levels=ix2.levels(c), reads=[n_c2 - 1]).setup()
        made.append(rd)
        rd._witness()
        api.sync()
        assert np.array_equal(rd.results()[0], ix2.roots()[1 + c]) and np.array_equal(np.asarray(rd.results()[3]).reshape(-1, 4), s["new"][-1])
        au = AnnUpdateHotPath(ix2, c, ([0], _rows(71, 1, dim)), grow=None, k=13, tau=TAU).setup()
        made.append(au)
        au._witness()
        api.sync()
        assert np.array_equal(au.results()[0], res[8])
        mv = AnnMoveHotPath(ix2, c, 1 - c, [n_c2 - 1], k=13, tau=TAU).setup()
        made.append(mv)
        mv._witness()
        api.sync()
        assert np.array_equal(mv.results()[0], res[8]) and np.array_equal(mv.results()[4][0], res[6][-1]), "the appended leaf moves on"
        new2 = _rows(72, 2, dim)
        w2 = AnnWriteHotPath(ix2, c, ([n_c2 - 1, n_c2], new2), k=13, tau=TAU).setup()
        made.append(w2)
        w2._witness()
        api.sync()
        r2 = w2.results()
        assert np.array_equal(np.stack(r2[:2]), np.stack(res[7:])), "the second write starts from the pair the first one published"
        assert w2.db_indices.tolist() == [s["n_db"], s["n_db"] + 1], "the appended member's database slot is read from the written index's slots"
        ix3 = ix2.written(w2)
        made.append(ix3)
        db3, ids3 = AU.updated_database(s["db2"], s["ids2"], c, [n_c2 - 1, n_c2], O.quantize(new2, P))
        _same_index(_resident(ix3, s["K"], dim), api.ann_index_build(db3, ids3, s["cent"]), s["K"])
        assert np.array_equal(ix3.database_tree().download((2 * api.merkle_levels(ix3.n)[0], 4)), api.merkle_tree_build(db3))
        assert np.array_equal(ix3.roots()[-1], r2[8])
    finally:
        for x in reversed(made):
            x.free()
