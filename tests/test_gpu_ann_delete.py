"""Deletes proved against the committed index root on the GPU (pipeline.AnnDeleteHotPath, AnnIndex.removed; vdb_wit_ann_delete*,
vdb_ann_index_remove_dev).  The streams are tests/ann_delete_model.py's bit for bit (tests/test_ann_delete_cpu.py holds that model against
the index model first); host and device forms, rank windows cut at a carried cell, inside block S and between S and F, the launch list,
refused arguments, the index after the batch against a fresh build over its compacted database, chained batches, the Mock stage, the
whole proof, changed instances, cells tampered in HBM, the binding of the cluster's tree to its root, a dropped half that is not empty,
and a query and a read against the removed index."""
import ctypes

import numpy as np
import pytest

import ann_delete_model as AD
import ann_model as AN
import ann_update_model as AU
import merkle_update_model as MU
import topk_model as TM
from test_gpu_batch_query import _dev
from test_gpu_rounds import TAU
from test_gpu_sweep import _check_window, _windowed

pytestmark = pytest.mark.gpu
P, L, DIM = 48, 12, 3


@pytest.fixture(scope="module")
def api():
    from halo2_vectordb_amd import api as a
    a.init(0)
    return a


def _rows(seed, n, dim):
    return np.random.default_rng(seed).integers(0, 219, size=(n, dim)).astype(np.float64)


_MODELS = {}


def _case(O, name, seed=60, slots=None, c=None, sizes=None):
    """-> dict(f64 rows, quantized rows, the index model before the batch, the cluster's tree before the batch (device layout), the model
    and its tree after the batch, at its old size); computed once per case and left unchanged"""
    key = (name, None if slots is None else tuple(slots), c, sizes)
    if key not in _MODELS:
        sizes0, c0, slots0 = AD.SHAPES[name]
        sizes, c, slots = sizes0 if sizes is None else sizes, c0 if c is None else c, slots0 if slots is None else slots
        ids = AD.ids_of(sizes)
        K = len(sizes)
        f = dict(db=_rows(seed, len(ids), DIM), cent=_rows(seed + 1, K, DIM))
        db, cent = O.quantize(f["db"], P), O.quantize(f["cent"], P)
        ix = AN.index_model(O, db, ids, cent)
        tree = MU.build_tree(O, AN.select_cluster(db, ids, c)[0])
        before = MU.flat_levels(tree)
        m = AD.delete_model(O, ix["roots"][:K + 1], c, tree, slots, plan_k=13)
        _MODELS[key] = dict(f=f, db=db, cent=cent, ids=ids, K=K, dim=DIM, c=c, slots=list(slots), ix=ix, before=before, m=m, tree=tree, n_c=int(sizes[c]))
    return _MODELS[key]


def _delete_dev(api, s, levels=None, profile=False):
    """vdb_wit_ann_delete_dev into poisoned buffers -> (stream, flags, public, levels after[, launches per kernel of a second run])"""
    from halo2_vectordb_amd._lib import check
    lib = api.init()
    m, K = len(s["slots"]), s["K"]
    cells, n_in, ub, sb, sh = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint()
    check(lib.vdb_wit_ann_delete_size(K, s["n_c"], s["dim"], m, ctypes.byref(cells), ctypes.byref(n_in), ctypes.byref(ub), ctypes.byref(sb), ctypes.byref(sh)))
    cells, idx = cells.value, np.ascontiguousarray(s["slots"], dtype=np.uint64)
    levels = s["before"] if levels is None else levels
    up = []
    try:
        d_lv, d_roots = _dev(api, up, levels), _dev(api, up, s["ix"]["roots"][:K + 1])
        d_adv, d_sel, d_pub = api.DeviceBuffer(cells * 32), api.DeviceBuffer(cells), api.DeviceBuffer((4 * m + 3) * 32)
        up += [d_adv, d_sel, d_pub]
        check(lib.vdb_memset_dev(d_adv.ptr, 0xA5, ctypes.c_size_t(cells * 32)))
        check(lib.vdb_memset_dev(d_sel.ptr, 0xFF, ctypes.c_size_t(cells)))
        run = lambda: check(lib.vdb_wit_ann_delete_dev(d_lv.ptr, d_roots.ptr, K, s["c"], s["n_c"], s["dim"], api._p(idx), m, d_adv.ptr, d_sel.ptr, d_pub.ptr))
        run()
        api.sync()
        out = [d_adv.download((cells, 4)), d_sel.download((cells,), dtype=np.uint8), d_pub.download((4 * m + 3, 4)), d_lv.download(levels.shape)]
        if profile:
            d_lv.upload(levels)
            api.profile_begin(deferred=True)
            run()
            api.sync()
            out.append({name: int(v["launches"]) for name, v in api.profile_end().items()})
        return out
    finally:
        for b in up:
            b.free()


# ---------------------------------------------------------------------------------------------------------------- streams and tree
@pytest.mark.parametrize("name", sorted(AD.SHAPES))
def test_entry_points_write_the_models_stream_and_leave_the_models_tree(api, O, name):
    s = _case(O, name)
    m, K, c = s["m"], s["K"], s["c"]
    stream, flags, pub, levels1 = _delete_dev(api, s)
    assert stream.shape == m["advice"].shape
    bad = np.flatnonzero((stream != m["advice"]).any(axis=1))
    assert bad.size == 0, f"first differing advice cells {bad[:5]} of {stream.shape[0]} (blocks {m['regions']})"
    assert np.array_equal(flags & 1, m["selectors"]) and not (flags & ~np.uint8(3)).any()
    # the flag bytes: outside E' and S the model's (the selection's leading zero is not flagged by the generator, as in the query circuit);
    # inside them the gate bits above, the single cells below, and one flag pattern for every node hash, wherever it lies
    r, u = m["regions"], m["update"]
    outside = np.ones(flags.shape[0], dtype=bool)
    outside[r["update"]:r["new_roots"]] = False
    diff = np.flatnonzero((flags != m["flags"]) & outside)
    assert diff.size == 0 and not flags[:K + 2].any(), (diff[:8], r)
    depth = len(s["tree"]) - 1
    hashes = [r["update"] + lv + off for reg in u["regions"] for lv in reg["levels"] for off in (20, 20 + 4506 + 16)]
    hashes += [r["shrink"] + 2 + h * 4506 for h in range(depth - 1 + m["s"])] if m["s"] else []
    assert all(np.array_equal(flags[h:h + 4506], flags[hashes[0]:hashes[0] + 4506]) for h in hashes) and len(hashes) >= 4 * depth * len(s["slots"])
    assert not flags[[r["update"] + x for x in u["carried"]]].any(), "a carried leaf is a plain witness cell"
    assert (flags[[r["update"] + x for x in u["constants"]]] == 2).all()
    if m["s"]:
        assert flags[r["shrink"]] == 0 and flags[r["shrink"] + 1] == 2
    assert np.array_equal(pub, m["public"]) and pub.shape[0] == 4 * len(s["slots"]) + 3
    assert np.array_equal(levels1, MU.flat_levels(s["tree"]))
    host = api.wit_ann_delete(s["before"], s["ix"]["roots"][:K + 1], c, s["n_c"], s["dim"], s["slots"], selectors=True)
    assert np.array_equal(host["stream"], stream) and np.array_equal(host["flags"], flags) and np.array_equal(host["public"], pub)
    assert np.array_equal(host["levels"], levels1) and host["input_cells"] == K + 2 and host["update_base"] == r["update"]
    assert host["shrink_base"] == r["shrink"] and host["shrink"] == m["s"]


def test_two_windowed_calls_write_the_bytes_of_one(api, O):
    from halo2_vectordb_amd._lib import check
    lib = api.init()
    s = _case(O, "last_repeat")
    m, K = s["m"], s["K"]
    want, pub, r, u = m["advice"], m["public"], m["regions"], m["update"]
    assert m["s"] == 2
    cells = want.shape[0]
    lk = np.zeros((0, 4), dtype=np.uint64)
    idx = np.ascontiguousarray(s["slots"], dtype=np.uint64)
    up = []
    try:
        d_roots, d_pub = _dev(api, up, s["ix"]["roots"][:K + 1]), _dev(api, up, np.zeros_like(pub))
        # in front of and behind a carried cell of E', inside its inputs and a level; in S: between S_0 and Z_0, inside a Z hash, inside an
        # S hash; between S and F; the frame the call shares with the update: inside the header, inside an indicator block, between C and
        # D, inside F, near the end
        for cut in (r["update"] + u["carried"][1], r["update"] + u["carried"][2] + 1, r["update"] + u["n_in"] - 2, r["update"] + u["regions"][2]["levels"][1] + 25,
                    r["shrink"] + 1, r["shrink"] + 2 + 4506 + 31, r["new_roots"] - 4506 - 7, r["new_roots"],
                    2, r["indicator"] + 8 + 5, r["sponge_old"], r["new_roots"] + 11, cells - 3):
            halves = []
            for window in ((0, cut, 0, 0), (cut, cells, 0, 0)):
                d_lv = _dev(api, up, s["before"])                   # every call starts from the tree before the batch
                run = lambda d_adv, d_lk: check(lib.vdb_wit_ann_delete_dev(d_lv.ptr, d_roots.ptr, K, s["c"], s["n_c"], s["dim"], api._p(idx), len(idx),
                                                                           d_adv.ptr, None, d_pub.ptr))
                g_adv, _ = _windowed(api, lib, check, want, lk, window, run)
                _check_window(want, lk, g_adv, lk, window, (cut, window))
                assert np.array_equal(d_pub.download(pub.shape), pub), (cut, window)
                assert np.array_equal(d_lv.download(s["before"].shape), MU.flat_levels(s["tree"])), (cut, window)
                halves.append(g_adv)
            assert np.array_equal(np.concatenate([halves[0][:cut], halves[1][cut:]]), want), cut
    finally:
        for b in up:
            b.free()


def test_launch_list_depends_on_neither_K_nor_m_and_refused_arguments_launch_nothing(api, O):
    from halo2_vectordb_amd._lib import check
    lib = api.init()
    counts = {}
    counts["shrink_m1"] = _delete_dev(api, _case(O, "shrink"), profile=True)[4]                       # 5 -> 4: d = 3, s = 1
    counts["shrink_m2"] = _delete_dev(api, _case(O, "shrink", slots=[1, 3]), profile=True)[4]         # 5 -> 3: d = 3, s = 1
    counts["K1"] = _delete_dev(api, _case(O, "k1"), profile=True)[4]                                 # 3 -> 2: d = 2, s = 1
    counts["K3"] = _delete_dev(api, _case(O, "shrink", slots=[0], c=2), profile=True)[4]             # 3 -> 2 in cluster 2 of three
    counts["flat"] = _delete_dev(api, _case(O, "flat"), profile=True)[4]                             # 4 -> 3: d = 2, s = 0
    assert counts["shrink_m1"] == counts["shrink_m2"] and counts["K1"] == counts["K3"], counts
    want = dict(k_annu_header=1, k_annu_indicator=1, k_nv_select=1, k_mk_leaf_states=3, k_mk_leaf_trace=3, k_mku_touchers=1, k_mku_level=3,
                k_mku_writeback=1, k_mku_inputs=1, k_mku_level_trace=1, k_mku_index=1, k_annd_shrink_trace=1, k_annu_new_roots=1, k_annd_public=1,
                k_inv_fixup=1)
    assert counts["shrink_m1"] == want and counts["K1"] == dict(want, k_mku_level=2), counts
    no_s = dict(want, k_mku_level=2)
    del no_s["k_annd_shrink_trace"]
    assert counts["flat"] == no_s, counts
    # refusals: c >= K, K = 0, K too large, no delete, too many, emptying the cluster (m = n_c and m > n_c), a slot at the fill, a slot at
    # the fill at its turn, a tree of one leaf
    s = _case(O, "shrink")
    up = []
    try:
        d_lv, d_roots = _dev(api, up, s["before"]), _dev(api, up, s["ix"]["roots"][:4])
        d_out = api.DeviceBuffer(1 << 16)
        up.append(d_out)
        check(lib.vdb_memset_dev(d_out.ptr, 0xA5, ctypes.c_size_t(1 << 16)))
        api.sync()
        api.profile_begin(deferred=True)
        for K, c, n_c, idx in ((3, 3, 5, [0]), (0, 0, 5, [0]), (4097, 0, 5, [0]), (3, 0, 5, []), (3, 0, 5000, [0] * 2049), (3, 0, 5, [0] * 5), (3, 0, 2, [0] * 3),
                               (3, 0, 5, [5]), (3, 0, 5, [0, 4]), (3, 0, 5, [4, 3, 3]), (3, 0, 1, [0])):
            uidx = np.ascontiguousarray(idx + [0], dtype=np.uint64)
            with pytest.raises(api.VdbError) as e:
                check(lib.vdb_wit_ann_delete_dev(d_lv.ptr, d_roots.ptr, K, c, n_c, s["dim"], api._p(uidx), len(idx), d_out.ptr, None, d_out.at(1 << 15)))
            assert e.value.code == -3, (K, c, n_c, idx)
        api.sync()
        assert api.profile_end() == {}
        assert (d_out.download((1 << 16,), dtype=np.uint8) == 0xA5).all() and np.array_equal(d_lv.download(s["before"].shape), s["before"])
    finally:
        for b in up:
            b.free()


# ---------------------------------------------------------------------------------------------------------------- the index after the batch
def _same_index(got, want):
    for key in ("grouped", "slots", "offsets", "roots"):
        assert np.array_equal(got[key], want[key]), key
    assert np.array_equal(got["segments"], want["segments"]) and np.array_equal(got["forest"], want["forest"])


def _resident(ix, K, dim):
    n = ix.n
    return dict(grouped=ix.d_grouped.download((n, dim, 4)), slots=ix.d_slots.download((n,), dtype=np.uint32),
                offsets=ix.d_offsets.download((K + 1,), dtype=np.uint64), forest=ix.d_forest.download((ix.n_digests, 4)), segments=ix.segments, roots=ix.roots())


@pytest.mark.parametrize("name", sorted(AD.SHAPES))
def test_removed_index_is_a_fresh_build_over_its_compacted_database(api, O, name):
    s = _case(O, name)
    c, k = s["c"], len(s["slots"])
    old = api.ann_index_build(s["db"], s["ids"], s["cent"])
    got = api.ann_index_remove(old, c, MU.flat_levels(s["tree"]), s["slots"])
    n2 = s["db"].shape[0] - k
    assert got["grouped"].shape[0] == n2 and np.array_equal(got["slots"], np.arange(n2, dtype=np.uint32))
    ids2 = np.repeat(np.arange(s["K"]), np.diff(got["offsets"].astype(np.int64)))
    assert np.all(np.diff(ids2) >= 0)
    _same_index(got, api.ann_index_build(got["grouped"], ids2, s["cent"]))       # ... over the result's own grouped rows in order
    db2, want_ids = AD.compacted_database(s["db"], s["ids"], c, s["slots"])
    assert np.array_equal(got["grouped"], db2) and np.array_equal(ids2, want_ids), "position p holds original member origin[p]"
    assert np.array_equal(got["roots"][-1], s["m"]["public"][-1]), "the removed index's root is the circuit's public index_root_new"
    assert api.ann_index_remove_layout(np.diff(old["offsets"].astype(np.int64)), c, s["slots"])[0] == s["m"]["s"]


def test_chained_batches_on_resident_indices_and_the_old_index_stays(api, O):
    from halo2_vectordb_amd.pipeline import AnnDeleteHotPath, AnnIndex, AnnUpdateHotPath
    s = _case(O, "last_repeat")
    K, dim, c = s["K"], s["dim"], s["c"]
    made = []
    try:
        ix0 = AnnIndex(len(s["ids"]), dim, K, s["f"]["db"], s["ids"], s["f"]["cent"], P=P, L=13)
        made.append(ix0)
        before = [b.download((b.nbytes,), dtype=np.uint8) for b in (ix0.d_grouped, ix0.d_slots, ix0.d_offsets, ix0.d_forest, ix0.d_roots)]
        hp1 = AnnDeleteHotPath(ix0, c, s["slots"], k=13, tau=TAU).setup()
        made.append(hp1)
        assert hp1.shrink == 2 and hp1.origin == AD.simulate(s["n_c"], s["slots"])[0]
        hp1._witness()
        api.sync()
        ix1 = ix0.removed(hp1)
        made.append(ix1)
        db1, ids1 = AD.compacted_database(s["db"], s["ids"], c, s["slots"])
        # delete then append: two writes into the cluster that shrank to two members (a replacement, and an append that doubles its tree
        # again) ...
        new2 = _rows(61, 2, dim)
        hp2 = AnnUpdateHotPath(ix1, c, ([0, 2], new2), grow=None, k=13, tau=TAU).setup()
        made.append(hp2)
        assert hp2.grow == 1 and hp2.appends == 1
        hp2._witness()
        api.sync()
        assert np.array_equal(hp2.results()[0], hp1.results()[6]), "the update starts from the delete's public index_root_new"
        ix2 = ix1.updated(hp2)
        made.append(ix2)
        db2, ids2 = AU.updated_database(db1, ids1, c, [0, 2], O.quantize(new2, P))
        # ... ) and delete then delete into another cluster
        hp3 = AnnDeleteHotPath(ix1, 2, [0, 0], k=13, tau=TAU).setup()
        made.append(hp3)
        assert hp3.shrink == 2
        hp3._witness()
        api.sync()
        assert np.array_equal(hp3.results()[0], hp1.results()[6])
        ix3 = ix1.removed(hp3)
        made.append(ix3)
        db3, ids3 = AD.compacted_database(db1, ids1, 2, [0, 0])
        for ix, db, ids, root in ((ix1, db1, ids1, hp1.results()[6]), (ix2, db2, ids2, hp2.results()[5]), (ix3, db3, ids3, hp3.results()[6])):
            _same_index(_resident(ix, K, dim), api.ann_index_build(db, ids, s["cent"]))
            assert np.array_equal(ix.qvec, db) and np.array_equal(ix.cluster_ids, ids) and ix.n == db.shape[0]
            assert np.array_equal(ix.roots()[-1], root)
        after = [b.download((b.nbytes,), dtype=np.uint8) for b in (ix0.d_grouped, ix0.d_slots, ix0.d_offsets, ix0.d_forest, ix0.d_roots)]
        assert all(np.array_equal(x, y) for x, y in zip(before, after)), "the old index's buffers are only read"
    finally:
        for x in reversed(made):
            x.free()


def test_remove_refuses_emptying_a_cluster_and_a_slot_above_the_fill(api, O):
    s = _case(O, "shrink")
    old = api.ann_index_build(s["db"], s["ids"], s["cent"])
    api.sync()
    api.profile_begin(deferred=True)
    for c, slots in ((0, [5]), (0, [0, 4]), (1, [0, 0]), (3, [0]), (0, [])):
        with pytest.raises(api.VdbError) as e:
            api.ann_index_remove(old, c, MU.flat_levels(s["tree"]), slots)
        assert e.value.code == -3
    api.sync()
    assert api.profile_end() == {}


# ---------------------------------------------------------------------------------------------------------------- the proof
PROVED = "last_repeat"


@pytest.fixture(scope="module")
def proved(api, O):
    """one AnnDeleteHotPath with its keys and its proof, shared by the tests below"""
    from halo2_vectordb_amd.pipeline import AnnDeleteHotPath, AnnIndex
    from halo2_vectordb_amd.rounds import ProverRounds
    s = _case(O, PROVED)
    index = AnnIndex(len(s["ids"]), s["dim"], s["K"], s["f"]["db"], s["ids"], s["f"]["cent"], P=P, L=13)
    hp = AnnDeleteHotPath(index, s["c"], s["slots"], k=13, tau=TAU).setup()
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
    m = s["m"]
    assert hp.n_cells == m["advice"].shape[0] and hp.n_in == s["K"] + 2 and hp.n_lookup == 0 and np.array_equal(hp.bp, m["break_points"])
    assert hp.shrink == m["s"] and hp.shrink_base == m["regions"]["shrink"] and hp.n_input_rows() == 0
    assert pr.keygen_report.violations() == 0, pr.keygen_report.as_dict()
    assert pr.mock_check().violations() == 0
    assert np.array_equal(proved["stream"], m["advice"])
    root_old, c, slots, removed, last, moved, root_new = hp.results()
    assert np.array_equal(np.concatenate([root_old[None], c[None], np.stack([slots, removed, last, moved], axis=1).reshape(-1, 4), root_new[None]]), m["public"])
    assert np.array_equal(root_old, proved["index"].roots()[-1])
    assert TM.to_ints(last) == [s["n_c"] - 1 - j for j in range(len(s["slots"]))] and TM.to_ints(slots) == s["slots"]
    assert np.array_equal(hp.d_levels.download((2 * hp.lp, 4)), MU.flat_levels(s["tree"]))
    want = TM.to_ints(m["public"])
    assert out["instances"] == want and len(want) == 4 * len(s["slots"]) + 3
    vk = verifier.VerifyingKey.from_prover(pr, out["opened"])
    assert verifier.verify(out["proof"], want, vk)
    for at in (0, 1, 2, 3, 4, 5, len(want) - 1):              # index_root_old, c, a slot, a removed leaf, a last, a moved leaf, index_root_new
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
    lay = CS.ann_delete_layout(s["K"], hp.m, hp.dim, hp.depth, hp.shrink)
    c, u = s["c"], lay["update_layout"]
    one = O.fr_from_ints([1])
    d_flags = api.DeviceBuffer(hp.n_cells)
    try:
        d_flags.upload(np.asarray(pr.circuit.gate).astype(np.uint8))
        assert pr.mock_check(d_flags).violations() == 0              # the witness as it lies in HBM, not emitted again
        carried = [lay["update"] + u["block"][2 * j] for j in range(hp.m)]
        z1 = lay["shrink"] + 2 + 18 + 2238 + 12 + 2238 - 1            # somewhere in the last rows of the first Z hash
        # every carried leaf (the self-carry of delete 0 among them), S_0, Z_0, a cell of a Z hash, the written cluster's out_j and another's
        for cell in carried + [lay["shrink"], lay["shrink"] + 1, z1, lay["new_roots"] + 8 * c + 7, lay["new_roots"] + 8 * (s["K"] - 1) + 7]:
            hp.d_stream.upload(O.fr_add(stream[cell:cell + 1], one), offset=cell * 32)
            rep = pr.mock_check(d_flags)
            hp.d_stream.upload(np.ascontiguousarray(stream[cell:cell + 1]), offset=cell * 32)
            assert rep.violations() >= 1, (cell, rep.as_dict())
        assert pr.mock_check(d_flags).violations() == 0
    finally:
        d_flags.free()


def test_tree_of_another_cluster_breaks_the_picked_tie(api, O):
    """cluster 0's tree (two leaves) passed as the levels of a delete from cluster 1 of the same shape: ids 0 0 1 1 2"""
    from halo2_vectordb_amd import circuit_sym as CS
    from halo2_vectordb_amd.pipeline import AnnDeleteHotPath, AnnIndex
    from halo2_vectordb_amd.rounds import ProverRounds
    ids = np.asarray([0, 0, 1, 1, 2])
    f = dict(db=_rows(96, 5, DIM), cent=_rows(97, 3, DIM))
    index = AnnIndex(5, DIM, 3, f["db"], ids, f["cent"], P=P, L=13)
    try:
        for levels, broken in ((None, False), (index.levels(0), True)):
            hp = AnnDeleteHotPath(index, 1, [0], k=13, tau=TAU, levels=levels).setup()
            pr = ProverRounds(hp).keygen()
            try:
                rep = pr.keygen_report
                assert (rep.violations() >= 1) == broken, rep.as_dict()
                if broken:
                    lay = CS.ann_delete_layout(3, 1, DIM, 1, 1)
                    picked = lay["sponge_old"] - 1
                    assert rep.copies_unequal >= 1 and int(pr.circuit.copy_of[rep.first_copy]) == picked, rep.as_dict()
            finally:
                pr.free()
                hp.free()
    finally:
        index.free()


def test_dropped_half_that_is_not_empty_breaks_the_shrink_tie(api, O):
    """5 -> 4 members halves the tree of 8 leaves; with leaf 6 of the dropped half nonzero (its ancestors rehashed) S_1 = H(S_0, Z_2) is
    not the root the update block ends in: emptiness of the removed half is proved, not assumed"""
    from halo2_vectordb_amd import circuit_sym as CS
    from halo2_vectordb_amd.pipeline import AnnDeleteHotPath, AnnIndex
    from halo2_vectordb_amd.rounds import ProverRounds
    s = _case(O, "shrink")
    index = AnnIndex(len(s["ids"]), DIM, s["K"], s["f"]["db"], s["ids"], s["f"]["cent"], P=P, L=13)
    try:
        lv = [[x.copy() for x in row] for row in MU.build_tree(O, AN.select_cluster(s["db"], s["ids"], s["c"])[0])]
        lv[0][6] = lv[0][0].copy()
        for l in range(3):
            i = 6 >> (l + 1)
            lv[l + 1][i] = O.poseidon_hash_many(np.stack([lv[l][2 * i], lv[l][2 * i + 1]])[None])[0]
        hp = AnnDeleteHotPath(index, s["c"], s["slots"], k=13, tau=TAU, levels=MU.flat_levels(lv)).setup()
        pr = ProverRounds(hp).keygen()
        try:
            rep = pr.keygen_report
            assert rep.copies_unequal >= 2, rep.as_dict()            # the picked tie (the root is not the cluster's) and the S_s tie
            lay = CS.ann_delete_layout(s["K"], 1, DIM, 3, 1)
            cop = np.array(pr.circuit.copy_of)[lay["shrink"]:lay["new_roots"]]
            tied = np.flatnonzero(cop < lay["shrink"])
            assert tied.size == 1, "S_s is the one cell of block S that copies a cell in front of it"
            top, root = lay["shrink"] + int(tied[0]), int(cop[tied[0]])
            assert lay["update"] <= root < lay["shrink"]
            hp._witness()
            api.sync()
            stream = hp.d_stream.download((hp.n_cells, 4))
            assert not np.array_equal(stream[top], stream[root]), "S_s differs from the update block's final root"
            assert np.array_equal(stream[lay["shrink"]], hp.d_levels.download((16, 4))[12]), "S_0 is the halved tree's root"
        finally:
            pr.free()
            hp.free()
    finally:
        index.free()


def test_query_and_read_run_on_the_removed_index(api, O, proved):
    """the chain: the public index_root_new is the root against which a query proves on the removed index; a read opens the moved member
    against its cluster's new root"""
    from halo2_vectordb_amd import verifier
    from halo2_vectordb_amd.pipeline import AnnQueryHotPath, ReadHotPath
    from halo2_vectordb_amd.rounds import ProverRounds
    s, hp, out = proved["s"], proved["hp"], proved["out"]
    c, dim = s["c"], s["dim"]
    made = []
    try:
        ix2 = proved["index"].removed(hp)
        made.append(ix2)
        root_new = out["instances"][-1]
        assert TM.to_ints(ix2.roots()[-1:])[0] == root_new
        members = api.dequantize(ix2.members(c), P)
        # position 0 holds original member 2 after [4, 0, 0], position 1 original member 1
        assert np.array_equal(ix2.members(c), AN.select_cluster(s["db"], s["ids"], c)[0][[2, 1]])
        q = AnnQueryHotPath(ix2, s["f"]["cent"][c] + 0.25, k=13, P=P, L=L, tau=TAU).setup()  # a query next to centroid c probes cluster c
        made.append(q)
        assert q.cluster == c
        pr = ProverRounds(q).keygen()
        made.append(pr)
        assert pr.keygen_report.violations() == 0, pr.keygen_report.as_dict()
        o2 = pr.prove(None, seed=24)
        assert o2["instances"][-1] == root_new and o2["instances"][:dim] in [TM.to_ints(x) for x in ix2.members(c)]
        assert verifier.verify(o2["proof"], o2["instances"], verifier.VerifyingKey.from_prover(pr, o2["opened"]))
        n_c2 = int(ix2.sizes[c])
        rd = ReadHotPath(n=n_c2, dim=dim, m=1, k=13, P=P, tau=TAU, vectors=members, levels=ix2.levels(c), reads=[0]).setup()
        made.append(rd)
        rd._witness()
        api.sync()
        assert np.array_equal(rd.results()[0], ix2.roots()[1 + c]) and np.array_equal(np.asarray(rd.results()[3]).reshape(-1, 4), ix2.members(c)[0])
    finally:
        for x in reversed(made):
            x.free()


def test_single_cell_alteration_sweep(api, O):
    """tests/alteration_model.py's method on the device map and the kernels' bytes at one shape with a real move and a shrink: the one
    kind of cell that stays free is the inverse witness of the is_zero whose operand is zero (tests/test_ann_delete_cpu.py pins it to
    indicator c's)"""
    from halo2_vectordb_amd.pipeline import AnnDeleteHotPath, AnnIndex
    from test_gpu_alteration import device_sweep
    s = _case(O, "shrink")
    index = AnnIndex(len(s["ids"]), s["dim"], s["K"], s["f"]["db"], s["ids"], s["f"]["cent"], P=P, L=13)
    try:
        hp = AnnDeleteHotPath(index, s["c"], s["slots"], k=13, tau=TAU).setup()
        device_sweep(api, O, "ann delete K 3 c 0 m 1 s 1", hp)          # frees the hot path
    finally:
        index.free()
