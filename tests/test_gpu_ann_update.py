"""Inserts and replacements proved against the committed index root on the GPU (pipeline.AnnUpdateHotPath, AnnIndex.updated;
vdb_wit_ann_update*, vdb_ann_index_apply_dev).  The streams are tests/ann_update_model.py's bit for bit (tests/test_ann_update_cpu.py holds
that model against the index model first); host and device forms, rank windows cut inside every new block, the launch list, refused
arguments, the index after the batch against a fresh build, the Mock stage, the whole proof, changed instances, cells tampered in HBM,
the binding of the cluster's tree to its root, and a query against the updated index."""
import ctypes

import numpy as np
import pytest

import ann_model as AN
import ann_update_model as AU
import merkle_ops_model as MO
import merkle_update_model as MU
import topk_model as TM
from test_gpu_batch_query import _dev
from test_gpu_rounds import TAU
from test_gpu_sweep import _check_window, _windowed

pytestmark = pytest.mark.gpu
P, L = 48, 12
IDS3 = [0, 0, 1, 2, 2, 2]                                    # clusters of 2 / 1 / 3 members
# name: (ids, dim, c, slots written, grow): replace slot 0, append, append again (or a write to the appended slot where nothing grows)
CASES = {
    "K3_c0_grow1": (IDS3, 3, 0, [0, 2, 3], 1),
    "K3_c2_grow1": (IDS3, 4, 2, [0, 3, 4], 1),
    "K3_c2_grow0": (IDS3, 3, 2, [0, 3, 3], 0),
    "K3_c1_one_member": (IDS3, 4, 1, [1, 0], 1),
    "K1_grow0": ([0] * 5, 4, 0, [0, 5, 6], 0),
    "K1_grow1": ([0] * 7, 3, 0, [0, 7, 8], 1),
}


@pytest.fixture(scope="module")
def api():
    from halo2_vectordb_amd import api as a
    a.init(0)
    return a


def _rows(seed, n, dim):
    return np.random.default_rng(seed).integers(0, 219, size=(n, dim)).astype(np.float64)


_MODELS = {}


def _case(O, name, seed=80):
    """-> dict(f64 rows, quantized rows, the index model before the batch, the cluster's grown tree before the batch (device layout), the
    model and its tree after the batch); computed once per case and left unchanged"""
    if name not in _MODELS:
        ids, dim, c, slots, grow = CASES[name]
        ids = np.asarray(ids)
        K = int(ids.max()) + 1
        f = dict(db=_rows(seed, len(ids), dim), cent=_rows(seed + 1, K, dim))
        # the written vectors lie next to centroid c and apart from each other: index.probe finds c for them (the circuit does not prove it)
        f["new"] = f["cent"][c][None, :] + np.outer(np.arange(1, len(slots) + 1), np.eye(dim)[0] + 2 * np.eye(dim)[1])
        db, cent, new = (O.quantize(f[k], P) for k in ("db", "cent", "new"))
        ix = AN.index_model(O, db, ids, cent)
        tree = MO.grow_tree(O, MU.build_tree(O, AN.select_cluster(db, ids, c)[0]), grow)
        grown = MU.flat_levels(tree)
        m = AU.update_model(O, ix["roots"][:K + 1], c, tree, slots, new, grow, plan_k=13)
        _MODELS[name] = dict(f=f, db=db, cent=cent, new=new, ids=ids, K=K, dim=dim, c=c, slots=slots, grow=grow, ix=ix, grown=grown, m=m, tree=tree,
                             n_c=int((ids == c).sum()))
    return _MODELS[name]


def _update_dev(api, s, levels=None, profile=False, K=None, roots=None, slots=None, new=None):
    """vdb_wit_ann_update_dev into poisoned buffers -> (stream, flags, public, levels after[, launches per kernel of a second run])"""
    from halo2_vectordb_amd._lib import check
    lib = api.init()
    slots, new = s["slots"] if slots is None else slots, s["new"] if new is None else new
    m, K = len(slots), s["K"] if K is None else K
    roots = s["ix"]["roots"][:K + 1] if roots is None else roots
    cells, n_in, ub = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
    check(lib.vdb_wit_ann_update_size(K, s["n_c"], s["dim"], m, s["grow"], ctypes.byref(cells), ctypes.byref(n_in), ctypes.byref(ub)))
    cells, idx = cells.value, np.ascontiguousarray(slots, dtype=np.uint64)
    levels = s["grown"] if levels is None else levels
    up = []
    try:
        d_lv, d_roots, d_new = _dev(api, up, levels), _dev(api, up, roots), _dev(api, up, new)
        d_adv, d_sel, d_pub = api.DeviceBuffer(cells * 32), api.DeviceBuffer(cells), api.DeviceBuffer((3 * m + 3) * 32)
        up += [d_adv, d_sel, d_pub]
        check(lib.vdb_memset_dev(d_adv.ptr, 0xA5, ctypes.c_size_t(cells * 32)))
        check(lib.vdb_memset_dev(d_sel.ptr, 0xFF, ctypes.c_size_t(cells)))
        run = lambda: check(lib.vdb_wit_ann_update_dev(d_lv.ptr, d_roots.ptr, K, s["c"], s["n_c"], s["dim"], s["grow"], d_new.ptr, api._p(idx), m, d_adv.ptr,
                                                       d_sel.ptr, d_pub.ptr))
        run()
        api.sync()
        out = [d_adv.download((cells, 4)), d_sel.download((cells,), dtype=np.uint8), d_pub.download((3 * m + 3, 4)), d_lv.download(levels.shape)]
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
@pytest.mark.parametrize("name", sorted(CASES))
def test_entry_points_write_the_models_stream_and_leave_the_models_tree(api, O, name):
    s = _case(O, name)
    m, K, c = s["m"], s["K"], s["c"]
    stream, flags, pub, levels1 = _update_dev(api, s)
    assert stream.shape == m["advice"].shape
    bad = np.flatnonzero((stream != m["advice"]).any(axis=1))
    assert bad.size == 0, f"first differing advice cells {bad[:5]} of {stream.shape[0]} (blocks {m['regions']})"
    assert np.array_equal(flags & 1, m["selectors"]) and not (flags & ~np.uint8(3)).any()
    # the flag bytes: the update block's are those of the block emitted alone; the new blocks' are the model's (the selection's leading
    # zero is not flagged by the generator, as in the query circuit); no lookup cell
    r = m["regions"]
    alone = api.wit_merkle_update(s["grown"], s["n_c"], s["new"], s["slots"], selectors=True, grow=s["grow"])
    assert np.array_equal(flags[r["update"]:r["new_roots"]], alone["flags"]) and np.array_equal(stream[r["update"]:r["new_roots"]], alone["stream"])
    outside = np.ones(flags.shape[0], dtype=bool)
    outside[r["update"]:r["new_roots"]] = False
    assert np.array_equal(flags[outside], m["flags"][outside]) and not flags[:K + 2].any()
    assert np.array_equal(pub, m["public"]) and pub.shape[0] == 3 * len(s["slots"]) + 3
    assert np.array_equal(levels1, MU.flat_levels(s["tree"])) and np.array_equal(levels1, alone["levels"])
    host = api.wit_ann_update(s["grown"], s["ix"]["roots"][:K + 1], c, s["n_c"], s["new"], s["slots"], grow=s["grow"], selectors=True)
    assert np.array_equal(host["stream"], stream) and np.array_equal(host["flags"], flags) and np.array_equal(host["public"], pub)
    assert np.array_equal(host["levels"], levels1) and host["input_cells"] == K + 2 and host["update_base"] == r["update"]


def test_indicators_far_from_c_take_their_inverse_from_the_inverse_list(api, O):
    """K = 300: |c - j| reaches 299, beyond the small-inverse table (260 entries); block B is the integer template's cell for cell"""
    s = dict(_case(O, "K3_c2_grow0"))
    K, c = 300, 299
    roots = O.quantize(_rows(90, K + 1, 1), P)[:, 0].copy()
    roots[1 + c] = s["ix"]["roots"][1 + s["c"]]
    s.update(c=c)
    stream, flags, pub, _ = _update_dev(api, s, K=K, roots=roots)
    cells, gates = [], []
    for j in range(K):
        x, g, _ = TM.is_equal(c, j)
        cells += x[4:] if j == 0 else x
        gates += g[4:] if j == 0 else g
    lo = K + 2
    assert np.array_equal(stream[lo:lo + len(cells)], TM.to_limbs(cells)) and np.array_equal(flags[lo:lo + len(cells)] & 1, np.asarray(gates, dtype=np.uint8))
    assert len(cells) == 8 + 12 * (K - 1) and np.array_equal(pub[0], O.poseidon_merkle_root(roots[None])) and TM.to_ints(pub[1:2]) == [c]


def test_two_windowed_calls_write_the_bytes_of_one(api, O):
    from halo2_vectordb_amd._lib import check
    lib = api.init()
    s = _case(O, "K3_c2_grow1")
    m, K = s["m"], s["K"]
    want, pub, r = m["advice"], m["public"], m["regions"]
    cells = want.shape[0]
    lk = np.zeros((0, 4), dtype=np.uint64)
    idx = np.ascontiguousarray(s["slots"], dtype=np.uint64)
    up = []
    try:
        d_new, d_roots, d_pub = _dev(api, up, s["new"]), _dev(api, up, s["ix"]["roots"][:K + 1]), _dev(api, up, np.zeros_like(pub))
        u = m["update"]
        # inside the header, inside an indicator block, between C and D, inside F, inside the update block (its inputs, a level), near the end
        for cut in (2, r["indicator"] + 8 + 5, r["sponge_old"], r["new_roots"] + 11, r["update"] + u["n_in"] - 2,
                    r["update"] + u["regions"][1]["levels"][0] + 25, cells - 3):
            halves = []
            for window in ((0, cut, 0, 0), (cut, cells, 0, 0)):
                d_lv = _dev(api, up, s["grown"])                    # every call starts from the tree before the batch
                run = lambda d_adv, d_lk: check(lib.vdb_wit_ann_update_dev(d_lv.ptr, d_roots.ptr, K, s["c"], s["n_c"], s["dim"], s["grow"], d_new.ptr,
                                                                           api._p(idx), len(idx), d_adv.ptr, None, d_pub.ptr))
                g_adv, _ = _windowed(api, lib, check, want, lk, window, run)
                _check_window(want, lk, g_adv, lk, window, (cut, window))
                assert np.array_equal(d_pub.download(pub.shape), pub), (cut, window)
                assert np.array_equal(d_lv.download(s["grown"].shape), MU.flat_levels(s["tree"])), (cut, window)
                halves.append(g_adv)
            assert np.array_equal(np.concatenate([halves[0][:cut], halves[1][cut:]]), want), cut
    finally:
        for b in up:
            b.free()


def test_launch_list_depends_on_neither_K_nor_m_and_refused_arguments_launch_nothing(api, O):
    from halo2_vectordb_amd._lib import check
    lib = api.init()
    a, b = _case(O, "K3_c2_grow0"), _case(O, "K1_grow0")          # depth 2 against depth 3: only the level launches may differ
    counts = {}
    counts["K3_m3"] = _update_dev(api, a, profile=True)[4]
    counts["K3_m1"] = _update_dev(api, a, profile=True, slots=[3], new=a["new"][:1])[4]
    counts["K1_m3"] = _update_dev(api, b, profile=True)[4]
    counts["K1_m1"] = _update_dev(api, b, profile=True, slots=[2], new=b["new"][:1])[4]
    assert counts["K3_m3"] == counts["K3_m1"] and counts["K1_m3"] == counts["K1_m1"], counts
    want = dict(k_annu_header=1, k_annu_indicator=1, k_nv_select=1, k_mk_leaf_states=3, k_mk_leaf_trace=3, k_mku_touchers=1, k_mku_level=2,
                k_mku_writeback=1, k_mku_inputs=1, k_mku_level_trace=1, k_mku_index=1, k_annu_new_roots=1, k_annu_public=1, k_inv_fixup=1)
    assert counts["K3_m3"] == want and counts["K1_m3"] == dict(want, k_mku_level=3), counts
    grown = _update_dev(api, _case(O, "K3_c2_grow1"), profile=True)[4]
    assert grown == dict(want, k_mku_level=3, k_mku_grow_trace=1), grown
    # refusals: c >= K, K = 0, K too large, an index above the fill at its turn, an index >= lp 2^g, no write, depth 0, d + g > 30
    s = a
    up = []
    try:
        d_lv, d_roots, d_new = _dev(api, up, s["grown"]), _dev(api, up, s["ix"]["roots"][:4]), _dev(api, up, s["new"])
        d_out = api.DeviceBuffer(1 << 16)
        up.append(d_out)
        check(lib.vdb_memset_dev(d_out.ptr, 0xA5, ctypes.c_size_t(1 << 16)))
        api.sync()
        api.profile_begin(deferred=True)
        for K, c, n_c, grow, idx in ((3, 3, 3, 0, [0]), (0, 0, 3, 0, [0]), (4097, 0, 3, 0, [0]), (3, 2, 3, 0, [0, 4]), (3, 2, 5, 0, [6]), (3, 2, 3, 0, []),
                                     (3, 1, 1, 0, [0]), (3, 2, 3, 29, [0]), (3, 2, 2, 0, [0, 3])):
            uidx = np.ascontiguousarray(idx + [0], dtype=np.uint64)
            with pytest.raises(api.VdbError) as e:
                check(lib.vdb_wit_ann_update_dev(d_lv.ptr, d_roots.ptr, K, c, n_c, s["dim"], grow, d_new.ptr, api._p(uidx), len(idx), d_out.ptr, None,
                                                 d_out.at(1 << 15)))
            assert e.value.code == -3, (K, c, n_c, grow, idx)
        api.sync()
        assert api.profile_end() == {}
        assert (d_out.download((1 << 16,), dtype=np.uint8) == 0xA5).all() and np.array_equal(d_lv.download(s["grown"].shape), s["grown"])
    finally:
        for b in up:
            b.free()


# ---------------------------------------------------------------------------------------------------------------- the index after the batch
def _same_index(got, want, K):
    for key in ("grouped", "slots", "offsets", "roots"):
        assert np.array_equal(got[key], want[key]), key
    assert np.array_equal(got["segments"], want["segments"]) and np.array_equal(got["forest"], want["forest"])


@pytest.mark.parametrize("name", sorted(CASES))
def test_applied_index_is_a_fresh_build_over_the_updated_database(api, O, name):
    s = _case(O, name)
    K, c = s["K"], s["c"]
    old = api.ann_index_build(s["db"], s["ids"], s["cent"])
    app = AU.track_fill(s["slots"], s["n_c"])
    n = s["db"].shape[0]
    got = api.ann_index_apply(old, c, s["grow"], MU.flat_levels(s["tree"]), s["new"], s["slots"], np.arange(n, n + app))
    db2, ids2 = AU.updated_database(s["db"], s["ids"], c, s["slots"], s["new"])
    _same_index(got, api.ann_index_build(db2, ids2, s["cent"]), K)
    assert np.array_equal(got["roots"][-1], s["m"]["public"][-1]), "the applied index's root is the circuit's public index_root_new"


def test_two_chained_batches_on_resident_indices_and_the_old_index_stays(api, O):
    from halo2_vectordb_amd.pipeline import AnnIndex, AnnUpdateHotPath
    s = _case(O, "K3_c0_grow1")
    K, dim = s["K"], s["dim"]
    made = []
    try:
        ix0 = AnnIndex(6, dim, K, s["f"]["db"], s["ids"], s["f"]["cent"], P=P, L=13)
        made.append(ix0)
        before = [b.download((b.nbytes,), dtype=np.uint8) for b in (ix0.d_grouped, ix0.d_slots, ix0.d_offsets, ix0.d_forest, ix0.d_roots)]
        hp1 = AnnUpdateHotPath(ix0, s["c"], (s["slots"], s["f"]["new"]), grow=None, k=13, tau=TAU).setup()
        made.append(hp1)
        assert hp1.grow == 1 and hp1.appends == 2
        hp1._witness()
        api.sync()
        ix1 = ix0.updated(hp1)
        made.append(ix1)
        db1, ids1 = AU.updated_database(s["db"], s["ids"], s["c"], s["slots"], s["new"])
        # the second batch goes to another cluster of the updated index: a replacement and an append into its padding
        new2 = _rows(95, 2, dim)
        hp2 = AnnUpdateHotPath(ix1, 2, ([1, 3], new2), grow=None, k=13, tau=TAU).setup()
        made.append(hp2)
        assert hp2.grow == 0 and hp2.appends == 1
        hp2._witness()
        api.sync()
        assert np.array_equal(hp2.results()[0], hp1.results()[5]), "the second proof starts from the first's public index_root_new"
        ix2 = ix1.updated(hp2)
        made.append(ix2)
        db2, ids2 = AU.updated_database(db1, ids1, 2, [1, 3], O.quantize(new2, P))
        for ix, db, ids in ((ix1, db1, ids1), (ix2, db2, ids2)):
            want = api.ann_index_build(db, ids, s["cent"])
            n = db.shape[0]
            got = dict(grouped=ix.d_grouped.download((n, dim, 4)), slots=ix.d_slots.download((n,), dtype=np.uint32),
                       offsets=ix.d_offsets.download((K + 1,), dtype=np.uint64), forest=ix.d_forest.download((ix.n_digests, 4)), segments=ix.segments,
                       roots=ix.roots())
            _same_index(got, want, K)
            assert np.array_equal(ix.qvec, db) and np.array_equal(ix.cluster_ids, ids) and ix.n == n
        assert np.array_equal(ix2.roots()[-1], hp2.results()[5])
        after = [b.download((b.nbytes,), dtype=np.uint8) for b in (ix0.d_grouped, ix0.d_slots, ix0.d_offsets, ix0.d_forest, ix0.d_roots)]
        assert all(np.array_equal(x, y) for x, y in zip(before, after)), "the old index's buffers are only read"
    finally:
        for x in reversed(made):
            x.free()


def test_apply_refuses_a_hole_and_a_growth_that_is_not_the_smallest(api, O):
    s = _case(O, "K3_c0_grow1")
    old = api.ann_index_build(s["db"], s["ids"], s["cent"])
    api.sync()
    api.profile_begin(deferred=True)
    for grow, slots in ((1, [3]), (0, [0, 2, 3]), (2, [0, 2, 3])):
        with pytest.raises(api.VdbError) as e:
            api.ann_index_apply(old, s["c"], grow, MU.flat_levels(s["tree"]), s["new"][:len(slots)], slots, np.arange(6, 8))
        assert e.value.code == -3
    api.sync()
    assert api.profile_end() == {}


# ---------------------------------------------------------------------------------------------------------------- the proof
PROVED = "K3_c2_grow1"


@pytest.fixture(scope="module")
def proved(api, O):
    """one AnnUpdateHotPath with its keys and its proof, shared by the tests below"""
    from halo2_vectordb_amd.pipeline import AnnIndex, AnnUpdateHotPath
    from halo2_vectordb_amd.rounds import ProverRounds
    s = _case(O, PROVED)
    index = AnnIndex(len(s["ids"]), s["dim"], s["K"], s["f"]["db"], s["ids"], s["f"]["cent"], P=P, L=13)
    hp = AnnUpdateHotPath(index, s["c"], (s["slots"], s["f"]["new"]), grow=s["grow"], k=13, tau=TAU).setup()
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
    assert pr.keygen_report.violations() == 0, pr.keygen_report.as_dict()
    assert pr.mock_check().violations() == 0
    assert np.array_equal(proved["stream"], m["advice"])
    root_old, c, idx, old_leaves, new_leaves, root_new = hp.results()
    assert np.array_equal(np.concatenate([root_old[None], c[None], np.stack([idx, old_leaves, new_leaves], axis=1).reshape(-1, 4), root_new[None]]), m["public"])
    assert np.array_equal(root_old, proved["index"].roots()[-1])
    assert np.array_equal(hp.d_levels.download((2 * hp.lp, 4)), MU.flat_levels(s["tree"]))
    want = TM.to_ints(m["public"])
    assert out["instances"] == want and len(want) == 3 * len(s["slots"]) + 3
    vk = verifier.VerifyingKey.from_prover(pr, out["opened"])
    assert verifier.verify(out["proof"], want, vk)
    for at in (0, 1, 4, len(want) - 1):                       # index_root_old, c, a new leaf, index_root_new
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
    lay = CS.ann_update_layout(s["K"], hp.m, hp.dim, hp.depth, hp.grow)
    c, K = s["c"], s["K"]
    one = O.fr_from_ints([1])
    d_flags = api.DeviceBuffer(hp.n_cells)
    try:
        d_flags.upload(np.asarray(pr.circuit.gate).astype(np.uint8))
        assert pr.mock_check(d_flags).violations() == 0              # the witness as it lies in HBM, not emitted again
        ind_c = lay["indicator"] + 8 + 12 * (c - 1) + 4 + 6           # is_equal(c, Constant(c))'s output
        # a cluster root (the written cluster's and another's), centroids_root, an indicator, an out_j (the written cluster's and another's)
        for cell in (lay["roots"] + c, lay["roots"], lay["centroids_root"], ind_c, lay["indicator"] + 6, lay["new_roots"] + 8 * c + 7, lay["new_roots"] + 7):
            hp.d_stream.upload(O.fr_add(stream[cell:cell + 1], one), offset=cell * 32)
            rep = pr.mock_check(d_flags)
            hp.d_stream.upload(np.ascontiguousarray(stream[cell:cell + 1]), offset=cell * 32)
            assert rep.violations() >= 1, (cell, rep.as_dict())
        assert pr.mock_check(d_flags).violations() == 0
    finally:
        d_flags.free()


def test_tree_of_another_cluster_breaks_the_picked_tie(api, O):
    """cluster 0's tree (two leaves) passed as the levels of an update of cluster 1 ... of the same shape: ids 0 0 1 1 2"""
    from halo2_vectordb_amd import circuit_sym as CS
    from halo2_vectordb_amd.pipeline import AnnIndex, AnnUpdateHotPath
    from halo2_vectordb_amd.rounds import ProverRounds
    ids, dim = np.asarray([0, 0, 1, 1, 2]), 3
    f = dict(db=_rows(96, 5, dim), cent=_rows(97, 3, dim), new=_rows(98, 1, dim))
    index = AnnIndex(5, dim, 3, f["db"], ids, f["cent"], P=P, L=13)
    try:
        for levels, broken in ((None, False), (index.levels(0), True)):
            hp = AnnUpdateHotPath(index, 1, ([1], f["new"]), grow=0, k=13, tau=TAU, levels=levels).setup()
            pr = ProverRounds(hp).keygen()
            try:
                rep = pr.keygen_report
                assert (rep.violations() >= 1) == broken, rep.as_dict()
                if broken:
                    lay = CS.ann_update_layout(3, 1, dim, 1, 0)
                    picked = lay["sponge_old"] - 1
                    assert rep.copies_unequal >= 1 and int(pr.circuit.copy_of[rep.first_copy]) == picked, rep.as_dict()
            finally:
                pr.free()
                hp.free()
    finally:
        index.free()


def test_query_and_read_run_on_the_updated_index(api, O, proved):
    """the chain: the public index_root_new is the root against which a query near the inserted vector proves, and that query returns the
    inserted vector; a read opens it against its cluster's new root"""
    from halo2_vectordb_amd import verifier
    from halo2_vectordb_amd.pipeline import AnnQueryHotPath, ReadHotPath
    from halo2_vectordb_amd.rounds import ProverRounds
    s, hp, out = proved["s"], proved["hp"], proved["out"]
    c, dim = s["c"], s["dim"]
    made = []
    try:
        ix2 = proved["index"].updated(hp)
        made.append(ix2)
        root_new = out["instances"][-1]
        assert TM.to_ints(ix2.roots()[-1:])[0] == root_new
        inserted = s["f"]["new"][-1]                              # the last append: slot n_c + 1 of the cluster
        assert ix2.probe(inserted + 0.25) == c
        q = AnnQueryHotPath(ix2, inserted + 0.25, k=13, P=P, L=L, tau=TAU).setup()
        made.append(q)
        assert q.cluster == c
        pr = ProverRounds(q).keygen()
        made.append(pr)
        assert pr.keygen_report.violations() == 0, pr.keygen_report.as_dict()
        o2 = pr.prove(None, seed=24)
        assert o2["instances"][-1] == root_new and o2["instances"][:dim] == TM.to_ints(O.quantize(inserted[None], P)[0])
        assert verifier.verify(o2["proof"], o2["instances"], verifier.VerifyingKey.from_prover(pr, o2["opened"]))
        n_c2 = int(ix2.sizes[c])
        members = api.dequantize(ix2.members(c), P)
        rd = ReadHotPath(n=n_c2, dim=dim, m=1, k=13, P=P, tau=TAU, vectors=members, levels=ix2.levels(c), reads=[n_c2 - 1]).setup()
        made.append(rd)
        rd._witness()
        api.sync()
        assert np.array_equal(rd.results()[0], ix2.roots()[1 + c]) and np.array_equal(np.asarray(rd.results()[3]).reshape(-1, 4), O.quantize(inserted[None], P)[0])
    finally:
        for x in reversed(made):
            x.free()


def test_single_cell_alteration_sweep(api, O):
    """tests/alteration_model.py's method on the device map and the kernels' bytes at one shape: the one kind of cell that stays free is
    the inverse witness of the is_zero whose operand is zero (tests/test_ann_update_cpu.py pins it to indicator c's)"""
    from halo2_vectordb_amd.pipeline import AnnIndex, AnnUpdateHotPath
    from test_gpu_alteration import device_sweep
    s = _case(O, "K3_c0_grow1")
    index = AnnIndex(len(s["ids"]), s["dim"], s["K"], s["f"]["db"], s["ids"], s["f"]["cent"], P=P, L=13)
    try:
        hp = AnnUpdateHotPath(index, s["c"], (s["slots"][:2], s["f"]["new"][:2]), grow=1, k=13, tau=TAU).setup()
        device_sweep(api, O, "ann update K 3 c 0 m 2 grow 1", hp)      # frees the hot path
    finally:
        index.free()
