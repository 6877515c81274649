"""The recentre of one cluster on the GPU (pipeline.AnnRecentreHotPath, vdb_wit_ann_recentre*; AnnIndex.recentred_with,
vdb_ann_index_recentre_dev): the streams are tests/ann_recentre_model.py's bit for bit (tests/test_ann_recentre_cpu.py holds that model
against the host-built map first); host and device forms, the launch lists, refused arguments, rank windows, the device-placed map, the
proof, the index after it against a build from scratch, the chain over all K clusters against recentred(), an update followed by a
recentre, and the alteration sweep."""
import ctypes

import numpy as np
import pytest

import ann_mean_model as MM
import ann_recentre_model as RM
import merkle_update_model as MU
import topk_model as TM
from test_ann_recentre_cpu import L, P, index_of
from test_gpu_batch_query import _dev
from test_gpu_rounds import TAU
from test_gpu_sweep import _check_window, _windowed

pytestmark = pytest.mark.gpu

# K, n_c, dim, c; the last: K past one 64-lane block of indicators and a path of depth 7
CASES = [(2, 2, 3, 1), (3, 65, 2, 0), (5, 70, 65, 4), (70, 2, 3, 69)]
_cache = {}


@pytest.fixture(scope="module")
def api():
    from halo2_vectordb_amd import api as a
    a.init(0)
    return a


def case(O, K, n_c, dim, c):
    """-> (model, centroids, members, roots (K + 2, 4), the centroids' tree before and after the write as the device lays them out),
    computed once per case and shared; nothing changes it"""
    key = (K, n_c, dim, c)
    if key not in _cache:
        cent, mem, clusters, roots = index_of(O, K, n_c, dim, c)
        tree = MU.build_tree(O, cent)
        before = MU.flat_levels(tree)
        m = RM.recentre_model(O, tree, mem, roots[:K + 1], c, P, L)
        _cache[key] = (m, cent, mem, roots, before, MU.flat_levels(tree))
    return _cache[key]


def _index(O, K, n_c, dim, c):
    """the resident index of a case (test_ann_recentre_cpu.index_of: arbitrary centroids, cluster c the members, every other cluster one
    row, its own centroid)"""
    from halo2_vectordb_amd.pipeline import AnnIndex
    cent, mem, clusters, _ = index_of(O, K, n_c, dim, c)
    ids = np.concatenate([np.full(x.shape[0], j) for j, x in enumerate(clusters)])
    return AnnIndex(ids.shape[0], dim, K, np.concatenate(clusters), ids, cent, P=P, L=L)


def _hot_path(O, K, n_c, dim, c, k=13, **kw):
    from halo2_vectordb_amd.pipeline import AnnRecentreHotPath
    index = _index(O, K, n_c, dim, c)
    return index, AnnRecentreHotPath(index, c, k=k, P=P, L=L, tau=TAU, **kw)


@pytest.mark.parametrize("K,n_c,dim,c", CASES)
def test_witness_is_the_models_resident_absent_and_from_host_arrays(api, O, K, n_c, dim, c):
    from halo2_vectordb_amd import circuit_sym as CS
    from halo2_vectordb_amd._lib import check
    m, cent, mem, roots, before, after = case(O, K, n_c, dim, c)
    host = api.wit_ann_recentre(before, mem, roots[:K + 1], c, P, L, selectors=True)
    assert host["n_in"] == m["n_in"] == K + 2 and host["stream"].shape == m["advice"].shape
    bad = np.flatnonzero((host["stream"] != m["advice"]).any(axis=1))
    assert bad.size == 0, f"first differing advice cells {bad[:5]} of {host['stream'].shape[0]} (blocks {m['regions']})"
    assert np.array_equal(host["lookup"], m["lookup"]) and np.array_equal(host["selectors"], m["selectors"])
    gen = m["generator"].copy()                              # the flag bytes beyond the gate bit: the model's outside the qdiv blocks
    # ... and outside the update block, whose flag bytes and cells are those of the block emitted alone (as in the index update)
    r = m["regions"]
    alone = api.wit_merkle_update(before, K, m["new_centroid"][None], [c], selectors=True)
    assert np.array_equal(host["flags"][r["centroid_update"]:r["sponge_new"]], alone["flags"])
    assert np.array_equal(host["stream"][r["centroid_update"]:r["sponge_new"]], alone["stream"]) and np.array_equal(alone["levels"], after)
    gen[r["centroid_update"]:r["sponge_new"]] = True
    bad = np.flatnonzero((host["flags"] != m["flags"]) & ~gen)
    assert bad.size == 0, f"first differing flag bytes at {bad[:8]}: {host['flags'][bad[:8]]} against {m['flags'][bad[:8]]} (blocks {m['regions']})"
    assert np.array_equal(host["public"], m["public"]) and np.array_equal(host["public"][0], roots[-1])
    assert np.array_equal(host["new_centroid"], m["new_centroid"]) and np.array_equal(host["new_centroid"], MM.means(O, mem, P, L))
    assert np.array_equal(host["levels"], after) and host["update_base"] == m["regions"]["centroid_update"]
    lay = CS.ann_recentre_layout(K, n_c, dim, P, L)          # ann_recentre_layout is annr_blocks through vdb_wit_ann_recentre_size
    cells, lk, n_in, ub = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
    check(api.init().vdb_wit_ann_recentre_size(P, L, K, n_c, dim, ctypes.byref(cells), ctypes.byref(lk), ctypes.byref(n_in), ctypes.byref(ub)))
    assert (cells.value, lk.value, n_in.value, ub.value) == (lay["total"], lay["total_l"], lay["n_in"], lay["centroid_update"])
    index, hp = _hot_path(O, K, n_c, dim, c)
    try:
        assert np.array_equal(index.roots(), roots) and np.array_equal(index.members(c), mem)
        hp.setup()
        assert hp.resident and (hp.n_cells, hp.n_in, hp.n_lookup) == (m["advice"].shape[0], K + 2, m["lookup"].shape[0])
        d_flags = hp.keygen_flags()
        assert np.array_equal(d_flags.download((hp.n_cells,), dtype=np.uint8), host["flags"])
        d_flags.free()
        for resident in (True, False):
            check(hp.lib.vdb_memset_dev(hp.d_stream.ptr, 0xA5, ctypes.c_size_t(hp.n_cells * 32)))
            check(hp.lib.vdb_memset_dev(hp.d_lookup.ptr, 0xA5, ctypes.c_size_t(hp.n_lookup * 32)))
            check(hp.lib.vdb_memset_dev(hp.d_new.ptr, 0xA5, ctypes.c_size_t(dim * 32)))
            check(hp.lib.vdb_memset_dev(hp.d_pub.ptr, 0xA5, ctypes.c_size_t(3 * 32)))
            hp.resident = resident
            hp._witness()
            api.sync()
            assert np.array_equal(hp.d_stream.download((hp.n_cells, 4)), host["stream"]), resident
            assert np.array_equal(hp.d_lookup.download((hp.n_lookup, 4)), host["lookup"]), resident
            root_old, c_fr, root_new, new = hp.results()
            assert np.array_equal(np.stack([root_old, c_fr, root_new]), m["public"]) and np.array_equal(new, m["new_centroid"]), resident
            assert np.array_equal(hp.d_levels.download(after.shape), after) and np.array_equal(hp.d_levels0.download(before.shape), before), resident
    finally:
        hp.free()
        index.free()


def test_launch_lists_differ_in_the_path_levels_alone_and_refused_arguments_launch_nothing(api, O):
    from halo2_vectordb_amd import circuit_sym as CS
    from halo2_vectordb_amd._lib import check
    counts = {}
    for K, n_c, dim, c in ((2, 2, 3, 1), (5, 70, 65, 4)):
        index, hp = _hot_path(O, K, n_c, dim, c)
        try:
            hp.setup()
            hp._witness()
            api.sync()
            api.profile_begin(deferred=True)
            hp._witness()
            api.sync()
            counts[K] = {kern: int(v["launches"]) for kern, v in api.profile_end().items()}
            lib = hp.lib
            d_out = api.DeviceBuffer(1 << 16)
            check(lib.vdb_memset_dev(d_out.ptr, 0xA5, ctypes.c_size_t(1 << 16)))
            check(lib.vdb_memcpy_d2d(hp.d_levels.ptr, hp.d_levels0.ptr, ctypes.c_size_t(2 * hp.lp * 32)))
            api.sync()
            api.profile_begin(deferred=True)

            def call(K_=K, c_=c, n_c_=n_c, dim_=dim, P_=P, L_=L):
                return lib.vdb_wit_ann_recentre_dev(P_, L_, hp.d_levels.ptr, hp.p_members, index.d_roots.ptr, None, K_, c_, n_c_, dim_, d_out.ptr,
                                                    d_out.at(1 << 14), None, d_out.at(1 << 15), d_out.at(3 << 14))
            big = 1 << 24
            # K = 1 (no path), the frame's refusals, the mean audit's own, the instance limit, the cell limit (a circuit whose instance
            # count passes: held against the layout first)
            huge = dict(n_c_=1 << 16, dim_=256, K_=2)
            lay = CS.ann_recentre_layout(huge["K_"], huge["n_c_"], huge["dim_"], P, L)
            assert lay["total"] > 1 << 34 and huge["n_c_"] * huge["dim_"] <= big
            sized = [dict(K_=1), dict(K_=0), dict(K_=4097), dict(n_c_=big + 1), dict(n_c_=0), dict(dim_=0), dict(dim_=(1 << 20) + 1),
                     dict(n_c_=big // dim + 1), huge]
            for kw in sized:                                        # the size call first: it shares the layout and writes nothing
                cells = ctypes.c_uint64()
                assert lib.vdb_wit_ann_recentre_size(P, L, kw.get("K_", K), kw.get("n_c_", n_c), kw.get("dim_", dim), ctypes.byref(cells), None, None,
                                                     None) == -3, kw
            for kw in sized + [dict(c_=K)]:
                with pytest.raises(api.VdbError) as e:
                    check(call(**kw))
                assert e.value.code == -3, kw
            with pytest.raises(api.VdbError) as e:
                check(call(K_=1, c_=0))
            assert "a tree of one leaf has no path" in str(e.value)
            api.sync()
            assert api.profile_end() == {}
            assert (d_out.download((1 << 16,), dtype=np.uint8) == 0xA5).all()
            assert np.array_equal(hp.d_levels.download((2 * hp.lp, 4)), hp.d_levels0.download((2 * hp.lp, 4)))
            d_out.free()
        finally:
            hp.free()
            index.free()
    a, b = dict(counts[2]), dict(counts[5])
    assert (a.pop("k_mku_level"), b.pop("k_mku_level")) == (1, 3), counts          # one launch per level of the centroids' path
    assert a == b, counts
    assert a["k_annm_sum"] == 1 and a["k_annr_div"] == 1 and a["k_inv_fixup"] == 1 and a["k_nv_select"] == 1, counts
    assert a["k_mku_inputs"] == 2 and a["k_mk_tree_trace"] == 1 and a["k_annu_public"] == 1, counts        # I and U's witnesses; MM; the public row
    assert a["k_mk_leaf_trace"] == 4, counts                 # D, MM's leaves, U's new leaf, G
    for absent in ("k_annm_div", "k_annu_new_roots", "k_mk_level_values", "k_mku_grow_trace"):
        assert absent not in a, counts


def test_windowed_calls_write_the_bytes_of_one(api, O):
    from halo2_vectordb_amd._lib import check
    lib = api.init()
    K, n_c, dim, c = 3, 3, 2, 2                              # a padded members' tree (its zero cell) and a path of two levels
    cent, mem, clusters, roots = index_of(O, K, n_c, dim, c)
    tree = MU.build_tree(O, cent)
    before = MU.flat_levels(tree)
    m = RM.recentre_model(O, tree, mem, roots[:K + 1], c, P, L)
    after = MU.flat_levels(tree)
    want, lk, r = m["advice"], m["lookup"], m["regions"]
    cells, q_n, q_lk, n_lk = want.shape[0], m["qdiv_cells"], m["qdiv_lk"], len(m["lookup"])
    u, ub = m["update"], r["centroid_update"]
    up = []
    try:
        d_lv, d_mem, d_roots = _dev(api, up, before), _dev(api, up, mem), _dev(api, up, roots[:K + 1])
        d_new, d_pub = api.DeviceBuffer(max(dim * 32, 32)), api.DeviceBuffer(96)
        up += [d_new, d_pub]

        def run(d_adv, d_lkb):
            d_lv.upload(before)
            check(lib.vdb_wit_ann_recentre_dev(P, L, d_lv.ptr, d_mem.ptr, d_roots.ptr, None, K, c, n_c, dim, d_adv.ptr, d_lkb.ptr, None, d_new.ptr, d_pub.ptr))
        # inside the header; inside I; on len; one cell behind it; inside a qadd of the chain; between the two quotients (the lookup cut
        # between their runs); inside MM; inside U's leaf sponge; at U's second level and inside it; inside G
        lv1 = ub + u["regions"][0]["levels"][1]
        cuts = [(2, 0), (r["members"] + 3, 0), (r["len"], 0), (r["len"] + 1, 0), (r["chain"] + 6, 0), (r["div"] + q_n, q_lk), (r["merkle_m"] + 1000, n_lk),
                (ub + u["n_in"] + 700, n_lk), (lv1, n_lk), (lv1 + 25, n_lk), (r["sponge_new"] + 900, n_lk)]
        splits = [[x] for x in cuts] + [[cuts[1], cuts[5]], [cuts[4], cuts[6], cuts[9]]]
        # the seams: where the head ends, where M, MM, U and G start, U's assigned witnesses from its blocks, one cell into G
        splits += [[x] for x in ((r["members"], 0), (r["div"], 0), (r["merkle_m"], n_lk), (ub, n_lk), (ub + u["n_in"], n_lk), (r["sponge_new"], n_lk),
                                 (r["sponge_new"] + 1, n_lk))]
        for split in splits:
            edges = [(0, 0)] + split + [(cells, n_lk)]
            parts = []
            for (lo, llo), (hi, lhi) in zip(edges[:-1], edges[1:]):
                window = (lo, hi, llo, lhi)
                g_adv, g_lk = _windowed(api, lib, check, want, lk, window, run)
                _check_window(want, lk, g_adv, g_lk, window, (split, window))
                assert np.array_equal(d_pub.download((3, 4)), m["public"]), (split, window)
                assert np.array_equal(d_new.download((dim, 4)), m["new_centroid"]), (split, window)
                assert np.array_equal(d_lv.download(after.shape), after), (split, window)
                parts.append((g_adv[lo:hi], g_lk[llo:lhi]))
            assert np.array_equal(np.concatenate([p[0] for p in parts]), want), split
            assert np.array_equal(np.concatenate([p[1] for p in parts]), lk), split
    finally:
        for b in up:
            b.free()


def test_kernels_witness_and_flags_satisfy_the_map(api, O):
    from halo2_vectordb_amd import circuit_sym as CS
    from test_merkle_update_cpu import fetchers
    K, n_c, dim, c = 3, 65, 2, 0
    m, cent, mem, roots, before, after = case(O, K, n_c, dim, c)
    got = api.wit_ann_recentre(before, mem, roots[:K + 1], c, P, L, selectors=True)
    ff, fv, vals = fetchers(dict(advice=got["stream"], flags=got["flags"]))
    cm, public, info = CS.build_ann_recentre(K, n_c, dim, P, L, ff, fv)
    rep = cm.check_witness(vals, TM.to_ints(got["lookup"]), got["flags"])
    assert not any(rep.values()), rep
    assert [vals[x] for x in public] == TM.to_ints(got["public"])
    assert [int(cm.copy_of[x]) for x in info["new_vector"]] == info["mean"] and cm.copy_of[info["members_root"]] == info["picked"]
    assert cm.copy_of[info["update_public"][0]] == 1 and cm.copy_of[info["update_public"][1]] == 0


@pytest.mark.parametrize("K,n_c,dim,c", [(2, 2, 3, 1), (3, 1, 2, 2), (5, 3, 1, 0)])
def test_device_placed_map_is_the_host_builders(api, O, K, n_c, dim, c):
    from halo2_vectordb_amd.rounds import ProverRounds
    index, hp = _hot_path(O, K, n_c, dim, c)
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
        assert d[6] == h[6] and len(h[6]) == 3
        for i in (0, 2, 4, 5):
            assert np.array_equal(d[i], h[i]), i
        val = lambda x: np.where(x[1] >= 0, np.asarray(x[3] + [0], dtype=object)[np.maximum(x[1], -1)], -1)
        assert np.array_equal(val(d), val(h))
    finally:
        hp.free()
        index.free()


# ---------------------------------------------------------------------------------------------------------------- the proof
def test_proof_is_accepted_and_bound_to_both_roots_and_the_cluster(api, O):
    from halo2_vectordb_amd import verifier
    from halo2_vectordb_amd.rounds import ProverRounds
    K, n_c, dim, c = 2, 3, 4, 1
    index, hp = _hot_path(O, K, n_c, dim, c, k=13)             # the smallest k that holds the 2^12-entry table
    pr = None
    try:
        pr = ProverRounds(hp.setup()).keygen()
        assert pr.keygen_report.violations() == 0, pr.keygen_report.as_dict()
        out = pr.prove(None, seed=29)
        root_old, _, root_new, new = hp.results()
        assert np.array_equal(root_old, index.roots()[-1]) and np.array_equal(new, index.means()[c])
        want = [TM.to_ints(root_old[None])[0], c, TM.to_ints(root_new[None])[0]]
        assert out["instances"] == want and want[0] != want[2]
        vk = verifier.VerifyingKey.from_prover(pr, out["opened"])
        assert verifier.verify(out["proof"], want, vk)
        for i in range(3):
            wrong = list(want)
            wrong[i] = (wrong[i] + 1) % O.R_MOD
            assert not verifier.verify(out["proof"], wrong, vk), i
    finally:
        if pr is not None:
            pr.free()
        hp.free()
        index.free()


# ---------------------------------------------------------------------------------------------------------------- the index after it
def _buffers(ix):
    """every resident buffer of an index, downloaded"""
    return dict(grouped=ix.d_grouped.download((ix.n, ix.dim, 4)), slots=ix.d_slots.download((ix.n,), dtype=np.uint32),
                offsets=ix.d_offsets.download((ix.K + 1,), dtype=np.uint64), forest=ix.d_forest.download((ix.n_digests, 4)), roots=ix.roots(),
                centroids=ix.d_cent.download((ix.K, ix.dim, 4)))


def test_recentred_with_is_the_index_built_from_scratch_with_row_c_replaced(api, O):
    from halo2_vectordb_amd.pipeline import AnnIndex
    K, n_c, dim, c = 5, 70, 65, 4
    index, hp = _hot_path(O, K, n_c, dim, c)
    made = [index, hp]
    try:
        roots_before = index.roots()
        hp.setup()
        hp._witness()
        api.sync()
        api.profile_begin(deferred=True)
        ix2 = index.recentred_with(hp)
        made.append(ix2)
        api.sync()
        launches = {kern: int(v["launches"]) for kern, v in api.profile_end().items()}
        assert launches == {"k_mk_leaf_states": 1}, launches     # no k_ann_group, k_ann_forest_level, k_ann_gather, no member leaf
        cent2 = index.qcent.copy()
        cent2[c] = index.means()[c]
        fresh = AnnIndex(index.n, dim, K, index.qvec, index.cluster_ids, cent2, P=P, L=L)
        made.append(fresh)
        got, want = _buffers(ix2), _buffers(fresh)
        for name in want:
            assert np.array_equal(got[name], want[name]), name
        assert np.array_equal(ix2.qcent, cent2) and np.array_equal(ix2.roots()[-1], hp.results()[2])
        assert np.array_equal(index.roots(), roots_before) and np.array_equal(index.d_cent.download((K, dim, 4)), index.qcent)
    finally:
        for x in reversed(made):
            x.free()


def test_the_chain_over_all_clusters_ends_on_recentred_and_every_mean_audit_passes(api, O):
    from halo2_vectordb_amd.pipeline import AnnIndex, AnnMeanHotPath, AnnRecentreHotPath
    K, dim, sizes = 3, 2, (2, 1, 3)
    rng = np.random.default_rng(91)
    rows = rng.integers(-109, 110, (sum(sizes), dim)).astype(np.float64)
    ids = rng.permutation(np.repeat(np.arange(K), sizes))
    ix = AnnIndex(rows.shape[0], dim, K, rows, ids, rng.integers(-109, 110, (K, dim)).astype(np.float64), P=P, L=L)
    made = [ix]
    try:
        at, cur = ix.roots()[-1], ix
        for c in range(K):
            hp = AnnRecentreHotPath(cur, c, k=13, P=P, L=L, tau=TAU).setup()
            made.append(hp)
            hp._witness()
            api.sync()
            root_old, c_fr, root_new, _ = hp.results()
            assert np.array_equal(root_old, at) and TM.to_ints(c_fr[None]) == [c]
            cur = cur.recentred_with(hp)
            made.append(cur)
            at = root_new
            assert np.array_equal(cur.roots()[-1], at)
        target = ix.recentred()
        made.append(target)
        assert np.array_equal(cur.roots(), target.roots()) and np.array_equal(cur.qcent, target.qcent)
        for c in range(K):
            hm = AnnMeanHotPath(cur, c, k=13, P=P, L=L, tau=TAU).setup()
            made.append(hm)
            hm._witness()
            api.sync()
            root, _, ok = hm.results()
            assert ok.tolist() == [1] * dim and np.array_equal(root, at)
    finally:
        for x in reversed(made):
            x.free()


def test_an_update_then_a_recentre_chain_the_roots_and_restore_the_mean(api, O):
    from halo2_vectordb_amd.pipeline import AnnMeanHotPath, AnnRecentreHotPath, AnnUpdateHotPath
    K, n_c, dim, c = 2, 3, 4, 1
    cent, mem, clusters, _ = index_of(O, K, n_c, dim, c, at_mean=True)
    from halo2_vectordb_amd.pipeline import AnnIndex
    ids = np.concatenate([np.full(x.shape[0], j) for j, x in enumerate(clusters)])
    index = AnnIndex(ids.shape[0], dim, K, np.concatenate(clusters), ids, cent, P=P, L=L)
    made = [index]
    try:
        row = np.asarray([200.0, 3.0, 150.0, 77.0])
        au = AnnUpdateHotPath(index, c, ([n_c], row[None]), grow=None, k=13, tau=TAU).setup()
        made.append(au)
        au._witness()
        api.sync()
        ix2 = index.updated(au)
        made.append(ix2)
        before = AnnMeanHotPath(ix2, c, k=13, P=P, L=L, tau=TAU).setup()
        made.append(before)
        before._witness()
        api.sync()
        assert not before.results()[2].all()
        hp = AnnRecentreHotPath(ix2, c, k=13, P=P, L=L, tau=TAU).setup()
        made.append(hp)
        hp._witness()
        api.sync()
        root_old, _, root_new, new = hp.results()
        assert np.array_equal(root_old, au.results()[5]) and hp.n == n_c + 1
        ix3 = ix2.recentred_with(hp)
        made.append(ix3)
        assert np.array_equal(ix3.roots()[-1], root_new) and np.array_equal(new, MM.means(O, ix2.members(c), P, L))
        after = AnnMeanHotPath(ix3, c, k=13, P=P, L=L, tau=TAU).setup()
        made.append(after)
        after._witness()
        api.sync()
        root, _, ok = after.results()
        assert ok.tolist() == [1] * dim and np.array_equal(root, root_new)
    finally:
        for x in reversed(made):
            x.free()


def test_single_cell_alteration_sweep(api, O):
    """tests/alteration_model.py's method by the device sweep of tests/test_gpu_alteration.py at (K 2, n_c 2, dim 3, c 1): the map as the
    device placed it and the bytes the kernels wrote; a cell may stay free only by a rule of alteration_model.explain"""
    from test_gpu_alteration import device_sweep
    index, hp = _hot_path(O, 2, 2, 3, 1)
    try:
        device_sweep(api, O, "ann recentre K 2 n_c 2 c 1 dim 3", hp.setup())       # frees the hot path
    finally:
        index.free()
