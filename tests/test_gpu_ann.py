"""The approximate-nearest-neighbour index and query circuit on the GPU (pipeline.AnnIndex, AnnQueryHotPath; vdb_ann_index_build_dev,
vdb_wit_ann_query*): the resident index and the witness streams are tests/ann_model.py's bit for bit (tests/test_ann_cpu.py holds that model
against the oracle first); launch counts, refused arguments, the proof, and the binding of the cluster searched to the centroid that won."""
import ctypes

import numpy as np
import pytest

import ann_model as AN
import topk_model as TM
from test_gpu_rounds import TAU

pytestmark = pytest.mark.gpu
P, L, DIM = 48, 12, 4
SHAPES = {                                                   # n, K, ids
    "1-4-7": (12, 3, [2, 0, 1, 2, 1, 2, 1, 2, 2, 1, 2, 2]),
    "1-1": (2, 2, [1, 0]),
    "5": (5, 1, [0] * 5),
    "wave": (70, 5, [4 if i % 17 else i % 4 for i in range(70)]),
}


@pytest.fixture(scope="module")
def api():
    from halo2_vectordb_amd import api as a
    a.init(0)
    return a


def _rows(seed, n, dim=DIM):
    return np.random.default_rng(seed).integers(0, 219, size=(n, dim)).astype(np.float64)


def _setup(O, name, seed=40):
    n, K, ids = SHAPES[name]
    f = dict(db=_rows(seed, n), cent=_rows(seed + 1, K), query=_rows(seed + 2, 1)[0])
    return n, K, np.asarray(ids), f, O.quantize(f["db"], P), O.quantize(f["cent"], P), O.quantize(f["query"], P)


def _winner(O, query, cent):
    a = TM.topk_model(O, "euclidean", query[None], cent, 1, P, L, inputs=False)
    return int(np.flatnonzero(a["indicators"][0, 0].any(axis=1))[-1])


@pytest.mark.parametrize("name", list(SHAPES))
def test_index_is_the_models(api, O, name):
    n, K, ids, _, db, cent, _ = _setup(O, name)
    got, want = api.ann_index_build(db, ids, cent), AN.index_model(O, db, ids, cent)
    for key in ("grouped", "slots", "offsets", "roots"):
        assert np.array_equal(got[key], want[key]), key
    for s in range(K + 1):
        seg = got["forest"][int(got["segments"][s]):int(got["segments"][s + 1])]
        assert np.array_equal(seg, want["forest"][s]), s
        if s < K:
            assert np.array_equal(seg, api.merkle_tree_build(AN.select_cluster(db, ids, s)[0]))


def test_launch_count_does_not_depend_on_K_and_refused_arguments_launch_nothing(api, O):
    from halo2_vectordb_amd._lib import check
    lib = api.init()
    db = O.quantize(_rows(7, 12), P)
    counts = {}
    for K, ids in ((3, [0] * 8 + [1, 1, 2, 2]), (6, [0] * 7 + [1, 2, 3, 4, 5])):      # deepest tree: three levels (8 leaves) in both
        cent, ids = O.quantize(_rows(8, K), P), np.ascontiguousarray(ids, dtype=np.uint32)
        digests, _ = api.ann_forest_layout(ids, K)
        bufs = [api.DeviceBuffer(x) for x in (db.nbytes, cent.nbytes, db.nbytes, 12 * 4, (K + 1) * 8, digests * 32, (K + 2) * 32)]
        try:
            bufs[0].upload(db)
            bufs[1].upload(cent)
            run = lambda: check(lib.vdb_ann_index_build_dev(bufs[0].ptr, api._p(ids), bufs[1].ptr, 12, K, DIM, *[b.ptr for b in bufs[2:]]))
            run()
            api.sync()
            api.profile_begin(deferred=True)
            run()
            api.sync()
            counts[K] = {name: int(v["launches"]) for name, v in api.profile_end().items()}
            api.profile_begin(deferred=True)
            for bad_K, bad in ((K, [K] + [0] * 11), (K + 1, list(ids)), (0, list(ids))):     # id >= K, an empty cluster, K = 0
                with pytest.raises(api.VdbError) as e:
                    check(lib.vdb_ann_index_build_dev(bufs[0].ptr, api._p(np.ascontiguousarray(bad, dtype=np.uint32)), bufs[1].ptr, 12, bad_K, DIM,
                                                      *[b.ptr for b in bufs[2:]]))
                assert e.value.code == -3
            api.sync()
            assert api.profile_end() == {}
        finally:
            for b in bufs:
                b.free()
    assert counts[3] == counts[6] == dict(k_ann_group=1, k_ann_gather=1, k_mk_leaf_states=3, k_ann_forest_level=3, k_ann_roots=1), counts


def _witness_case(api, O, name, cluster=None):
    n, K, ids, _, db, cent, query = _setup(O, name)
    ix = AN.index_model(O, db, ids, cent)
    w = _winner(O, query, cent) if cluster is None else cluster
    members, _ = AN.select_cluster(db, ids, w)
    assert AN.distances_distinct(O, "euclidean", query, cent, P, L) and AN.distances_distinct(O, "euclidean", query, members, P, L)
    return query, cent, members, ix["roots"][1:1 + K], ix


@pytest.mark.parametrize("name", list(SHAPES))
def test_host_witness_is_the_models(api, O, name):
    query, cent, members, roots, ix = _witness_case(api, O, name)
    m = AN.query_model(O, "euclidean", query, cent, members, roots, P, L)
    got = api.wit_ann_query("euclidean", query, cent, members, roots, P, L, selectors=True)
    assert got["n_in"] == m["n_in"] and got["stream"].shape == m["advice"].shape
    assert np.array_equal(got["stream"], m["advice"]) and np.array_equal(got["lookup"], m["lookup"])
    assert np.array_equal(got["selectors"], m["selectors"])
    # the flag bytes beyond the gate bit (constant cells, lookup sources), of which the oracle keeps none, are the generators': every
    # block's are those of the block emitted alone (the members' tree copies the zero cell where the centroids' padding has loaded it);
    # the assigned inputs and the selection hold no constant cell
    r, K, block = m["regions"], cent.shape[0], np.zeros(got["flags"].shape[0], dtype=bool)
    zero = (1 << (K - 1).bit_length()) > K
    words = np.concatenate([ix["roots"][:1], roots])[None]
    for lo, hi, alone in ((r["nearest_c"], r["merkle_c"], api.wit_nearest("euclidean", query, cent, P, L, selectors=True)),
                          (r["merkle_c"], r["nearest_m"], api.wit_merkle(cent, selectors=True)),
                          (r["nearest_m"], r["merkle_m"], api.wit_nearest("euclidean", query, members, P, L, selectors=True)),
                          (r["merkle_m"], r["select"], api.wit_merkle(members, zero_cached=zero, selectors=True)),
                          (r["sponge"], got["flags"].shape[0], api.wit_merkle(words, selectors=True))):
        assert np.array_equal(got["flags"][lo:hi], alone["flags"]) and np.array_equal(got["stream"][lo:hi], alone["stream"]), lo
        block[lo:hi] = True
    assert np.array_equal(got["flags"][~block], m["selectors"][~block])
    assert np.array_equal(got["centroid_indicator"], m["centroid_indicator"]) and np.array_equal(got["member_indicator"], m["member_indicator"])
    assert np.array_equal(got["public"], m["public"]) and np.array_equal(got["index_root"], ix["roots"][-1])


def test_kernels_witness_and_flags_satisfy_the_map(api, O):
    """the stream and the flag bytes as the kernels wrote them, held against circuit_sym.build_ann_query on the host builder: no copy, constant
    or lookup of the map is violated, the gate bits are the map's and no cell is flagged constant that the map does not hold constant"""
    from halo2_vectordb_amd import circuit_sym as CS
    from test_merkle_update_cpu import fetchers
    query, cent, members, roots, _ = _witness_case(api, O, "1-4-7")
    got = api.wit_ann_query("euclidean", query, cent, members, roots, P, L, selectors=True)
    ff, fv, vals = fetchers(dict(advice=got["stream"], flags=got["flags"]))
    cm, public, info = CS.build_ann_query("euclidean", cent.shape[0], members.shape[0], DIM, P, L, ff, fv)
    rep = cm.check_witness(vals, TM.to_ints(got["lookup"]), got["flags"])
    assert not any(rep.values()), rep
    assert [vals[c] for c in public] == TM.to_ints(got["public"]) and cm.copy_of[info["selected"]] == info["members_root"]


def _hot_path(O, name, k=13, **kw):
    from halo2_vectordb_amd.pipeline import AnnIndex, AnnQueryHotPath
    n, K, ids, f, db, cent, query = _setup(O, name)
    index = AnnIndex(n, DIM, K, f["db"], ids, f["cent"], P=P, L=L)
    return index, AnnQueryHotPath(index, f["query"], k=k, P=P, L=L, tau=TAU, **kw)


def test_hot_path_is_the_model_split_windows_and_resident_roots(api, O):
    from halo2_vectordb_amd._lib import check
    query, cent, members, roots, ix = _witness_case(api, O, "1-4-7")
    m = AN.query_model(O, "euclidean", query, cent, members, roots, P, L, plan_k=13)
    index, hp = _hot_path(O, "1-4-7")
    try:
        assert np.array_equal(index.roots(), ix["roots"])
        hp.setup()
        assert hp.n_cells == m["advice"].shape[0] and hp.n_in == m["n_in"] and hp.n_lookup == m["lookup"].shape[0]
        assert np.array_equal(hp.bp, m["break_points"])
        d_flags = hp.keygen_flags()
        assert np.array_equal(d_flags.download((hp.n_cells,), dtype=np.uint8) & 1, m["selectors"])
        d_flags.free()
        hp._witness()
        api.sync()
        assert np.array_equal(hp.d_stream.download((hp.n_cells, 4)), m["advice"]) and np.array_equal(hp.d_lookup.download((hp.n_lookup, 4)), m["lookup"])
        ind_c, ind_m, res, root = hp.results()
        assert np.array_equal(ind_c, m["centroid_indicator"]) and np.array_equal(ind_m, m["member_indicator"])
        assert np.array_equal(res, m["result"]) and np.array_equal(root, ix["roots"][-1])
        # a two-way window split reproduces the unsplit stream
        lib, cut, lcut = hp.lib, hp.n_cells // 2 + 3, hp.n_lookup // 2 + 1
        check(lib.vdb_memset_dev(hp.d_stream.ptr, 0xA5, ctypes.c_size_t(hp.n_cells * 32)))
        check(lib.vdb_memset_dev(hp.d_lookup.ptr, 0xA5, ctypes.c_size_t(hp.n_lookup * 32)))
        for adv, lk in (((0, cut), (0, lcut)), ((cut, hp.n_cells), (lcut, hp.n_lookup))):
            with api.wit_window(adv=adv, lookup=lk):
                hp._witness()
        api.sync()
        assert np.array_equal(hp.d_stream.download((hp.n_cells, 4)), m["advice"]) and np.array_equal(hp.d_lookup.download((hp.n_lookup, 4)), m["lookup"])
    finally:
        hp.free()
        index.free()


def test_proof_is_accepted_and_bound_to_the_index_root(api, O):
    from halo2_vectordb_amd import verifier
    from halo2_vectordb_amd.rounds import ProverRounds
    query, cent, members, roots, ix = _witness_case(api, O, "1-4-7")
    assert members.shape[0] == 7
    index, hp = _hot_path(O, "1-4-7")
    pr = None
    try:
        pr = ProverRounds(hp.setup()).keygen()
        assert pr.keygen_report.violations() == 0, pr.keygen_report.as_dict()
        out = pr.prove(None, seed=17)
        want = TM.to_ints(AN.query_model(O, "euclidean", query, cent, members, roots, P, L)["public"])
        assert out["instances"] == want and len(want) == DIM + 1
        vk = verifier.VerifyingKey.from_prover(pr, out["opened"])
        assert verifier.verify(out["proof"], want, vk)
        wrong = list(want)
        wrong[-1] = (wrong[-1] + 1) % O.R_MOD
        assert not verifier.verify(out["proof"], wrong, vk)
    finally:
        if pr is not None:
            pr.free()
        hp.free()
        index.free()


def test_wrong_cluster_and_altered_root_are_noticed(api, O):
    """the binding: a cluster other than the winning centroid's breaks the sel = mroot copy; so does an altered cluster root, and an
    altered centroid coordinate changes the index root"""
    from halo2_vectordb_amd import circuit_sym as CS
    from halo2_vectordb_amd.pipeline import AnnIndex, AnnQueryHotPath
    from halo2_vectordb_amd.rounds import ProverRounds
    n, K, ids, f, db, cent, query = _setup(O, "1-4-7")
    w = _winner(O, query, cent)
    index = AnnIndex(n, DIM, K, f["db"], ids, f["cent"], P=P, L=L)
    good_root = index.roots()[-1]
    roots = index.roots()[1:1 + K].copy()
    roots[w] = O.fr_add(roots[w:w + 1], O.fr_from_ints([1]))[0]
    cent2 = cent.copy()
    cent2[(w + 1) % K, 0] = O.fr_add(cent2[(w + 1) % K, :1], O.fr_from_ints([1]))[0]
    try:
        assert index.probe(f["query"]) == w
        for kw, broken in ((dict(cluster=(w + 1) % K), True), (dict(cluster_roots=roots), True), (dict(centroids=cent2), False)):
            hp = AnnQueryHotPath(index, f["query"], k=13, P=P, L=L, tau=TAU, **kw).setup()
            pr = ProverRounds(hp).keygen()
            try:
                rep = pr.keygen_report
                assert (rep.violations() >= 1) == broken, (kw.keys(), rep.as_dict())
                if broken:
                    # the one copy that breaks is the selection's output against the members' root: build_ann_query's `selected`
                    # (the last cell before the sponge, tests/test_ann_cpu.py)
                    selected = CS.ann_query_layout("euclidean", K, hp.n, DIM, P, L)["sponge"] - 1
                    assert rep.copies_unequal >= 1 and rep.first_copy == selected, rep.as_dict()
                else:
                    assert not np.array_equal(hp.results()[3], good_root)
            finally:
                pr.free()
                hp.free()
    finally:
        index.free()


def test_read_opens_a_member_against_its_cluster_root(api, O):
    from halo2_vectordb_amd.pipeline import AnnIndex, ReadHotPath
    n, K, ids, f, db, cent, _ = _setup(O, "1-4-7")
    index = AnnIndex(n, DIM, K, f["db"], ids, f["cent"], P=P, L=L)
    hp = None
    try:
        c = 2
        members = f["db"][np.flatnonzero(ids == c)]
        hp = ReadHotPath(n=len(members), dim=DIM, m=2, k=13, P=P, tau=TAU, vectors=members, levels=index.levels(c), reads=[0, 6]).setup()
        hp._witness()
        api.sync()
        assert np.array_equal(hp.results()[0], index.roots()[1 + c])
        assert np.array_equal(hp.results()[3], O.quantize(members[[0, 6]], P))
    finally:
        if hp is not None:
            hp.free()
        index.free()


def test_query_launch_count_depends_on_neither_K_nor_the_cluster_size_and_one_resident_tree_alone_is_refused(api, O):
    """with both trees read from the forest the witness call launches the same kernels the same number of times at K 3, n_c 7 and at K 5,
    n_c 65 (the library's event profiler); a call that names one resident tree without the other is refused before anything is launched"""
    from halo2_vectordb_amd._lib import check
    counts = {}
    for name, cluster in (("1-4-7", 2), ("wave", 4)):          # the cluster is named: the count, not the binding, is in question
        index, hp = _hot_path(O, name, cluster=cluster)
        try:
            hp.setup()
            hp._witness()
            api.sync()
            api.profile_begin(deferred=True)
            hp._witness()
            api.sync()
            counts[name] = (hp.K, hp.n, {kern: int(v["launches"]) for kern, v in api.profile_end().items()})
            api.profile_begin(deferred=True)
            for lc, lm in ((index.levels_ptr(hp.K), None), (None, index.levels_ptr(hp.cluster))):
                with pytest.raises(api.VdbError) as e:
                    check(hp.lib.vdb_wit_ann_query_dev(hp.metric, P, L, hp.d_vec.ptr, hp.p_cent, index.members_ptr(hp.cluster), hp.p_roots, lc, lm, hp.K, hp.n,
                                                       DIM, hp.d_stream.ptr, hp.d_lookup.ptr, None, hp.d_ind_c.ptr, hp.d_ind_m.ptr, hp.d_pub.ptr))
                assert e.value.code == -3
            api.sync()
            assert api.profile_end() == {}
        finally:
            hp.free()
            index.free()
    (K0, n0, c0), (K1, n1, c1) = counts["1-4-7"], counts["wave"]
    assert (K0, n0, K1, n1) == (3, 7, 5, 65) and c0 == c1 and sum(c0.values()) >= 1, counts


def test_single_cluster_entry_points_refuse_what_they_refused_and_launch_nothing(api, O):
    """vdb_wit_ann_query_size and vdb_wit_ann_query_dev forward to vdb_wit_ann_probe*: K = 0, an empty cluster, dim = 0, a cluster above
    VDB_ANN_MAX_VECTORS and (the device call) null members are VDB_ERR_ARG as they were, before anything is launched"""
    from halo2_vectordb_amd._lib import check
    index, hp = _hot_path(O, "1-1")
    try:
        hp.setup()
        hp._witness()
        api.sync()
        lc, lm, members = index.levels_ptr(hp.K), index.levels_ptr(hp.cluster), index.members_ptr(hp.cluster)
        cells, lk, n_in = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
        dev = lambda K, n_c, dim, mem: hp.lib.vdb_wit_ann_query_dev(hp.metric, P, L, hp.d_vec.ptr, hp.p_cent, mem, hp.p_roots, lc, lm, K, n_c, dim,
                                                                    hp.d_stream.ptr, hp.d_lookup.ptr, None, hp.d_ind_c.ptr, hp.d_ind_m.ptr, hp.d_pub.ptr)
        size = lambda K, n_c, dim: hp.lib.vdb_wit_ann_query_size(hp.metric, P, L, K, n_c, dim, ctypes.byref(cells), ctypes.byref(lk), ctypes.byref(n_in))
        check(size(hp.K, hp.n, DIM))
        assert (cells.value, lk.value, n_in.value) == (hp.n_cells, hp.n_lookup, hp.n_in)
        api.profile_begin(deferred=True)
        for K, n_c, dim in ((0, hp.n, DIM), (hp.K, 0, DIM), (hp.K, hp.n, 0), (hp.K, (1 << 24) + 1, DIM)):
            for call in (lambda: size(K, n_c, dim), lambda: dev(K, n_c, dim, members)):
                with pytest.raises(api.VdbError) as e:
                    check(call())
                assert e.value.code == -3, (K, n_c, dim)
        with pytest.raises(api.VdbError) as e:
            check(dev(hp.K, hp.n, DIM, None))
        assert e.value.code == -3
        api.sync()
        assert api.profile_end() == {}
    finally:
        hp.free()
        index.free()


def test_single_cluster_hot_path_is_the_probe_at_one_cluster_and_one_neighbour(api, O):
    from halo2_vectordb_amd.pipeline import AnnProbeQueryHotPath
    n, K, ids, f, db, cent, query = _setup(O, "1-4-7")
    index, hp = _hot_path(O, "1-4-7")
    try:
        assert isinstance(hp, AnnProbeQueryHotPath) and hp.probes == hp.topk == 1
        assert hp.cluster == index.probe(f["query"]) == _winner(O, query, cent) and hp.clusters == [hp.cluster]
        hp.setup()
        hp._witness()
        api.sync()
        ind_c, ind_m, res, root = hp.results()
        assert (ind_c.shape, ind_m.shape, res.shape, root.shape) == ((K, 4), (hp.n, 4), (DIM, 4), (4,)) and hp.n == 7
        slots = np.flatnonzero((db == res[None]).all(axis=(1, 2)))
        assert len(slots) == 1 and np.array_equal(hp.neighbours(), slots)
    finally:
        hp.free()
        index.free()


def test_single_cluster_c_entry_points_write_the_hot_paths_and_the_wrappers_bytes(api, O):
    """vdb_wit_ann_query_dev and vdb_wit_ann_query called as vdb.h declares them: the device form, with the two resident trees and with
    neither, fills fresh buffers with the hot path's stream, lookup stream, indicators and public values (which
    test_hot_path_is_the_model_split_windows_and_resident_roots holds to the model); the host form gives api.wit_ann_query's arrays"""
    from halo2_vectordb_amd._lib import check
    query, cent, members, roots = (np.ascontiguousarray(a, dtype=np.uint64) for a in _witness_case(api, O, "1-4-7")[:4])
    index, hp = _hot_path(O, "1-4-7")
    K, n_c = hp.K, hp.n
    bufs = []
    try:
        hp.setup()
        hp._witness()
        api.sync()
        sizes = dict(stream=hp.n_cells, lookup=hp.n_lookup, ind_c=K, ind_m=n_c, pub=DIM + 1)
        want = dict(stream=hp.d_stream.download((hp.n_cells, 4)), lookup=hp.d_lookup.download((hp.n_lookup, 4)), ind_c=hp.d_ind_c.download((K, 4)),
                    ind_m=hp.d_ind_m.download((n_c, 4)), pub=hp.d_pub.download((DIM + 1, 4)))
        for lc, lm in ((index.levels_ptr(K), index.levels_ptr(hp.cluster)), (None, None)):
            d = {key: api.DeviceBuffer(rows * 32) for key, rows in sizes.items()}
            bufs += list(d.values())
            for b in d.values():
                check(hp.lib.vdb_memset_dev(b.ptr, 0xA5, ctypes.c_size_t(b.nbytes)))
            check(hp.lib.vdb_wit_ann_query_dev(hp.metric, P, L, hp.d_vec.ptr, hp.p_cent, index.members_ptr(hp.cluster), hp.p_roots, lc, lm, K, n_c, DIM,
                                               d["stream"].ptr, d["lookup"].ptr, None, d["ind_c"].ptr, d["ind_m"].ptr, d["pub"].ptr))
            api.sync()
            for key, rows in sizes.items():
                assert np.array_equal(d[key].download((rows, 4)), want[key]), (key, lc is None)
        got = api.wit_ann_query("euclidean", query, cent, members, roots, P, L, selectors=True)
        assert np.array_equal(got["stream"], want["stream"]) and np.array_equal(got["lookup"], want["lookup"])
        h = dict(stream=np.zeros((hp.n_cells, 4), dtype=np.uint64), lookup=np.zeros((hp.n_lookup, 4), dtype=np.uint64), flags=np.zeros(hp.n_cells, dtype=np.uint8),
                 centroid_indicator=np.zeros((K, 4), dtype=np.uint64), member_indicator=np.zeros((n_c, 4), dtype=np.uint64),
                 public=np.zeros((DIM + 1, 4), dtype=np.uint64))
        check(hp.lib.vdb_wit_ann_query(hp.metric, P, L, api._p(query), api._p(cent), api._p(members), api._p(roots), K, n_c, DIM, *[api._p(a) for a in h.values()]))
        for key, a in h.items():
            assert np.array_equal(a, got[key]), key
    finally:
        for b in bufs:
            b.free()
        hp.free()
        index.free()


@pytest.mark.parametrize("name", ["1-1", "5"])
def test_single_cell_alteration_sweep(api, O, name):
    """tests/alteration_model.py's method on this circuit at its two smallest shapes, by the device sweep of tests/test_gpu_alteration.py: the
    map as the device placed it and the bytes the kernels wrote; every cell the model calls bound — the selection, the selected root, the
    sponge's words and the shared zero cell among them — is noticed by the device MockProver when altered alone.  No allow-list is kept
    here: a cell may stay free only by a rule of alteration_model.explain (the reference's is_zero inverse of a zero operand), and
    tests/test_ann_alteration_cpu.py holds that none of the cells this circuit adds is among them."""
    from test_gpu_alteration import device_sweep
    index, hp = _hot_path(O, name)
    try:
        device_sweep(api, O, f"ann euclidean {name} dim {DIM}", hp.setup())       # frees the hot path
    finally:
        index.free()


def test_index_roots_are_the_demo_flows_roots(api, O):
    """tests/test_gpu_demo.py's (dim 4, n 12, K 3, I 3) case rebuilt: the roots GpuDemoZKDB reads off K + 2 witness streams are the index's —
    the centroids' root, every cluster's root, and the database's root as the one cluster of an index with K = 1 —, and one query through
    the one circuit searches the cluster and returns the vector the demo's two circuits do"""
    from halo2_vectordb_amd.pipeline import AnnIndex, AnnQueryHotPath
    from test_gpu_demo import L as DL, P as DP, GpuDemoZKDB, f64_kmeans
    dim, n, K, I, seed = 4, 12, 3, 3, 2
    rng = np.random.default_rng(1000 + seed)
    while True:
        db = rng.random((n, dim))
        _, ids = f64_kmeans(db, K, I)
        if len(set(ids)) == K:
            break
    zk = GpuDemoZKDB(api, O, db, K, I)
    assert zk.cluster_ids == ids
    index = AnnIndex(n, dim, K, db, zk.cluster_ids, zk.centroids, P=DP, L=DL)
    whole = AnnIndex(n, dim, 1, db, [0] * n, zk.centroids[:1], P=DP, L=DL)
    hp = None
    try:
        roots = index.roots()
        assert np.array_equal(roots[0], zk.centroids_root)
        for c in range(K):
            assert np.array_equal(roots[1 + c], zk.cluster_roots[c]), c
        assert np.array_equal(whole.roots()[1], zk.database_root)
        q = rng.random(dim)
        cid, _, _ = zk.chip_nearest(q, zk.centroids)
        hp = AnnQueryHotPath(index, q, k=14, P=DP, L=DL, tau=TAU).setup()
        hp._witness()
        api.sync()
        assert hp.cluster == cid
        assert np.array_equal(api.dequantize(hp.results()[2], DP), zk.ann(q)) and np.array_equal(hp.results()[3], roots[-1])
    finally:
        if hp is not None:
            hp.free()
        whole.free()
        index.free()
