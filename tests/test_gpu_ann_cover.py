"""The cover of the database by the index on the GPU (pipeline.AnnCoverHotPath, vdb_wit_ann_cover*; AnnIndex.database_tree,
vdb_ann_index_db_tree_dev): the streams are tests/ann_cover_model.py's bit for bit (tests/test_ann_cover_cpu.py holds that model against
the host-built map first); the resident, the host-array and the device form, the database tree against the tree builder, refused slots
and arguments, the launch lists, rank windows, the device-placed map, the Mock report, the proof, the chain build -> updated -> removed,
and the alteration sweep."""
import ctypes

import numpy as np
import pytest

import alteration_model as AM
import ann_cover_model as CM
import topk_model as TM
from test_ann_cover_cpu import DIM, L, P, SHAPES, database, database_f64, leaves_of
from test_gpu_batch_query import _dev
from test_gpu_rounds import TAU
from test_gpu_sweep import _check_window, _windowed

pytestmark = pytest.mark.gpu

# n = 300, 1,019 nodes, about 4.6 M cells: wavefront and tree borders in k_annc_forest_trace, stretches of two with a ragged tail in
# k_annc_products
BIG = (1, 40, 64, 65, 130)
CASES = SHAPES[:3] + [BIG]
_cache = {}


@pytest.fixture(scope="module")
def api():
    from halo2_vectordb_amd import api as a
    a.init(0)
    return a


def case(O, sizes):
    """-> (model, rows, ids, centroids, a, b), computed once per shape and shared; nothing changes it"""
    if sizes not in _cache:
        rows, ids, cent = database(O, sizes)
        a, b, _ = leaves_of(O, rows, ids, len(sizes))
        _cache[sizes] = (CM.cover_model(O, a, b, sizes, O.poseidon_merkle_root(cent)), rows, ids, cent, a, b)
    return _cache[sizes]


def _index(O, sizes):
    from halo2_vectordb_amd.pipeline import AnnIndex
    rows, ids, cent = database(O, sizes)
    return AnnIndex(rows.shape[0], DIM, len(sizes), rows, ids, cent, P=P, L=13)


def _hot_path(O, sizes, k=15, **kw):
    from halo2_vectordb_amd.pipeline import AnnCoverHotPath
    index = _index(O, sizes)
    return index, AnnCoverHotPath(index, k=k, L=L, tau=TAU, **kw)


def _differ(got, want):
    return np.flatnonzero((got != want).any(axis=1) if got.ndim == 2 else got != want)


@pytest.mark.parametrize("sizes", CASES)
def test_witness_is_the_models_resident_from_device_leaves_and_from_host_arrays(api, O, sizes):
    from halo2_vectordb_amd import circuit_sym as CS
    from halo2_vectordb_amd._lib import check
    m, rows, ids, cent, a, b = case(O, sizes)
    K, n = len(sizes), sum(sizes)
    croot = O.poseidon_merkle_root(cent)
    host = api.wit_ann_cover(a, b, sizes, croot, selectors=True)
    assert host["n_in"] == m["n_in"] == K + 1 + 2 * n and host["stream"].shape == m["advice"].shape
    bad = _differ(host["stream"], m["advice"])
    assert bad.size == 0, f"first differing advice cells {bad[:5]} of {host['stream'].shape[0]} (blocks {m['regions']})"
    bad = _differ(host["flags"], m["flags"])
    assert bad.size == 0, f"first differing flag bytes at {bad[:8]}: {host['flags'][bad[:8]]} against {m['flags'][bad[:8]]} (blocks {m['regions']})"
    assert np.array_equal(host["public"], m["public"])
    lay = CS.ann_cover_layout(sizes)                         # ann_cover_layout is annc_blocks through vdb_wit_ann_cover_size
    assert (lay["total"], lay["n_in"]) == (host["stream"].shape[0], host["n_in"])
    index, hp = _hot_path(O, sizes)
    up = []
    try:
        # the database tree of the index is the tree builder's over the rows in slot order, and so is its root
        want_tree = api.merkle_tree_build(index.qvec)
        lp = want_tree.shape[0] // 2
        assert np.array_equal(index.database_tree().download((2 * lp, 4)), want_tree)
        assert index.database_tree() is index.database_tree()
        assert np.array_equal(want_tree[2 * lp - 2], m["public"][0]) and np.array_equal(index.roots()[-1], m["public"][1])
        forest = index.d_forest.download((index.n_digests, 4))
        slots = index.d_slots.download((n,), dtype=np.uint32)
        assert np.array_equal(api.ann_index_db_tree(forest, sizes, slots), want_tree)
        hp.setup()
        assert hp.resident and (hp.n_cells, hp.n_in, hp.n_lookup) == (m["advice"].shape[0], m["n_in"], 0)
        d_flags = hp.keygen_flags()
        assert np.array_equal(d_flags.download((hp.n_cells,), dtype=np.uint8), m["flags"])
        d_flags.free()
        d_a, d_b = _dev(api, up, a), _dev(api, up, b)
        for resident in (True, False):
            check(hp.lib.vdb_memset_dev(hp.d_stream.ptr, 0xA5, ctypes.c_size_t(hp.n_cells * 32)))
            check(hp.lib.vdb_memset_dev(hp.d_pub.ptr, 0xA5, ctypes.c_size_t(2 * 32)))
            if not resident:                                     # the device form over the two leaf arrays: the K + 1 trees are hashed by the call
                hp.resident, hp.p_tree, hp.p_a, hp.p_b = False, None, d_a.ptr, d_b.ptr
            hp._witness()
            api.sync()
            bad = _differ(hp.d_stream.download((hp.n_cells, 4)), m["advice"])
            assert bad.size == 0, (resident, bad[:5], m["regions"])
            assert np.array_equal(np.stack(hp.results()), m["public"]), resident
    finally:
        for x in up:
            x.free()
        hp.free()
        index.free()


def test_slots_that_are_no_permutation_are_refused(api, O):
    from halo2_vectordb_amd._lib import check
    sizes = (3, 1, 5)
    index = _index(O, sizes)
    up = []
    try:
        n = index.n
        slots = index.d_slots.download((n,), dtype=np.uint32)
        assert sorted(slots.tolist()) == list(range(n))
        sizes64 = np.ascontiguousarray(sizes, dtype=np.uint64)
        d_out = api.DeviceBuffer(2 * 16 * 32)
        up.append(d_out)
        repeated, beyond = slots.copy(), slots.copy()
        repeated[4] = repeated[2]
        beyond[n - 1] = n
        for bad_slots in (repeated, beyond):
            d_s = _dev(api, up, bad_slots)
            with pytest.raises(api.VdbError) as e:
                check(index.lib.vdb_ann_index_db_tree_dev(index.d_forest.ptr, api._p(sizes64), d_s.ptr, len(sizes), n, d_out.ptr))
            assert e.value.code == -3 and "permutation" in str(e.value)
        d_s = _dev(api, up, slots)
        check(index.lib.vdb_ann_index_db_tree_dev(index.d_forest.ptr, api._p(sizes64), d_s.ptr, len(sizes), n, d_out.ptr))
        assert np.array_equal(d_out.download((32, 4)), api.merkle_tree_build(index.qvec))
        # before anything is launched: sizes that do not sum to n, an empty cluster, K = 0
        api.sync()
        api.profile_begin(deferred=True)
        for s, K_, n_ in ((sizes64, 3, n + 1), (np.asarray([3, 0, 6], dtype=np.uint64), 3, n), (sizes64, 0, n), (sizes64, 3, 0)):
            assert index.lib.vdb_ann_index_db_tree_dev(index.d_forest.ptr, api._p(s), d_s.ptr, K_, n_, d_out.ptr) == -3
        api.sync()
        assert api.profile_end() == {}
    finally:
        for x in up:
            x.free()
        index.free()


def test_launch_list_depends_on_neither_k_nor_n_and_refused_arguments_launch_nothing(api, O):
    from halo2_vectordb_amd import circuit_sym as CS
    from halo2_vectordb_amd._lib import check
    counts = {}
    for sizes in ((1, 2), BIG):
        index, hp = _hot_path(O, sizes)
        try:
            hp.setup()
            hp._witness()
            api.sync()
            api.profile_begin(deferred=True)
            hp._witness()
            api.sync()
            counts[sizes] = {kern: int(v["launches"]) for kern, v in api.profile_end().items()}
            if sizes != (1, 2):
                continue
            lib, n, K = hp.lib, hp.n, hp.K
            d_out = api.DeviceBuffer(1 << 16)
            check(lib.vdb_memset_dev(d_out.ptr, 0xA5, ctypes.c_size_t(1 << 16)))
            api.sync()
            api.profile_begin(deferred=True)
            tree, forest, croot = index.database_tree().ptr, index.d_forest.ptr, index.d_roots.ptr
            u64 = lambda *x: np.asarray(x, dtype=np.uint64)

            def call(s=u64(*sizes), K_=K, n_=n, tree_=tree, forest_=forest):
                return lib.vdb_wit_ann_cover_dev(None, None, croot, api._p(s), K_, n_, tree_, forest_, d_out.ptr, None, d_out.at(1 << 15))
            big = 1 << 24
            huge = u64(1 << 21)                                  # one cluster of 2^21 rows: about 1.9e10 cells
            assert 2 * ((1 << 21) - 1) * CM.NODE > 1 << 34
            refused = [dict(K_=0), dict(s=u64(*([1] * 4097)), K_=4097, n_=4097), dict(s=u64(1, 0, 2), K_=3), dict(s=u64(big, 1), n_=big + 1),
                       dict(n_=n + 1), dict(n_=n - 1), dict(s=huge, K_=1, n_=1 << 21), dict(tree_=None), dict(forest_=None)]
            for kw in refused:
                with pytest.raises(api.VdbError) as e:
                    check(call(**kw))
                assert e.value.code == -3, kw
            for kw in refused[:7]:                               # the size call shares the layout and writes nothing
                cells = ctypes.c_uint64()
                s = kw.get("s", u64(*sizes))
                assert lib.vdb_wit_ann_cover_size(api._p(s), kw.get("K_", K), kw.get("n_", n), ctypes.byref(cells), None) == -3, kw
            api.sync()
            assert api.profile_end() == {}
            assert (d_out.download((1 << 16,), dtype=np.uint8) == 0xA5).all()
            d_out.free()
        finally:
            hp.free()
            index.free()
    a, b = counts[(1, 2)], counts[BIG]
    assert a == b, counts
    assert a == {"k_annc_inputs": 1, "k_push_cells": 1, "k_annc_forest_trace": 1, "k_mk_leaf_states": 2, "k_mk_leaf_trace": 2, "k_annc_products": 1}, counts


def test_windowed_calls_write_the_bytes_of_one(api, O):
    from halo2_vectordb_amd._lib import check
    lib = api.init()
    sizes = (3, 1, 5)
    m, rows, ids, cent, a, b = case(O, sizes)
    K, n = len(sizes), sum(sizes)
    want, r, lk = m["advice"], m["regions"], np.zeros((0, 4), dtype=np.uint64)
    cells = want.shape[0]
    up = []
    try:
        d_a, d_b, d_c = _dev(api, up, a), _dev(api, up, b), _dev(api, up, O.poseidon_merkle_root(cent))
        d_pub = api.DeviceBuffer(64)
        up.append(d_pub)
        s64 = np.ascontiguousarray(sizes, dtype=np.uint64)

        def run(d_adv, d_lkb):
            check(lib.vdb_wit_ann_cover_dev(d_a.ptr, d_b.ptr, d_c.ptr, api._p(s64), K, n, None, None, d_adv.ptr, None, d_pub.ptr))
        # three windows each: inside the header and inside b; on the zero cell and inside the second permutation of a database node;
        # at the seam TD | TC and inside cluster 2's tree; inside D and inside G; inside a g_sub of SA and a g_mul of MA; at SB and
        # inside MB; the last cell alone
        node = CM.NODE
        splits = [[2, r["b"] + 4], [r["zero"], r["tree_d"] + 3 * node + 2300], [r["tree_c"], r["tree_c_at"][2] + node + 17],
                  [r["sponge"] + 900, r["gamma"] + 2251], [r["sub_a"] + 4 * 3 + 1, r["mul_a"] + 4 * 2 + 2], [r["sub_b"], r["mul_b"] + 5],
                  [r["zero"] + 1, cells - 1]]
        for split in splits:
            edges = [0] + split + [cells]
            parts = []
            for lo, hi in zip(edges[:-1], edges[1:]):
                window = (lo, hi, 0, 0)
                g_adv, g_lk = _windowed(api, lib, check, want, lk, window, run)
                _check_window(want, lk, g_adv, g_lk, window, (split, window))
                assert np.array_equal(d_pub.download((2, 4)), m["public"]), (split, window)
                parts.append(g_adv[lo:hi])
            assert len(parts) == 3 and np.array_equal(np.concatenate(parts), want), split
    finally:
        for x in up:
            x.free()


@pytest.mark.parametrize("sizes", SHAPES[:3])
def test_device_placed_map_is_the_host_builders(api, O, sizes):
    from halo2_vectordb_amd.rounds import ProverRounds
    index, hp = _hot_path(O, sizes, k=12)
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
        assert d[6] == h[6] and len(h[6]) == 2
        for i in (0, 2, 4, 5):
            assert np.array_equal(d[i], h[i]), i
        val = lambda x: np.where(x[1] >= 0, np.asarray(x[3] + [0], dtype=object)[np.maximum(x[1], -1)], -1)
        assert np.array_equal(val(d), val(h))
    finally:
        hp.free()
        index.free()


def test_kernels_witness_and_flags_satisfy_the_device_placed_map_at_n_300(api, O):
    from halo2_vectordb_amd.rounds import ProverRounds
    m, *_ = case(O, BIG)
    index, hp = _hot_path(O, BIG, k=15)
    pr = None
    try:
        pr = ProverRounds(hp.setup()).keygen()
        assert pr.keygen_report.violations() == 0, pr.keygen_report.as_dict()
        assert [int(c) for c in pr.instance_cells] == [m["droot_cell"], m["iroot_cell"]]
        rep = pr.mock_check(None, TM.to_ints(m["public"]))
        assert rep.violations() == 0, rep.as_dict()
    finally:
        if pr is not None:
            pr.free()
        hp.free()
        index.free()


# ---------------------------------------------------------------------------------------------------------------- the proof
def test_proof_is_accepted_bound_to_both_roots_and_its_database_root_is_the_merkle_circuits(api, O):
    from halo2_vectordb_amd import verifier
    from halo2_vectordb_amd.pipeline import MerkleHotPath
    from halo2_vectordb_amd.rounds import ProverRounds
    sizes = (3, 1, 5)
    index, hp = _hot_path(O, sizes, k=12)
    pr = mh = None
    try:
        pr = ProverRounds(hp.setup()).keygen()
        assert pr.keygen_report.violations() == 0, pr.keygen_report.as_dict()
        out = pr.prove(None, seed=31)
        droot, iroot = hp.results()
        assert np.array_equal(iroot, index.roots()[-1])
        want = TM.to_ints(np.stack([droot, iroot]))
        assert out["instances"] == want
        vk = verifier.VerifyingKey.from_prover(pr, out["opened"])
        assert verifier.verify(out["proof"], want, vk)
        for i in range(2):
            wrong = list(want)
            wrong[i] = (wrong[i] + 1) % O.R_MOD
            assert not verifier.verify(out["proof"], wrong, vk), i
        # the root MerkleHotPath publishes over the same rows (the index quantizes at its own P)
        mh = MerkleHotPath(n=sum(sizes), dim=DIM, k=12, P=P, tau=TAU, vectors=database_f64(sizes)[0])
        mh.setup()
        mh._witness()
        api.sync()
        assert np.array_equal(mh.results(), droot)
    finally:
        for x in (pr, mh, hp, index):
            if x is not None:
                x.free()


# ---------------------------------------------------------------------------------------------------------------- the chain
def test_along_build_updated_removed_every_cover_is_clean_with_the_published_roots(api, O):
    from halo2_vectordb_amd.pipeline import AnnCoverHotPath, AnnDeleteHotPath, AnnUpdateHotPath
    from halo2_vectordb_amd.rounds import ProverRounds
    sizes = (3, 1, 5)
    made = [_index(O, sizes)]

    def covered(ix, index_root):
        hp = AnnCoverHotPath(ix, k=12, L=L, tau=TAU)
        made.append(hp)
        pr = ProverRounds(hp.setup()).keygen()
        made.append(pr)
        assert pr.keygen_report.violations() == 0, pr.keygen_report.as_dict()
        droot, iroot = hp.results()
        assert np.array_equal(iroot, index_root) and np.array_equal(iroot, ix.roots()[-1])
        assert np.array_equal(droot, api.poseidon_merkle_root(ix.qvec))
        return droot
    try:
        ix = made[0]
        d0 = covered(ix, ix.roots()[-1])
        c = 2
        rows = np.asarray([[200.0, 3.0, 150.0], [7.0, -8.0, 9.0]])
        au = AnnUpdateHotPath(ix, c, ([1, sizes[c]], rows), grow=None, k=13, tau=TAU).setup()        # one replace, one append
        made.append(au)
        au._witness()
        api.sync()
        ix2 = ix.updated(au)
        made.append(ix2)
        d1 = covered(ix2, au.results()[5])
        assert not np.array_equal(d1, d0) and ix2.n == ix.n + 1
        ad = AnnDeleteHotPath(ix2, 0, [1], k=13, tau=TAU).setup()                                    # one delete
        made.append(ad)
        ad._witness()
        api.sync()
        ix3 = ix2.removed(ad)
        made.append(ix3)
        d2 = covered(ix3, ad.results()[-1])
        assert not np.array_equal(d2, d1) and ix3.n == ix.n
    finally:
        for x in reversed(made):
            x.free()


def test_single_cell_alteration_sweep_finds_no_free_cell(api, O, monkeypatch):
    """tests/alteration_model.py's method by the device sweep of tests/test_gpu_alteration.py at sizes (1, 2): the map as the device
    placed it and the bytes the kernels wrote; there is no is_zero in the circuit, so no cell may stay free"""
    from test_gpu_alteration import device_sweep
    found, unnoticed = [], AM.unnoticed

    def recording(*a, **kw):
        found.append(unnoticed(*a, **kw))
        return found[-1]
    monkeypatch.setattr(AM, "unnoticed", recording)
    index, hp = _hot_path(O, (1, 2), k=12)
    try:
        device_sweep(api, O, "ann cover sizes (1, 2)", hp.setup())                 # frees the hot path
    finally:
        index.free()
    assert found == [[]], found
