"""The means of a resident index and the mean audit of one cluster on the GPU (AnnIndex.means / recentred, vdb_ann_cluster_means*;
pipeline.AnnMeanHotPath, vdb_wit_ann_mean*): the values are tests/ann_mean_model.py's bit for bit at every cluster size and width the
kernel walks differently; the streams are the model's bit for bit (tests/test_ann_mean_cpu.py holds that model against the host-built
map first); host and device forms, the launch lists, refused arguments, rank windows, the device-placed map, the proof, a centroid that
is not the mean, an update followed by a recentre, a k-means handed to the index, and the alteration sweep."""
import ctypes

import numpy as np
import pytest

import ann_mean_model as MM
import topk_model as TM
from test_ann_mean_cpu import L, P, case, index_of
from test_gpu_batch_query import _dev
from test_gpu_rounds import TAU
from test_gpu_sweep import _check_window, _windowed

pytestmark = pytest.mark.gpu

# K, dim, the cluster sizes: {1, 2, 3, 7, 63, 64, 65, 130} all occur; dim covers a partial wavefront, exactly one, one and a lane, three
VALUE_CASES = [(1, 1, [1]), (2, 3, [2, 63]), (5, 64, [3, 7, 64, 65, 130]), (5, 65, [1, 2, 3, 7, 63]), (2, 130, [65, 130]), (1, 130, [64])]
WITNESS_CASES = [(1, 1, 1, 0), (2, 2, 3, 1), (3, 65, 2, 0), (5, 70, 65, 4)]      # K, n_c, dim, c
_values = {}


@pytest.fixture(scope="module")
def api():
    from halo2_vectordb_amd import api as a
    a.init(0)
    return a


def value_case(O, K, dim, sizes):
    """-> (f64 rows on a signed grid, cluster ids, the model's means), computed once per case and shared; nothing changes it"""
    key = (K, dim, tuple(sizes))
    if key not in _values:
        rng = np.random.default_rng(1000 * K + dim)
        n = sum(sizes)
        rows = rng.integers(-109, 110, (n, dim)).astype(np.float64)
        ids = rng.permutation(np.repeat(np.arange(K), sizes))
        q = O.quantize(rows, P)
        _values[key] = (rows, ids, np.stack([MM.means(O, q[ids == k], P, L) for k in range(K)]))
    return _values[key]


def _value_index(O, K, dim, sizes):
    from halo2_vectordb_amd.pipeline import AnnIndex
    rows, ids, want = value_case(O, K, dim, sizes)
    return AnnIndex(rows.shape[0], dim, K, rows, ids, np.zeros((K, dim)), P=P, L=L), rows, ids, want


@pytest.mark.parametrize("K,dim,sizes", VALUE_CASES)
def test_means_are_the_models_bit_for_bit_in_both_forms(api, O, K, dim, sizes):
    ix, rows, ids, want = _value_index(O, K, dim, sizes)
    try:
        assert ix.sizes.tolist() == sizes
        got = ix.means()
        assert got.shape == (K, dim, 4)
        bad = np.argwhere((got != want).any(axis=2))
        assert bad.size == 0, f"first differing (cluster, word) {bad[:5].tolist()}"
        grouped, offsets = ix.d_grouped.download((ix.n, dim, 4)), ix.d_offsets.download((K + 1,), dtype=np.uint64)
        assert offsets.tolist() == ix.offsets.tolist()
        assert np.array_equal(api.ann_cluster_means(grouped, offsets, P, L), want)
        assert TM.to_ints(want) == [v for k in range(K) for v in MM.means_int(grouped[int(offsets[k]):int(offsets[k + 1])], P)]
    finally:
        ix.free()


def test_signs_zero_sums_and_inexact_quotients(api, O):
    """one word per cluster: sums that are negative, zero and positive, quotients that lose a fraction for both signs and under a count
    that is no power of two — where qdiv's sign handling and rounding can go wrong"""
    clusters = [[-5, 2, 1], [5, -2, -2], [7, -7], [100, 1, 1, 1, 1, 1, 1], [-100, -1, -1, -1, -1, -1, -1], [-3], [1, 1, -1, -1, 3], [-1, -1, 1, 1, -3]]
    grouped = O.quantize(np.asarray([[v] for c in clusters for v in c], dtype=np.float64), P)
    offsets = np.concatenate([[0], np.cumsum([len(c) for c in clusters])]).astype(np.uint64)
    got = TM.to_ints(api.ann_cluster_means(grouped, offsets, P, L))
    want = []
    for c in clusters:
        q = (abs(sum(c)) << P) // len(c)
        want.append((MM.R - q) % MM.R if sum(c) < 0 else q)
    assert got == want
    assert got == TM.to_ints(MM.index_means(O, grouped, offsets, P, L))
    assert got[2] == 0 and got[0] > MM.R // 2 and 0 < got[1] < MM.R // 2
    assert (abs(sum(clusters[0])) << P) % 3 and (100 + 6 << P) % 7                # the fractions are really lost


def test_means_take_one_launch_at_every_shape_and_refused_arguments_launch_nothing(api, O):
    from halo2_vectordb_amd._lib import check
    lib = api.init()
    counts = []
    for K, dim, sizes in (VALUE_CASES[0], VALUE_CASES[2]):
        ix = _value_index(O, K, dim, sizes)[0]
        try:
            ix.means()
            api.sync()
            api.profile_begin(deferred=True)
            ix.means()
            api.sync()
            counts.append({kern: int(v["launches"]) for kern, v in api.profile_end().items()})
        finally:
            ix.free()
    assert counts[0] == counts[1] == {"k_ann_means": 1}, counts
    K, dim, sizes = VALUE_CASES[1]
    ix = _value_index(O, K, dim, sizes)[0]
    up = []
    try:
        grouped = ix.d_grouped.download((ix.n, dim, 4))
        d_out = api.DeviceBuffer(K * dim * 32)
        up.append(d_out)
        check(lib.vdb_memset_dev(d_out.ptr, 0xA5, ctypes.c_size_t(K * dim * 32)))
        empty = _dev(api, up, np.asarray([0, 0, ix.n], dtype=np.uint64))          # an offset pair with n_k = 0
        falling = _dev(api, up, np.asarray([0, ix.n + 1, ix.n], dtype=np.uint64))
        short = _dev(api, up, np.asarray([0, 2, ix.n - 1], dtype=np.uint64))
        api.sync()
        api.profile_begin(deferred=True)
        dev = lambda off=ix.d_offsets, n=ix.n, K_=K, dim_=dim: lib.vdb_ann_cluster_means_dev(P, L, ix.d_grouped.ptr, off.ptr, n, K_, dim_, d_out.ptr)
        for kw in (dict(K_=0), dict(K_=4097), dict(dim_=0), dict(dim_=(1 << 20) + 1), dict(off=empty), dict(off=falling), dict(off=short), dict(n=ix.n - 1)):
            with pytest.raises(api.VdbError) as e:
                check(dev(**kw))
            assert e.value.code == -3, kw
        host = np.zeros((K, dim, 4), dtype=np.uint64)
        for off, K_, dim_ in (([0, 0, ix.n], K, dim), ([0, 2, ix.n], 0, dim), ([0, 2, ix.n], K, 0), ([0, 2, ix.n - 1], K, dim)):
            off = np.asarray(off, dtype=np.uint64)
            assert lib.vdb_ann_cluster_means(P, L, api._p(grouped), api._p(off), ix.n, K_, dim_, api._p(host)) == -3, (off, K_, dim_)
        api.sync()
        assert api.profile_end() == {}
        assert (d_out.download((K * dim * 32,), dtype=np.uint8) == 0xA5).all() and not host.any()
    finally:
        for b in up:
            b.free()
        ix.free()


# ---------------------------------------------------------------------------------------------------------------- the witness
def _index(O, K, n_c, dim, c, off_by=()):
    """the resident index of a case (test_ann_mean_cpu.index_of: centroid c the mean of the case's members, every other cluster one row,
    its own centroid); `off_by`: words of centroid c moved by one -> (AnnIndex, quantized centroids, members)"""
    from halo2_vectordb_amd.pipeline import AnnIndex
    cent, mem, _ = index_of(O, K, n_c, dim, c)
    cent = cent.copy()
    for j in off_by:
        cent[c, j] = O.fr_add(cent[c, j][None], O.fr_from_ints([1]))[0]
    rows = np.concatenate([mem if j == c else cent[j:j + 1] for j in range(K)])
    ids = np.concatenate([np.full(n_c if j == c else 1, j) for j in range(K)])
    return AnnIndex(rows.shape[0], dim, K, rows, ids, cent, P=P, L=L), cent, mem


def _hot_path(O, K, n_c, dim, c, k=13, off_by=(), **kw):
    from halo2_vectordb_amd.pipeline import AnnMeanHotPath
    index = _index(O, K, n_c, dim, c, off_by)[0]
    return index, AnnMeanHotPath(index, c, k=k, P=P, L=L, tau=TAU, **kw)


@pytest.mark.parametrize("K,n_c,dim,c", WITNESS_CASES)
def test_witness_is_the_models_resident_absent_and_from_host_arrays(api, O, K, n_c, dim, c):
    from halo2_vectordb_amd import circuit_sym as CS
    from halo2_vectordb_amd._lib import check
    m, cent, mem, roots, index_root = case(O, K, n_c, dim, c)
    host = api.wit_ann_mean(cent, mem, roots, c, P, L, selectors=True)
    assert host["n_in"] == m["n_in"] == K + 2 and host["stream"].shape == m["advice"].shape
    bad = np.flatnonzero((host["stream"] != m["advice"]).any(axis=1))
    assert bad.size == 0, f"first differing advice cells {bad[:5]} of {host['stream'].shape[0]} (blocks {m['regions']})"
    assert np.array_equal(host["lookup"], m["lookup"]) and np.array_equal(host["selectors"], m["selectors"])
    gen = m["generator"]                                     # the flag bytes beyond the gate bit: the model's outside the qdiv blocks
    assert np.array_equal(host["flags"][~gen], m["flags"][~gen])
    assert np.array_equal(host["mean_ok"], m["mean_ok"]) and host["mean_ok"].all()
    assert np.array_equal(host["public"], m["public"]) and np.array_equal(host["public"][0], index_root)
    lay = CS.ann_mean_layout(K, n_c, dim, P, L)              # ann_mean_layout is annm_blocks through vdb_wit_ann_mean_size
    cells, lk, n_in = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
    check(api.init().vdb_wit_ann_mean_size(P, L, K, n_c, dim, ctypes.byref(cells), ctypes.byref(lk), ctypes.byref(n_in)))
    assert (cells.value, lk.value, n_in.value) == (lay["total"], lay["total_l"], lay["n_in"])
    index, hp = _hot_path(O, K, n_c, dim, c)
    try:
        assert np.array_equal(index.roots()[:K + 1], roots) and np.array_equal(index.members(c), mem)
        assert np.array_equal(index.means()[c], cent[c])
        hp.setup()
        assert hp.resident and (hp.n_cells, hp.n_in, hp.n_lookup) == (m["advice"].shape[0], K + 2, m["lookup"].shape[0])
        d_flags = hp.keygen_flags()
        assert np.array_equal(d_flags.download((hp.n_cells,), dtype=np.uint8), host["flags"])
        d_flags.free()
        for resident in (True, False):
            check(hp.lib.vdb_memset_dev(hp.d_stream.ptr, 0xA5, ctypes.c_size_t(hp.n_cells * 32)))
            hp.resident = resident
            hp._witness()
            api.sync()
            assert np.array_equal(hp.d_stream.download((hp.n_cells, 4)), host["stream"]), resident
            assert np.array_equal(hp.d_lookup.download((hp.n_lookup, 4)), host["lookup"]), resident
            root, c_fr, ok = hp.results()
            assert np.array_equal(root, index_root) and TM.to_ints(c_fr[None]) == [c] and ok.tolist() == [1] * dim
    finally:
        hp.free()
        index.free()


def test_launch_list_depends_on_neither_K_nor_the_cluster_size_and_refused_arguments_launch_nothing(api, O):
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
            api.sync()
            api.profile_begin(deferred=True)

            def call(K_=K, c_=c, n_c_=n_c, dim_=dim, lc=None, lm=None, P_=P, L_=L):
                return lib.vdb_wit_ann_mean_dev(P_, L_, hp.p_cent, hp.p_members, index.d_roots.ptr, lc, lm, K_, c_, n_c_, dim_, d_out.ptr, d_out.at(1 << 14),
                                                None, d_out.at(1 << 15), d_out.at(3 << 14))
            big = 1 << 24
            # the frame's refusals, the mean audit's own, the instance limits, the cell limit (a circuit whose instance counts pass: held
            # against the layout first), one resident tree without the other
            huge = dict(n_c_=1 << 16, dim_=256, K_=1 << 12)
            lay = CS.ann_mean_layout(huge["K_"], huge["n_c_"], huge["dim_"], P, L)
            assert lay["total"] > 1 << 34 and huge["n_c_"] * huge["dim_"] <= big and huge["K_"] * huge["dim_"] <= big
            sized = [dict(K_=0), dict(K_=4097), dict(n_c_=big + 1), dict(n_c_=0), dict(dim_=0), dict(dim_=(1 << 20) + 1), dict(n_c_=big // dim + 1),
                     dict(K_=4096, dim_=big // 4096 + 1), huge]
            for kw in sized:                                        # the size call first: it shares the layout and writes nothing
                cells = ctypes.c_uint64()
                assert lib.vdb_wit_ann_mean_size(P, L, kw.get("K_", K), kw.get("n_c_", n_c), kw.get("dim_", dim), ctypes.byref(cells), None, None) == -3, kw
            for kw in sized + [dict(c_=K), dict(lc=index.levels_ptr(K)), dict(lm=index.levels_ptr(c))]:
                with pytest.raises(api.VdbError) as e:
                    check(call(**kw))
                assert e.value.code == -3, kw
            api.sync()
            assert api.profile_end() == {}
            assert (d_out.download((1 << 16,), dtype=np.uint8) == 0xA5).all()
            d_out.free()
        finally:
            hp.free()
            index.free()
    assert counts[2] == counts[5], counts
    got = counts[2]
    assert got["k_annm_sum"] == 1 and got["k_annm_div"] == 1 and got["k_nv_select"] == 2 and got["k_inv_fixup"] == 1, counts
    assert got["k_push_cells"] == 3, counts                  # the constant len, and each tree's zero cell (launched without padding too)
    assert got["k_mk_leaf_trace"] == 3 and got["k_mk_tree_trace"] == 2 and got["k_mku_inputs"] == 1, counts
    assert "k_annu_new_roots" not in got and "k_nv_qmin" not in got and "k_anna_pick" not in got, counts


def test_divisor_bound_holds_at_every_size_the_library_takes(api, O):
    """quantization(n_c) = n_c 2^P must stay below the 2^(2P) qdiv asserts for its divisor, n_c < 2^P (circuit_sym.ann_mean_layout refuses
    beyond it: tests/test_ann_mean_cpu.py).  The library takes P >= 32 and n_c <= VDB_ANN_MAX_VECTORS = 2^24, so its own refusal of
    n_c >= 2^P lies behind those two: every cluster it sizes passes the bound at the smallest P"""
    lib = api.init()
    cells = ctypes.c_uint64()
    assert lib.vdb_wit_ann_mean_size(31, L, 1, 1, 1, ctypes.byref(cells), None, None) == -3
    assert lib.vdb_wit_ann_mean_size(32, L, 1, (1 << 24) + 1, 1, ctypes.byref(cells), None, None) == -3
    assert lib.vdb_wit_ann_mean_size(32, L, 1, 3, 1, ctypes.byref(cells), None, None) == 0 and cells.value > 0


def test_windowed_calls_write_the_bytes_of_one(api, O):
    from halo2_vectordb_amd._lib import check
    lib = api.init()
    K, n_c, dim, c = 2, 2, 3, 1
    m, cent, mem, roots, _ = case(O, K, n_c, dim, c)
    want, lk, r = m["advice"], m["lookup"], m["regions"]
    cells, q_n, q_lk = want.shape[0], m["qdiv_cells"], m["qdiv_lk"]
    up = []
    try:
        d_cent, d_mem, d_roots = _dev(api, up, cent), _dev(api, up, mem), _dev(api, up, roots)
        d_ok, d_pub = api.DeviceBuffer(32), api.DeviceBuffer(64)
        up += [d_ok, d_pub]
        run = lambda d_adv, d_lkb: check(lib.vdb_wit_ann_mean_dev(P, L, d_cent.ptr, d_mem.ptr, d_roots.ptr, None, None, K, c, n_c, dim, d_adv.ptr, d_lkb.ptr, None,
                                                                 d_ok.ptr, d_pub.ptr))
        # inside the header; inside an indicator; inside the assigned members; inside a selection of S; on the constant; inside a qadd of
        # the chain; between the first and the second quotient (the lookup cut between their runs); inside MC
        cuts = [(2, 0), (r["indicator"] + 8 + 5, 0), (r["members"] + 3, 0), (r["own"] + 5, 0), (r["len"], 0), (r["len"] + 1, 0), (r["chain"] + 6, 0),
                (r["div"] + q_n, q_lk), (r["div"] + 2 * q_n, 2 * q_lk), (r["merkle_c"] + 1000, len(lk))]
        splits = [[x] for x in cuts] + [[cuts[3], cuts[7]], [cuts[6], cuts[8]]]          # two windows each, then three
        # the seams of the cluster frame the audits share: where the head ends, between the centroids and the members (inside the one
        # launch that assigns both), where MC and MM start, one cell into MM
        splits += [[x] for x in ((r["centroids"], 0), (r["members"], 0), (r["merkle_c"], len(lk)), (r["merkle_m"], len(lk)), (r["merkle_m"] + 1, len(lk)))]
        for split in splits:
            edges = [(0, 0)] + split + [(cells, len(lk))]
            parts = []
            for (lo, llo), (hi, lhi) in zip(edges[:-1], edges[1:]):
                window = (lo, hi, llo, lhi)
                g_adv, g_lk = _windowed(api, lib, check, want, lk, window, run)
                _check_window(want, lk, g_adv, g_lk, window, (split, window))
                assert np.array_equal(d_pub.download((2, 4)), m["public"]), (split, window)
                assert d_ok.download((dim,), dtype=np.uint8).tolist() == [1] * dim, (split, window)
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
    m, cent, mem, roots, _ = case(O, K, n_c, dim, c)
    got = api.wit_ann_mean(cent, mem, roots, c, P, L, selectors=True)
    ff, fv, vals = fetchers(dict(advice=got["stream"], flags=got["flags"]))
    cm, public, info = CS.build_ann_mean(K, n_c, dim, P, L, ff, fv)
    rep = cm.check_witness(vals, TM.to_ints(got["lookup"]), got["flags"])
    assert not any(rep.values()), rep
    assert [vals[x] for x in public] == TM.to_ints(got["public"])
    assert [int(cm.copy_of[x]) for x in info["mean"]] == info["own"] and cm.copy_of[info["members_root"]] == info["picked"]


@pytest.mark.parametrize("K,n_c,dim,c", [(1, 1, 1, 0), (2, 2, 3, 1), (3, 5, 2, 0)])
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
        assert d[6] == h[6] and len(h[6]) == 2
        for i in (0, 2, 4, 5):
            assert np.array_equal(d[i], h[i]), i
        val = lambda x: np.where(x[1] >= 0, np.asarray(x[3] + [0], dtype=object)[np.maximum(x[1], -1)], -1)
        assert np.array_equal(val(d), val(h))
    finally:
        hp.free()
        index.free()


# ---------------------------------------------------------------------------------------------------------------- the proof
def test_proof_is_accepted_and_bound_to_the_index_root_and_the_cluster(api, O):
    from halo2_vectordb_amd import verifier
    from halo2_vectordb_amd.rounds import ProverRounds
    K, n_c, dim, c = 2, 3, 4, 1
    index, hp = _hot_path(O, K, n_c, dim, c, k=13)             # the smallest k that holds the 2^12-entry table
    pr = None
    try:
        pr = ProverRounds(hp.setup()).keygen()
        assert pr.keygen_report.violations() == 0, pr.keygen_report.as_dict()
        out = pr.prove(None, seed=29)
        want = [TM.to_ints(index.roots()[-1][None])[0], c]
        assert out["instances"] == want
        assert hp.results()[2].tolist() == [1] * dim
        vk = verifier.VerifyingKey.from_prover(pr, out["opened"])
        assert verifier.verify(out["proof"], want, vk)
        for i in range(2):
            wrong = list(want)
            wrong[i] = (wrong[i] + 1) % O.R_MOD
            assert not verifier.verify(out["proof"], wrong, vk), i
    finally:
        if pr is not None:
            pr.free()
        hp.free()
        index.free()


def test_a_centroid_off_the_mean_in_two_words_is_flagged_and_fails_the_mock_report(api, O):
    """a failing Mock report, not a fault: the call succeeds on an index whose centroid c is not the mean in words 1 and 3"""
    from halo2_vectordb_amd import circuit_sym as CS
    from halo2_vectordb_amd.rounds import ProverRounds
    K, n_c, dim, c = 2, 3, 4, 1
    index, hp = _hot_path(O, K, n_c, dim, c, off_by=(1, 3))
    pr = None
    try:
        pr = ProverRounds(hp.setup()).keygen()
        assert hp.results()[2].tolist() == [1, 0, 1, 0]
        rep = pr.keygen_report
        lay = CS.ann_mean_layout(K, n_c, dim, P, L)
        mean_1 = lay["div"] + 2 * lay["units"]["qd"].n - 1
        assert rep.violations() == 2 and rep.copies_unequal == 2 and rep.first_copy == mean_1, rep.as_dict()
    finally:
        if pr is not None:
            pr.free()
        hp.free()
        index.free()


def test_an_update_breaks_the_mean_and_a_recentred_index_restores_it(api, O):
    from halo2_vectordb_amd import verifier
    from halo2_vectordb_amd.pipeline import AnnMeanHotPath, AnnUpdateHotPath
    from halo2_vectordb_amd.rounds import ProverRounds
    K, n_c, dim, c = 2, 3, 4, 1
    index, cent, mem = _index(O, K, n_c, dim, c)
    made, pr = [index], None
    try:
        row = np.asarray([200.0, 3.0, 150.0, 77.0])
        au = AnnUpdateHotPath(index, c, ([n_c], row[None]), grow=None, k=13, tau=TAU).setup()
        made.append(au)
        au._witness()
        api.sync()
        ix2 = index.updated(au)
        made.append(ix2)
        hp = AnnMeanHotPath(ix2, c, k=13, P=P, L=L, tau=TAU).setup()
        made.append(hp)
        assert hp.n == n_c + 1
        pr = ProverRounds(hp).keygen()
        ok = hp.results()[2]
        assert not ok.all() and pr.keygen_report.violations() == pr.keygen_report.copies_unequal == int((ok == 0).sum())
        pr.free()
        pr = None
        ix3 = ix2.recentred()
        made.append(ix3)
        want = np.stack([MM.means(O, ix2.members(j), P, L) for j in range(K)])
        assert np.array_equal(ix3.qcent, want) and np.array_equal(ix3.means(), want)
        assert np.array_equal(ix3.members(c), ix2.members(c)) and not np.array_equal(ix3.roots()[-1], ix2.roots()[-1])
        hp3 = AnnMeanHotPath(ix3, c, k=13, P=P, L=L, tau=TAU).setup()
        made.append(hp3)
        pr = ProverRounds(hp3).keygen()
        assert pr.keygen_report.violations() == 0, pr.keygen_report.as_dict()
        root, c_fr, ok = hp3.results()
        assert np.array_equal(root, ix3.roots()[-1]) and ok.tolist() == [1] * dim
        out = pr.prove(None, seed=31)
        assert out["instances"] == TM.to_ints(np.stack([root, c_fr]))
        assert verifier.verify(out["proof"], out["instances"], verifier.VerifyingKey.from_prover(pr, out["opened"]))
    finally:
        if pr is not None:
            pr.free()
        for x in reversed(made):
            x.free()


def test_a_kmeans_handed_to_the_index_is_a_fixed_point_of_the_mean_audit(api, O):
    """values alone (the first K rows start as their own centroids, whose zero distance Euclidean cannot prove): the centroids k-means
    ends on are the means of the clusters its final indicators name, bit for bit, and both clusters pass the mean audit"""
    from halo2_vectordb_amd.pipeline import AnnIndex, AnnMeanHotPath
    n, dim, K = 16, 4, 2
    rows = np.random.default_rng(21).integers(0, 219, (n, dim)).astype(np.float64)
    km = api.wit_kmeans("manhattan", O.quantize(rows, P), K, 2, P, L)
    ix = AnnIndex(n, dim, K, rows, km["indicators"], km["centroids"], P=P, L=L)
    made = [ix]
    try:
        assert ix.sizes.min() >= 1 and ix.sizes.max() >= 3
        assert np.array_equal(ix.means(), km["centroids"])
        for c in range(K):
            hp = AnnMeanHotPath(ix, c, k=13, P=P, L=L, tau=TAU).setup()
            made.append(hp)
            hp._witness()
            api.sync()
            root, _, ok = hp.results()
            assert ok.tolist() == [1] * dim and np.array_equal(root, ix.roots()[-1])
    finally:
        for x in reversed(made):
            x.free()


def test_single_cell_alteration_sweep(api, O):
    """tests/alteration_model.py's method by the device sweep of tests/test_gpu_alteration.py at (K 2, n_c 2, dim 3, c 1): the map as the
    device placed it and the bytes the kernels wrote; a cell may stay free only by a rule of alteration_model.explain"""
    from test_gpu_alteration import device_sweep
    index, hp = _hot_path(O, 2, 2, 3, 1)
    try:
        device_sweep(api, O, "ann mean K 2 n_c 2 c 1 dim 3", hp.setup())       # frees the hot path
    finally:
        index.free()
