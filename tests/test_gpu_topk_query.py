"""Top-k queries against one committed database in one proof (pipeline.TopKQueryHotPath; vdb_wit_nearest_topk*) on the GPU.  The
streams are tests/topk_model.py's, bit for bit — advice, lookup, gate-start flags, break points, indicators, results, public values,
root (tests/test_topk_cpu.py holds that model against the oracle first); t = 1 writes the batch entry point's bytes and, with q = 1,
the query circuit's key and proof; the launch count depends on neither q nor t; rank windows, limits, the whole proof, the second
prover, two sharded ranks and single altered cells of the new regions."""
import ctypes

import numpy as np
import pytest

import topk_model as TM
from test_gpu_batch_query import _dev
from test_gpu_rounds import FIXED, TAU, _meta, _verify
from test_gpu_sharded import _run
from test_gpu_sweep import _check_window, _windowed
from test_topk_cpu import f64_distances, separated_inputs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def api():
    from halo2_vectordb_amd import api as a
    a.init(0)
    return a


def _model(O, hp, metric, P, L, k):
    qv = hp.qvec
    return TM.topk_model(O, metric, qv[:hp.q], qv[hp.q:], hp.topk, P, L, plan_k=k, merkle=True)


def _stream_parity(api, O, hp, metric, P, L, k):
    """the whole circuit's streams against the model; -> the indicator bits (q, t, n)"""
    try:
        d_flags = hp.keygen_flags()
        flags = d_flags.download((hp.n_cells,), dtype=np.uint8)
        d_flags.free()
        hp._witness()
        api.sync()
        m = _model(O, hp, metric, P, L, k)
        assert m["advice"].shape[0] == hp.n_cells == hp.n_in + hp.nearest_cells + hp.merkle_cells and m["lookup"].shape[0] == hp.n_lookup
        got = hp.d_stream.download((hp.n_cells, 4))
        bad = np.flatnonzero((got != m["advice"]).any(axis=1))
        assert bad.size == 0, f"first differing advice cells {bad[:5]} of {hp.n_cells}"
        assert np.array_equal(hp.d_lookup.download((hp.n_lookup, 4)), m["lookup"])
        assert np.array_equal(flags & 1, m["selectors"])
        assert np.array_equal(hp.bp, m["break_points"])
        g_ind, g_res, g_root = hp.results()
        assert np.array_equal(g_ind, m["indicators"]) and np.array_equal(g_res, m["results"]) and np.array_equal(g_root, m["root"])
        ptr, count = hp.public_values_dev()
        assert count == hp.q * hp.topk * hp.dim + 1
        pub = hp.d_pub.download((count, 4))
        assert np.array_equal(pub[:-1], m["results"].reshape(-1, 4)) and np.array_equal(pub[-1], m["root"])
        return m["indicator_bits"]
    finally:
        hp.free()


@pytest.mark.parametrize("metric,q,n,dim", [("cosine", 3, 6, 4), ("euclidean", 3, 5, 4)])
def test_small_streams_are_the_models_and_name_the_f64_neighbours(api, O, metric, q, n, dim):
    from halo2_vectordb_amd.pipeline import TopKQueryHotPath
    v = separated_inputs(metric, q, n, dim, 3, seed=q * 10 + n)
    hp = TopKQueryHotPath(topk=3, q=q, n=n, dim=dim, k=12, L=11, metric=metric, tau=TAU, vectors=v).setup()
    bits = _stream_parity(api, O, hp, metric, 48, 11, 12)
    d = f64_distances(metric, v, q)
    for i in range(q):
        order = np.argsort(d[i], kind="stable")
        assert [list(b) for b in bits[i]] == [[int(j == order[r]) for j in range(n)] for r in range(3)], i


def test_tie_inside_the_top_t(api, O):
    """Hamming: two rows at the smallest distance — both indicators in round 0, the result the last of them, both gone in round 1"""
    from halo2_vectordb_amd.pipeline import TopKQueryHotPath
    v = np.asarray([[0, 0, 0, 0], [0, 0, 0, 1], [1, 1, 1, 1], [1, 0, 0, 0], [1, 1, 0, 0], [0, 1, 1, 1]], dtype=np.float64)
    hp = TopKQueryHotPath(topk=3, q=1, n=5, dim=4, k=12, L=11, metric="hamming", tau=TAU, vectors=v).setup()
    bits = _stream_parity(api, O, hp, "hamming", 48, 11, 12)
    assert bits[0].tolist() == [[1, 0, 1, 0, 0], [0, 0, 0, 1, 0], [0, 0, 0, 0, 1]]


def test_fewer_distinct_distances_than_rounds(api, O):
    from halo2_vectordb_amd.pipeline import TopKQueryHotPath
    v = np.asarray([[0, 0, 0, 0], [0, 0, 0, 1], [1, 1, 1, 1], [1, 0, 0, 0]], dtype=np.float64)
    hp = TopKQueryHotPath(topk=3, q=1, n=3, dim=4, k=12, L=11, metric="hamming", tau=TAU, vectors=v).setup()
    bits = _stream_parity(api, O, hp, "hamming", 48, 11, 12)
    assert bits[0].tolist() == [[1, 0, 1], [0, 1, 0], [1, 1, 1]]


def test_database_of_one_vector(api, O):
    from halo2_vectordb_amd.pipeline import TopKQueryHotPath
    hp = TopKQueryHotPath(topk=1, q=2, n=1, dim=4, k=12, L=11, metric="euclidean", tau=TAU).setup()
    bits = _stream_parity(api, O, hp, "euclidean", 48, 11, 12)
    assert bits.reshape(-1).tolist() == [1, 1]


def test_as_many_rounds_as_vectors(api, O):
    from halo2_vectordb_amd.pipeline import TopKQueryHotPath
    v = separated_inputs("euclidean", 2, 5, 3, 5, seed=55)
    hp = TopKQueryHotPath(topk=5, q=2, n=5, dim=3, k=12, L=11, metric="euclidean", tau=TAU, vectors=v).setup()
    bits = _stream_parity(api, O, hp, "euclidean", 48, 11, 12)
    assert (bits.sum(axis=1) == 1).all() and (bits.sum(axis=2) == 1).all()        # every vector once, a permutation per query


def test_tiled_scan_and_more_queries_than_lanes(api, O):
    """Manhattan, q = 70, n = 130, t = 5: three scan tiles per round, more queries than a wavefront has lanes"""
    from halo2_vectordb_amd.pipeline import TopKQueryHotPath
    rng = np.random.default_rng(130)
    v = rng.uniform(-2.5, 2.5, size=(70 + 130, 2))
    hp = TopKQueryHotPath(topk=5, q=70, n=130, dim=2, k=14, L=13, metric="manhattan", tau=TAU, vectors=v).setup()
    _stream_parity(api, O, hp, "manhattan", 48, 13, 14)


def _dev_call(api, metric, queries, db, topk, P, L, batch=False):
    """vdb_wit_nearest_topk_dev (or the batch entry point) into poisoned buffers -> (stream, lookup, flags, indicators, results)"""
    from halo2_vectordb_amd._lib import check
    lib = api.init()
    q, n, dim = queries.shape[0], db.shape[0], db.shape[1]
    cells, lk = ctypes.c_uint64(), ctypes.c_uint64()
    check(lib.vdb_wit_nearest_topk_size(api.METRICS[metric], P, L, q, n, dim, topk, ctypes.byref(cells), ctypes.byref(lk)))
    cells, lk = cells.value, lk.value
    up = []
    try:
        d_q, d_db = _dev(api, up, queries), _dev(api, up, db)
        d_adv, d_lk, d_sel = api.DeviceBuffer(cells * 32), api.DeviceBuffer(max(lk, 1) * 32), api.DeviceBuffer(cells)
        d_ind, d_res = api.DeviceBuffer(q * topk * n * 32), api.DeviceBuffer(q * topk * dim * 32)
        up += [d_adv, d_lk, d_sel, d_ind, d_res]
        check(lib.vdb_memset_dev(d_adv.ptr, 0xA5, ctypes.c_size_t(cells * 32)))
        check(lib.vdb_memset_dev(d_lk.ptr, 0xA5, ctypes.c_size_t(max(lk, 1) * 32)))
        check(lib.vdb_memset_dev(d_sel.ptr, 0, ctypes.c_size_t(cells)))
        if batch:
            assert topk == 1
            check(lib.vdb_wit_nearest_batch_dev(api.METRICS[metric], P, L, d_q.ptr, d_db.ptr, q, n, dim, d_adv.ptr, d_lk.ptr, d_sel.ptr, d_ind.ptr, d_res.ptr))
        else:
            check(lib.vdb_wit_nearest_topk_dev(api.METRICS[metric], P, L, d_q.ptr, d_db.ptr, q, n, dim, topk, d_adv.ptr, d_lk.ptr, d_sel.ptr, d_ind.ptr,
                                               d_res.ptr))
        api.sync()
        return (d_adv.download((cells, 4)), d_lk.download((max(lk, 1), 4))[:lk], d_sel.download((cells,), dtype=np.uint8),
                d_ind.download((q, topk, n, 4)), d_res.download((q, topk, dim, 4)))
    finally:
        for b in up:
            b.free()


@pytest.mark.parametrize("metric,q,n,dim,L", [("euclidean", 3, 5, 4, 11), ("cosine", 5, 9, 3, 12), ("manhattan", 66, 70, 2, 10), ("hamming", 4, 17, 6, 9),
                                              ("manhattan", 2, 1, 3, 11)])
def test_one_round_writes_the_bytes_of_the_batch_entry_point(api, O, metric, q, n, dim, L):
    rng = np.random.default_rng(q * 1000 + n * 10 + dim)
    v = rng.integers(0, 3, size=(q + n, dim)).astype(np.float64) * 0.5 if metric == "hamming" else rng.uniform(0.25, 3.0, size=(q + n, dim))
    qv = O.quantize(v, 48)
    got, want = _dev_call(api, metric, qv[:q], qv[q:], 1, 48, L), _dev_call(api, metric, qv[:q], qv[q:], 1, 48, L, batch=True)
    for name, a, b in zip(("stream", "lookup", "flags", "indicators", "results"), got, want):
        assert np.array_equal(a, b), name


@pytest.mark.parametrize("metric,q,n,dim,topk,L", [("euclidean", 3, 5, 4, 2, 11), ("hamming", 2, 9, 6, 4, 9), ("manhattan", 3, 70, 2, 3, 10)])
def test_host_entry_point_and_device_entry_point_write_the_models_streams(api, O, metric, q, n, dim, topk, L):
    rng = np.random.default_rng(q * 1000 + n * 10 + dim)
    v = rng.integers(0, 3, size=(q + n, dim)).astype(np.float64) * 0.5 if metric == "hamming" else rng.uniform(0.25, 3.0, size=(q + n, dim))
    qv = O.quantize(v, 48)
    m = TM.topk_model(O, metric, qv[:q], qv[q:], topk, 48, L, inputs=False)
    got = _dev_call(api, metric, qv[:q], qv[q:], topk, 48, L)
    host = api.wit_nearest_topk(metric, qv[:q], qv[q:], topk, P=48, L=L, selectors=True)
    for name, a, b, c in zip(("stream", "lookup", "flags", "indicators", "results"), got,
                             (m["advice"], m["lookup"], m["selectors"], m["indicators"], m["results"]),
                             (host["stream"], host["lookup"], host["flags"], host["indicators"], host["results"])):
        if name == "flags":
            assert np.array_equal(a & 1, b) and np.array_equal(a, c), name
        else:
            assert np.array_equal(a, b) and np.array_equal(a, c), name


def test_rounds_follow_the_serial_fold_on_values_no_order_holds_for(api, O):
    """full-width field elements as vectors: is_neg(m - x) is no order over such 'distances', every round's chain is whatever the
    serial fold makes of the entries the earlier rounds left, and the model folds serially"""
    rng = np.random.default_rng(99)
    q, n, dim, topk = 3, 150, 2, 3
    raw = O.random_fr(rng, (q + n) * dim).reshape(q + n, dim, 4)
    c = O.Ctx(store=True)
    c.nearest_vector("manhattan", raw[0], raw[q:], P=48, L=11)
    if c.err:
        pytest.fail("the oracle refuses these inputs; the model cannot be built")
    m = TM.topk_model(O, "manhattan", raw[:q], raw[q:], topk, 48, 11, inputs=False)
    got = _dev_call(api, "manhattan", raw[:q], raw[q:], topk, 48, 11)
    for name, a, b in zip(("stream", "lookup", "flags", "indicators", "results"), got,
                          (m["advice"], m["lookup"], m["selectors"], m["indicators"], m["results"])):
        assert np.array_equal(a & 1 if name == "flags" else a, b), name


def test_arguments_and_limits_are_refused_and_nothing_is_written(api, O):
    from halo2_vectordb_amd._lib import check
    lib = api.init()
    cells, lk = ctypes.c_uint64(), ctypes.c_uint64()
    for q, n, dim, topk in ((0, 4, 4, 1), (4, 0, 4, 1), (2, 4, 4, 0), (2, 4, 4, 5), ((1 << 24) + 1, 1, 1, 1), (1 << 12, 1 << 8, 1, 1 << 5),
                            (1 << 10, 16, 1 << 12, 8), (1 << 20, 16, 64, 1)):
        with pytest.raises(api.VdbError) as e:
            check(lib.vdb_wit_nearest_topk_size(0, 48, 11, q, n, dim, topk, ctypes.byref(cells), ctypes.byref(lk)))
        assert e.value.code == -3, (q, n, dim, topk)                      # VDB_ERR_ARG
    qv = O.quantize(np.random.default_rng(1).uniform(0.25, 3.0, size=(2 + 4, 3)), 48)
    up = []
    try:
        d_q, d_db = _dev(api, up, qv[:2]), _dev(api, up, qv[2:])
        d_out = api.DeviceBuffer(1 << 16)
        up.append(d_out)
        check(lib.vdb_memset_dev(d_out.ptr, 0xA5, ctypes.c_size_t(1 << 16)))
        for topk in (0, 5):
            with pytest.raises(api.VdbError) as e:
                check(lib.vdb_wit_nearest_topk_dev(0, 48, 11, d_q.ptr, d_db.ptr, 2, 4, 3, topk, d_out.ptr, d_out.at(1 << 15), None, d_out.at(1 << 14),
                                                   d_out.at(1 << 13)))
            assert e.value.code == -3
        api.sync()
        assert (d_out.download((1 << 16,), dtype=np.uint8) == 0xA5).all()
    finally:
        for b in up:
            b.free()


def test_launch_count_depends_on_neither_queries_nor_rounds(api, O):
    """the top-k entry point over (q, t), and the single-query and batch entry points, which are the same path at t = 1"""
    from halo2_vectordb_amd._lib import check
    lib = api.init()
    rng = np.random.default_rng(3)
    n, dim = 64, 8
    counts = {}
    for entry, q, topk in (("topk", 1, 1), ("topk", 1, 10), ("topk", 8, 10), ("topk", 1, 64), ("single", 1, 1), ("batch", 8, 1)):
        qv = O.quantize(rng.uniform(0.25, 3.0, size=(q + n, dim)), 48)
        cells, lk = ctypes.c_uint64(), ctypes.c_uint64()
        check(lib.vdb_wit_nearest_topk_size(0, 48, 13, q, n, dim, topk, ctypes.byref(cells), ctypes.byref(lk)))
        up = []
        try:
            d_q, d_db = _dev(api, up, qv[:q]), _dev(api, up, qv[q:])
            bufs = [api.DeviceBuffer(x) for x in (cells.value * 32, lk.value * 32, q * topk * n * 32, q * topk * dim * 32)]
            up += bufs
            out = (bufs[0].ptr, bufs[1].ptr, None, bufs[2].ptr, bufs[3].ptr)
            run = dict(topk=lambda: check(lib.vdb_wit_nearest_topk_dev(0, 48, 13, d_q.ptr, d_db.ptr, q, n, dim, topk, *out)),
                       single=lambda: check(lib.vdb_wit_nearest_dev(0, 48, 13, d_q.ptr, d_db.ptr, n, dim, *out)),
                       batch=lambda: check(lib.vdb_wit_nearest_batch_dev(0, 48, 13, d_q.ptr, d_db.ptr, q, n, dim, *out)))[entry]
            run()
            api.sync()
            api.profile_begin(deferred=True)
            run()
            api.sync()
            prof = api.profile_end()
            counts[(entry, q, topk)] = {name: int(v["launches"]) for name, v in prof.items()}
        finally:
            for b in up:
                b.free()
    first = counts[("topk", 1, 1)]
    assert all(c == first for c in counts.values()), counts
    assert {name: first[name] for name in first if name.startswith("k_nv_")} == dict(k_nv_rounds=1, k_nv_qmin=1, k_nv_is_equal=1, k_nv_mask=1,
                                                                                     k_nv_select=1), first


def test_rank_windows_store_their_cells_and_nothing_else(api, O):
    """vdb_wit_nearest_topk_dev under rank windows: random ones, one across a round boundary, one across a mask block, the full range"""
    from halo2_vectordb_amd._lib import check
    lib = api.init()
    rng = np.random.default_rng(2027)
    P = 48
    for case, (metric, q, n, dim, topk) in enumerate([("euclidean", 3, 5, 4, 3), ("cosine", 2, 7, 5, 2), ("manhattan", 3, 70, 3, 4), ("hamming", 2, 9, 6, 3)]):
        L = int(rng.integers(9, 14))
        v = rng.integers(0, 3, size=(q + n, dim)).astype(np.float64) * 0.5 if metric == "hamming" else rng.uniform(0.25, 3.0, size=(q + n, dim))
        qv = O.quantize(v, P)
        m = TM.topk_model(O, metric, qv[:q], qv[q:], topk, P, L, inputs=False)
        adv, lk, ind, res = m["advice"], m["lookup"], m["indicators"], m["results"]
        up = []
        try:
            d_q, d_db, d_ind, d_res = _dev(api, up, qv[:q]), _dev(api, up, qv[q:]), _dev(api, up, np.zeros_like(ind)), _dev(api, up, np.zeros_like(res))
            run = lambda d_adv, d_lk: check(lib.vdb_wit_nearest_topk_dev(api.METRICS[metric], P, L, d_q.ptr, d_db.ptr, q, n, dim, topk, d_adv.ptr, d_lk.ptr,
                                                                         None, d_ind.ptr, d_res.ptr))
            lo, hi = sorted(int(x) for x in rng.integers(0, len(adv) + 1, 2))
            llo, lhi = sorted(int(x) for x in rng.integers(0, len(lk) + 1, 2)) if len(lk) else (0, 0)
            round1 = m["regions"][(q - 1, 1)]["qmin"]               # the last query's round 1 starts here, behind round 0's mask blocks
            mask = m["regions"][(0, 0)]["mask"] + 8 * (n // 2)      # a mask block of the first query
            for window in ((lo, hi, llo, lhi), (round1 - 5, round1 + 7, 0, len(lk)), (mask + 3, mask + 8 + 2, 0, len(lk)), (0, len(adv), 0, len(lk))):
                tag = f"case {case}: {metric} q={q} n={n} dim={dim} t={topk} L={L} window {window}"
                check(lib.vdb_memset_dev(d_ind.ptr, 0, ctypes.c_size_t(ind.nbytes)))
                check(lib.vdb_memset_dev(d_res.ptr, 0, ctypes.c_size_t(res.nbytes)))
                g_adv, g_lk = _windowed(api, lib, check, adv, lk, window, run)
                _check_window(adv, lk, g_adv, g_lk, window, tag)
                assert np.array_equal(d_ind.download(ind.shape), ind) and np.array_equal(d_res.download(res.shape), res), tag
        finally:
            for b in up:
                b.free()


def test_one_round_of_one_query_is_the_query_circuit_key_and_proof(api, O):
    from halo2_vectordb_amd.pipeline import QueryHotPath, TopKQueryHotPath
    from halo2_vectordb_amd.rounds import ProverRounds
    made = []
    for cls, extra in ((QueryHotPath, {}), (TopKQueryHotPath, dict(q=1, topk=1))):
        hp = cls(n=6, dim=4, k=12, L=11, metric="cosine", tau=TAU, seed=20260002, blind_seed=5, **extra).setup()
        pr = ProverRounds(hp).keygen()
        try:
            assert pr.keygen_report.violations() == 0
            out = pr.prove(None, seed=23)
            made.append(({name: np.array(pr.fixed[name].commits) for name in FIXED}, int(O.fr_to_ints(np.asarray(pr.vk_digest()).reshape(1, 4))[0]),
                         out["proof"], out["instances"], hp.d_stream.download((hp.n_cells, 4))))
        finally:
            pr.free()
            hp.free()
    (f0, d0, p0, i0, s0), (f1, d1, p1, i1, s1) = made
    assert np.array_equal(s0, s1) and i0 == i1 and len(i0) == 5
    for name in FIXED:
        assert np.array_equal(f0[name], f1[name]), name
    assert d0 == d1 and p0 == p1


def test_proof_states_every_neighbour_and_the_root(api, O):
    from halo2_vectordb_amd import verifier
    from halo2_vectordb_amd.pipeline import TopKQueryHotPath
    from halo2_vectordb_amd.rounds import ProverRounds, quotient_identity_holds
    from oracle import pairing as PR
    q, n, dim, topk = 2, 6, 4, 3
    v = separated_inputs("cosine", q, n, dim, topk, seed=8)
    hp = TopKQueryHotPath(topk=topk, q=q, n=n, dim=dim, k=12, L=11, metric="cosine", tau=TAU, vectors=v).setup()
    pr = ProverRounds(hp).keygen()
    try:
        assert pr.keygen_report.violations() == 0, pr.keygen_report.as_dict()
        out = pr.prove(None, seed=17)
        m = _model(O, hp, "cosine", 48, 11, 12)
        want = TM.to_ints(m["results"]) + TM.to_ints(m["root"])
        assert out["instances"] == want and len(want) == q * topk * dim + 1
        assert quotient_identity_holds(pr, out["challenges"], out["evals"], out["instances"])
        vk = verifier.VerifyingKey.from_prover(pr, out["opened"])
        assert verifier.verify(out["proof"], want, vk)
        yvk = dict(meta=_meta(pr), opened=out["opened"], fixed={name: pr.fixed[name].commits for name in FIXED}, tau_h=PR.pt_mul(PR.G2, TAU))
        assert _verify(O, api, out["proof"], {**yvk, "instances": want})
        wrong_root = list(want)
        wrong_root[-1] = (wrong_root[-1] + 1) % O.R_MOD
        assert not verifier.verify(out["proof"], wrong_root, vk)
        swapped = list(want)                                         # the nearest and the second nearest of query 0 in the wrong order
        swapped[0:dim], swapped[dim:2 * dim] = want[dim:2 * dim], want[0:dim]
        assert swapped != want and not verifier.verify(out["proof"], swapped, vk)
    finally:
        pr.free()
        hp.free()


def test_second_prover_writes_the_same_key_and_proof(api, O):
    """oracle/prover.py on the model's witness and the device-placed map as downloaded"""
    from halo2_vectordb_amd.pipeline import TopKQueryHotPath
    from halo2_vectordb_amd.rounds import ProverRounds
    from oracle import prover as PV
    from test_gpu_cpu_prover import _compare, _int
    q, n, dim, topk, k, P, L = 2, 4, 3, 2, 12, 48, 11
    v = separated_inputs("euclidean", q, n, dim, topk, seed=21)
    hp = TopKQueryHotPath(topk=topk, q=q, n=n, dim=dim, k=k, P=P, L=L, metric="euclidean", tau=TAU, vectors=v).setup()
    pr = ProverRounds(hp).keygen()
    try:
        assert pr.keygen_report.violations() == 0
        m = _model(O, hp, "euclidean", P, L, k)
        stream = m["advice"]
        assert stream.shape[0] == hp.n_cells and m["lookup"].shape[0] == hp.n_lookup
        cm = pr.circuit
        cs = PV.Circuit(k, L, m["break_points"], m["selectors"], m["lookup"].shape[0], cm.copy_of, cm.const_idx, cm.consts, cm.lookup_src,
                        list(pr.instance_cells))
        assert len(pr.instance_cells) == q * topk * dim + 1 and np.array_equal(stream[pr.instance_cells[-1]], m["root"])
        _pk, outs = _compare(O, PV, hp, pr, cs, stream, m["lookup"], seeds=(34,))
        assert outs[0]["instances"] == TM.to_ints(m["results"]) + [_int(O, m["root"])]
    finally:
        pr.free()
        hp.free()


def test_two_sharded_ranks_write_the_one_rank_proof(tmp_path):
    one = _run(1, "topk_query", str(tmp_path / "p1.bin"), 0)
    assert one["every_rank_wrote_the_same_bytes"] and one["quotient_identity_at_x_holds"] and one["mock_prover_violations"] == 0
    rep = _run(2, "topk_query", str(tmp_path / "p2.bin"), 29573)
    assert rep["world"] == 2 and rep["every_rank_wrote_the_same_bytes"] and rep["quotient_identity_at_x_holds"]
    assert open(tmp_path / "p2.bin", "rb").read() == open(tmp_path / "p1.bin", "rb").read()
    assert rep["sha256"] == one["sha256"] and rep["n_instances"] == one["n_instances"] == 2 * 3 * 4 + 1


def test_every_altered_cell_of_a_mask_block_or_a_later_is_equal_is_noticed(api, O):
    """under-constraint spot check with the whole map on the device (vdb_mock_check_dev): each of the 8 cells of a mask block and each
    of the 12 cells of a round-1 is_equal, altered alone, gives at least one violation"""
    from halo2_vectordb_amd.pipeline import TopKQueryHotPath
    from halo2_vectordb_amd.rounds import ProverRounds
    q, n, dim, topk = 1, 4, 3, 2
    v = separated_inputs("euclidean", q, n, dim, topk, seed=4)
    hp = TopKQueryHotPath(topk=topk, q=q, n=n, dim=dim, k=12, L=11, metric="euclidean", tau=TAU, vectors=v).setup()
    pr = ProverRounds(hp).keygen()
    try:
        assert pr.keygen_report.violations() == 0
        assert pr.mock_check().violations() == 0
        m = _model(O, hp, "euclidean", 48, 11, 12)
        stream = hp.d_stream.download((hp.n_cells, 4))
        assert np.array_equal(stream, m["advice"])
        # the second mask block, and the round-1 is_equal of an entry that is not that round's minimum (where it is, x = 0 and
        # is_zero's inverse cell is free by construction: z + 0 * inv = 1 holds for every inv)
        loser = int(np.flatnonzero(m["indicator_bits"][0, 1] == 0)[0])
        mask, iseq = m["regions"][(0, 0)]["mask"] + 8, m["regions"][(0, 1)]["is_equal"] + 12 * loser
        one = O.fr_from_ints([1])
        d_flags = api.DeviceBuffer(hp.n_cells)
        try:
            d_flags.upload(np.asarray(pr.circuit.gate).astype(np.uint8))
            assert pr.mock_check(d_flags).violations() == 0          # the witness as it lies in HBM, not emitted again
            for cell in list(range(mask, mask + 8)) + list(range(iseq, iseq + 12)):
                hp.d_stream.upload(O.fr_add(stream[cell:cell + 1], one), offset=cell * 32)
                rep = pr.mock_check(d_flags)
                hp.d_stream.upload(np.ascontiguousarray(stream[cell:cell + 1]), offset=cell * 32)
                assert rep.violations() >= 1, (cell, rep.as_dict())
        finally:
            d_flags.free()
    finally:
        pr.free()
        hp.free()
