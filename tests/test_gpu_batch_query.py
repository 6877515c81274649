"""A batch of queries against one committed database in one proof (pipeline.BatchQueryHotPath; vdb_wit_nearest_batch*): the closure
a user of the reference's chips writes — assign the queries, assign the database, nearest_vector per query
(src/gadget/vectordb.rs:122-163), merkle_commitment once (:165-223) — on the GPU.  The streams are the oracle's context run in that
order, cell for cell; the batch entry point writes the bytes of q single-query calls; q = 1 is the query circuit, key and proof; the
whole proof states every result and the root; the second prover, two sharded ranks and a rank window agree."""
import ctypes

import numpy as np
import pytest

from test_gpu_rounds import FIXED, TAU, _meta, _verify
from test_gpu_sharded import _run
from test_gpu_sweep import _check_window, _windowed

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def api():
    from halo2_vectordb_amd import api as a
    a.init(0)
    return a


def _oracle(O, hp, metric, P, L, k, merkle=True):
    """the oracle's context run in the circuit's order; -> (context, indicators (q, n, 4), results (q, dim, 4), root)"""
    qv = hp.qvec
    q = hp.q
    c = O.Ctx(store=True, keygen=True, plan_k=k)
    c.assign_witnesses(qv[:q])
    c.assign_witnesses(qv[q:])
    outs = [c.nearest_vector(metric, qv[i], qv[q:], P=P, L=L) for i in range(q)]
    root = c.merkle_commitment(qv[q:]) if merkle else None
    return c, np.stack([o[0] for o in outs]), np.stack([o[1] for o in outs]), root


def _f64_distances(metric, v, q):
    """(q, n) distances of the f64 rows, queries first"""
    qs, db = v[:q], v[q:]
    if metric == "euclidean":
        return np.linalg.norm(db[None, :, :] - qs[:, None, :], axis=2)
    if metric == "manhattan":
        return np.abs(db[None, :, :] - qs[:, None, :]).sum(axis=2)
    if metric == "cosine":
        return 1 - (qs @ db.T) / (np.linalg.norm(qs, axis=1)[:, None] * np.linalg.norm(db, axis=1)[None, :])
    return 1 - (db[None, :, :] == qs[:, None, :]).mean(axis=2)


def _stream_parity(api, O, hp, metric, P, L, k):
    try:
        d_flags = hp.keygen_flags()
        flags = d_flags.download((hp.n_cells,), dtype=np.uint8)
        d_flags.free()
        hp._witness()
        api.sync()
        c, ind, res, root = _oracle(O, hp, metric, P, L, k)
        assert c.err == 0
        assert len(c) == hp.n_cells and c.n_lookup == hp.n_lookup
        assert len(c) == hp.n_in + hp.nearest_cells + hp.merkle_cells
        got, want = hp.d_stream.download((hp.n_cells, 4)), c.advice()
        bad = np.flatnonzero((got != want).any(axis=1))
        assert bad.size == 0, f"first differing advice cells {bad[:5]} of {hp.n_cells}"
        assert np.array_equal(hp.d_lookup.download((hp.n_lookup, 4)), c.lookup())
        assert np.array_equal(flags & 1, c.selectors().astype(np.uint8) & 1)
        assert np.array_equal(hp.bp, c.break_points())
        g_ind, g_res, g_root = hp.results()
        assert np.array_equal(g_ind, ind) and np.array_equal(g_res, res) and np.array_equal(g_root, root)
        ptr, count = hp.public_values_dev()
        assert count == hp.q * hp.dim + 1
        pub = hp.d_pub.download((count, 4))
        assert np.array_equal(pub[:-1], res.reshape(-1, 4)) and np.array_equal(pub[-1], root)
        bits = np.asarray(O.fr_to_ints(g_ind.reshape(-1, 4)), dtype=object).reshape(hp.q, hp.n)
        assert set(int(b) for b in bits.reshape(-1)) <= {0, 1} and all(int(row.sum()) >= 1 for row in bits)
        d = _f64_distances(metric, hp.vectors_f64, hp.q)
        for i in range(hp.q):
            order = np.sort(d[i])
            if len(order) == 1 or order[1] - order[0] > 1e-9:                 # a unique minimum: f64 names the same vector
                assert [int(b) for b in bits[i]] == [int(j == int(np.argmin(d[i]))) for j in range(hp.n)], i
        return bits
    finally:
        hp.free()


def test_cosine_batch_stream_is_the_oracles(api, O):
    from halo2_vectordb_amd.pipeline import BatchQueryHotPath
    hp = BatchQueryHotPath(q=3, n=6, dim=4, k=12, L=11, metric="cosine", tau=TAU).setup()
    assert (hp.n_in, hp.nearest_cells, hp.merkle_cells, hp.n_lookup) == (36, 923328, 72115, 142938)
    _stream_parity(api, O, hp, "cosine", 48, 11, 12)


def test_euclidean_batch_stream_is_the_oracles(api, O):
    from halo2_vectordb_amd.pipeline import BatchQueryHotPath
    hp = BatchQueryHotPath(q=3, n=5, dim=4, k=12, L=11, metric="euclidean", tau=TAU).setup()
    assert (hp.n_in + hp.nearest_cells, hp.n_lookup) == (368270, 54951)          # the cells before the commitment
    _stream_parity(api, O, hp, "euclidean", 48, 11, 12)


def test_tied_minimum_sets_every_indicator_of_the_tie(api, O):
    """Hamming over 0 / 1 vectors: a seed under which every query's smallest distance is reached by two database vectors at least —
    is_equal(min, d_i) sets all of them and select_by_indicator ends on the last (stream parity only: nothing is proved here)"""
    from halo2_vectordb_amd.pipeline import BatchQueryHotPath
    q, n, dim = 2, 5, 4
    for seed in range(200):
        v = np.random.default_rng(seed).integers(0, 2, size=(q + n, dim)).astype(np.float64)
        d = _f64_distances("hamming", v, q)
        if all(int((row == row.min()).sum()) >= 2 for row in d):
            break
    else:
        raise AssertionError("no seed with a tied minimum in every query")
    hp = BatchQueryHotPath(q=q, n=n, dim=dim, k=12, L=11, metric="hamming", tau=TAU, vectors=v).setup()
    bits = _stream_parity(api, O, hp, "hamming", 48, 11, 12)
    for i in range(q):
        assert [int(b) for b in bits[i]] == [int(x == d[i].min()) for x in d[i]] and int(bits[i].sum()) >= 2


def test_database_of_one_vector(api, O):
    """n = 1: no qmin chain at all, one is_equal, a select over one vector — every query's result is that vector"""
    from halo2_vectordb_amd.pipeline import BatchQueryHotPath
    hp = BatchQueryHotPath(q=2, n=1, dim=4, k=12, L=11, metric="euclidean", tau=TAU).setup()
    bits = _stream_parity(api, O, hp, "euclidean", 48, 11, 12)
    assert [int(b) for b in bits.reshape(-1)] == [1, 1]


def test_tiled_scan_and_more_than_one_wavefront_of_queries(api, O):
    """Manhattan, q = 70, n = 130, dim = 2: the prefix minima of a query span three 64-wide tiles of the scan (64 + 64 + 2), and the
    batch holds more queries than a wavefront has lanes"""
    from halo2_vectordb_amd.pipeline import BatchQueryHotPath
    rng = np.random.default_rng(130)
    v = rng.uniform(-2.5, 2.5, size=(70 + 130, 2))
    hp = BatchQueryHotPath(q=70, n=130, dim=2, k=14, L=13, metric="manhattan", tau=TAU, vectors=v).setup()
    _stream_parity(api, O, hp, "manhattan", 48, 13, 14)


def _dev(api, up, a):
    b = api.DeviceBuffer(max(a.nbytes, 32))
    b.upload(np.ascontiguousarray(a))
    up.append(b)
    return b


def _both_ways(api, metric, queries, db, P, L):
    """vdb_wit_nearest_batch_dev, and q calls of vdb_wit_nearest_dev at the matching offsets: -> two tuples of
    (stream, lookup, flags, indicators, results) as left in identically prepared buffers"""
    from halo2_vectordb_amd._lib import check
    lib = api.init()
    q, n, dim = queries.shape[0], db.shape[0], db.shape[1]
    cells, lk = ctypes.c_uint64(), ctypes.c_uint64()
    check(lib.vdb_wit_nearest_batch_size(api.METRICS[metric], P, L, q, n, dim, ctypes.byref(cells), ctypes.byref(lk)))
    c1, l1 = ctypes.c_uint64(), ctypes.c_uint64()
    check(lib.vdb_wit_nearest_size(api.METRICS[metric], P, L, n, dim, ctypes.byref(c1), ctypes.byref(l1)))
    assert cells.value == q * c1.value and lk.value == q * l1.value
    cells, lk, c1, l1 = cells.value, lk.value, c1.value, l1.value
    up, outs = [], []
    try:
        d_q, d_db = _dev(api, up, queries), _dev(api, up, db)
        for batch in (True, False):
            d_adv, d_lk, d_sel = api.DeviceBuffer(cells * 32), api.DeviceBuffer(max(lk, 1) * 32), api.DeviceBuffer(cells)
            d_ind, d_res = api.DeviceBuffer(q * n * 32), api.DeviceBuffer(q * dim * 32)
            up += [d_adv, d_lk, d_sel, d_ind, d_res]
            check(lib.vdb_memset_dev(d_adv.ptr, 0xA5, ctypes.c_size_t(cells * 32)))
            check(lib.vdb_memset_dev(d_lk.ptr, 0xA5, ctypes.c_size_t(max(lk, 1) * 32)))
            check(lib.vdb_memset_dev(d_sel.ptr, 0, ctypes.c_size_t(cells)))
            if batch:
                check(lib.vdb_wit_nearest_batch_dev(api.METRICS[metric], P, L, d_q.ptr, d_db.ptr, q, n, dim, d_adv.ptr, d_lk.ptr, d_sel.ptr, d_ind.ptr,
                                                    d_res.ptr))
            else:
                for i in range(q):
                    check(lib.vdb_wit_nearest_dev(api.METRICS[metric], P, L, d_q.at(i * dim * 32), d_db.ptr, n, dim, d_adv.at(i * c1 * 32),
                                                  d_lk.at(i * l1 * 32), ctypes.c_void_p(d_sel.ptr.value + i * c1), d_ind.at(i * n * 32),
                                                  d_res.at(i * dim * 32)))
            api.sync()
            outs.append((d_adv.download((cells, 4)), d_lk.download((max(lk, 1), 4)), d_sel.download((cells,), dtype=np.uint8),
                         d_ind.download((q, n, 4)), d_res.download((q, dim, 4))))
    finally:
        for b in up:
            b.free()
    return outs


@pytest.mark.parametrize("metric,q,n,dim,L", [("euclidean", 3, 5, 4, 11), ("cosine", 5, 9, 3, 12), ("manhattan", 66, 70, 2, 10), ("hamming", 4, 17, 6, 9),
                                              ("manhattan", 2, 1, 3, 11), ("euclidean", 1, 7, 130, 13)])
def test_batch_entry_point_writes_the_bytes_of_single_query_calls(api, O, metric, q, n, dim, L):
    rng = np.random.default_rng(q * 1000 + n * 10 + dim)
    v = rng.integers(0, 3, size=(q + n, dim)).astype(np.float64) * 0.5 if metric == "hamming" else rng.uniform(0.25, 3.0, size=(q + n, dim))
    qv = O.quantize(v, 48)
    got, want = _both_ways(api, metric, qv[:q], qv[q:], 48, L)
    for name, a, b in zip(("stream", "lookup", "flags", "indicators", "results"), got, want):
        assert np.array_equal(a, b), name
    # the host-pointer form returns the same streams
    host = api.wit_nearest_batch(metric, qv[:q], qv[q:], P=48, L=L, selectors=True)
    assert np.array_equal(host["stream"], got[0]) and np.array_equal(host["flags"], got[2])
    assert np.array_equal(host["indicators"], got[3]) and np.array_equal(host["results"], got[4])
    if host["lookup"].shape[0]:
        assert np.array_equal(host["lookup"], got[1])


def test_prefix_minima_follow_the_serial_fold_on_values_no_order_holds_for(api, O):
    """full-width field elements as vectors (nothing quantizes to them): is_neg(m - x) is no order over the Manhattan 'distances' of
    such inputs, and the qmin chain is whatever the serial fold makes of them — the batch writes the single-query path's bytes"""
    rng = np.random.default_rng(99)
    q, n, dim = 5, 150, 2
    raw = O.random_fr(rng, (q + n) * dim).reshape(q + n, dim, 4)
    got, want = _both_ways(api, "manhattan", raw[:q], raw[q:], 48, 11)
    for name, a, b in zip(("stream", "lookup", "flags", "indicators", "results"), got, want):
        assert np.array_equal(a, b), name


def test_batch_arguments_and_limits(api):
    from halo2_vectordb_amd._lib import check
    lib = api.init()
    cells, lk = ctypes.c_uint64(), ctypes.c_uint64()
    for q, n, dim in ((0, 4, 4), (4, 0, 4), ((1 << 24) + 1, 1, 1), (1 << 13, 1 << 12, 1), (1 << 20, 16, 64)):
        with pytest.raises(api.VdbError) as e:
            check(lib.vdb_wit_nearest_batch_size(0, 48, 11, q, n, dim, ctypes.byref(cells), ctypes.byref(lk)))
        assert e.value.code == -3, (q, n, dim)                      # VDB_ERR_ARG
    with pytest.raises(api.VdbError):
        check(lib.vdb_wit_nearest_batch_size(7, 48, 11, 2, 4, 4, ctypes.byref(cells), ctypes.byref(lk)))
    # a query equal to a database row under the cosine of a zero vector: the division by zero the reference panics on
    z = np.zeros((3, 4, 4), dtype=np.uint64)
    with pytest.raises(api.VdbError) as e:
        api.wit_nearest_batch("cosine", z[:1], z[1:], P=48, L=11)
    assert e.value.code == -5                                       # VDB_ERR_DOMAIN


def test_a_batch_of_one_is_the_query_circuit_key_and_proof(api, O):
    from halo2_vectordb_amd.pipeline import BatchQueryHotPath, QueryHotPath
    from halo2_vectordb_amd.rounds import ProverRounds
    made = []
    for cls, extra in ((QueryHotPath, {}), (BatchQueryHotPath, dict(q=1))):
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


def test_batch_proof_states_every_result_and_the_root(api, O):
    from halo2_vectordb_amd import verifier
    from halo2_vectordb_amd.pipeline import BatchQueryHotPath
    from halo2_vectordb_amd.rounds import ProverRounds, quotient_identity_holds
    from oracle import pairing as PR
    q, n, dim = 3, 6, 4
    hp = BatchQueryHotPath(q=q, n=n, dim=dim, k=12, L=11, metric="cosine", tau=TAU).setup()
    pr = ProverRounds(hp).keygen()
    try:
        assert pr.keygen_report.violations() == 0, pr.keygen_report.as_dict()
        cm = pr.circuit
        # a database word is copied by every query's distances, every query's select and its leaf
        assert all(int((cm.copy_of == w).sum()) >= 2 * q + 1 for w in range(q * dim, q * dim + 8))
        out = pr.prove(None, seed=17)
        c, _ind, res, root = _oracle(O, hp, "cosine", 48, 11, 12)
        want = O.fr_to_ints(res.reshape(-1, 4)) + O.fr_to_ints(root.reshape(1, 4))
        assert out["instances"] == want and len(want) == q * dim + 1
        assert quotient_identity_holds(pr, out["challenges"], out["evals"], out["instances"])
        vk = verifier.VerifyingKey.from_prover(pr, out["opened"])
        assert verifier.verify(out["proof"], want, vk)
        yvk = dict(meta=_meta(pr), opened=out["opened"], fixed={name: pr.fixed[name].commits for name in FIXED}, tau_h=PR.pt_mul(PR.G2, TAU))
        assert _verify(O, api, out["proof"], {**yvk, "instances": want})
        for i in (0, q * dim - 1, q * dim):                        # a word of the first result, of the last result, the root
            other = list(want)
            other[i] = (other[i] + 1) % O.R_MOD
            assert not verifier.verify(out["proof"], other, vk), i
        a, b = next((a, b) for a in range(q) for b in range(a + 1, q) if want[a * dim:(a + 1) * dim] != want[b * dim:(b + 1) * dim])
        swapped = list(want)
        swapped[a * dim:(a + 1) * dim], swapped[b * dim:(b + 1) * dim] = want[b * dim:(b + 1) * dim], want[a * dim:(a + 1) * dim]
        assert not verifier.verify(out["proof"], swapped, vk)
        # another database (and other queries) under the same key
        rng = np.random.default_rng(5)
        hp.set_vectors(rng.integers(0, 219, size=(q + n, dim)).astype(np.float64) + rng.random((q + n, dim)))
        assert pr.mock_check().violations() == 0
        out2 = pr.prove(None)
        assert out2["instances"] != want
        assert verifier.verify(out2["proof"], out2["instances"], verifier.VerifyingKey.from_prover(pr, out2["opened"]))
        assert not verifier.verify(out2["proof"], want, verifier.VerifyingKey.from_prover(pr, out2["opened"]))
    finally:
        pr.free()
        hp.free()


def test_second_prover_writes_the_same_key_and_proof(api, O):
    """oracle/prover.py on the oracle's witness of the closure and the device-placed map as downloaded: verifying key and proof bytes
    equal, as tests/test_gpu_cpu_prover.py holds the query circuit"""
    from halo2_vectordb_amd.pipeline import BatchQueryHotPath
    from halo2_vectordb_amd.rounds import ProverRounds
    from oracle import prover as PV
    from test_gpu_cpu_prover import _compare, _int
    q, n, dim, k, P, L = 2, 4, 3, 12, 48, 11
    hp = BatchQueryHotPath(q=q, n=n, dim=dim, k=k, P=P, L=L, metric="euclidean", tau=TAU).setup()
    pr = ProverRounds(hp).keygen()
    try:
        assert pr.keygen_report.violations() == 0
        c, _ind, res, root = _oracle(O, hp, "euclidean", P, L, k)
        stream = c.advice()
        assert c.err == 0 and stream.shape[0] == hp.n_cells and c.n_lookup == hp.n_lookup
        cm = pr.circuit
        cs = PV.Circuit(k, L, c.break_points(), c.selectors(), c.n_lookup, cm.copy_of, cm.const_idx, cm.consts, cm.lookup_src, list(pr.instance_cells))
        assert len(pr.instance_cells) == q * dim + 1 and np.array_equal(stream[pr.instance_cells[-1]], root)
        _pk, outs = _compare(O, PV, hp, pr, cs, stream, c.lookup(), seeds=(34,))
        assert outs[0]["instances"] == [int(v) for v in O.fr_to_ints(res.reshape(-1, 4))] + [_int(O, root)]
    finally:
        pr.free()
        hp.free()


def test_two_sharded_ranks_write_the_one_rank_proof(tmp_path):
    one = _run(1, "batch_query", str(tmp_path / "p1.bin"), 0)
    assert one["every_rank_wrote_the_same_bytes"] and one["quotient_identity_at_x_holds"] and one["mock_prover_violations"] == 0
    rep = _run(2, "batch_query", str(tmp_path / "p2.bin"), 29571)
    assert rep["world"] == 2 and rep["every_rank_wrote_the_same_bytes"] and rep["quotient_identity_at_x_holds"]
    assert open(tmp_path / "p2.bin", "rb").read() == open(tmp_path / "p1.bin", "rb").read()
    assert rep["sha256"] == one["sha256"] and rep["n_instances"] == one["n_instances"] == 3 * 4 + 1


def test_rank_windows_store_their_cells_and_nothing_else(api, O):
    """vdb_wit_nearest_batch_dev under random rank windows: cells inside equal the full run's (the oracle's), cells outside untouched,
    every rank computes every indicator and result"""
    from halo2_vectordb_amd._lib import check
    lib = api.init()
    rng = np.random.default_rng(2026)
    P = 48
    for case, (metric, q, n, dim) in enumerate([("euclidean", 3, 5, 4), ("cosine", 2, 7, 5), ("manhattan", 5, 70, 3), ("hamming", 4, 9, 6), ("euclidean", 6, 20, 67)]):
        L = int(rng.integers(9, 14))
        v = rng.integers(0, 3, size=(q + n, dim)).astype(np.float64) * 0.5 if metric == "hamming" else rng.uniform(0.25, 3.0, size=(q + n, dim))
        qv = O.quantize(v, P)
        c = O.Ctx(store=True)
        outs = [c.nearest_vector(metric, qv[i], qv[q:], P=P, L=L) for i in range(q)]
        assert c.err == 0
        ind, res = np.stack([o[0] for o in outs]), np.stack([o[1] for o in outs])
        adv, lk = c.advice(), c.lookup()
        up = []
        try:
            d_q, d_db, d_ind, d_res = _dev(api, up, qv[:q]), _dev(api, up, qv[q:]), _dev(api, up, np.zeros_like(ind)), _dev(api, up, np.zeros_like(res))
            run = lambda d_adv, d_lk: check(lib.vdb_wit_nearest_batch_dev(api.METRICS[metric], P, L, d_q.ptr, d_db.ptr, q, n, dim, d_adv.ptr, d_lk.ptr, None,
                                                                          d_ind.ptr, d_res.ptr))
            lo, hi = sorted(int(x) for x in rng.integers(0, len(adv) + 1, 2))
            llo, lhi = sorted(int(x) for x in rng.integers(0, len(lk) + 1, 2)) if len(lk) else (0, 0)
            per_q = len(adv) // q
            for window in ((lo, hi, llo, lhi), (per_q - 3, per_q + 5, 0, len(lk)), (0, len(adv), 0, len(lk))):
                tag = f"case {case}: {metric} q={q} n={n} dim={dim} L={L} window {window}"
                check(lib.vdb_memset_dev(d_ind.ptr, 0, ctypes.c_size_t(ind.nbytes)))
                check(lib.vdb_memset_dev(d_res.ptr, 0, ctypes.c_size_t(res.nbytes)))
                g_adv, g_lk = _windowed(api, lib, check, adv, lk, window, run)
                _check_window(adv, lk, g_adv, g_lk, window, tag)
                assert np.array_equal(d_ind.download(ind.shape), ind) and np.array_equal(d_res.download(res.shape), res), tag
        finally:
            for b in up:
                b.free()
