"""The top-k query circuit without a GPU.  tests/topk_model.py is the checker of the GPU streams, so nothing of it is taken on trust:
its three integer templates and its row walk are held against the oracle's own cells first; at t = 1 the model is the oracle's
nearest_vector run; the block-built constraint map (circuit_sym.build_nearest_topk) is the whole-circuit trace, at t = 1 the batch
map, accepts the model's witness for every metric and notices an altered cell in each region the feature adds; the model's rounds
name the vectors f64 sorting names; and the library exports the entry points."""
import ctypes
import os

import numpy as np
import pytest

import topk_model as TM
from halo2_vectordb_amd import circuit_sym as CS
from test_batch_query_cpu import same_map

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P, L = 48, 11
METRICS = ("euclidean", "cosine", "manhattan", "hamming")


def f64_distances(metric, v, q):
    """(q, n) distances of the f64 rows, queries first"""
    qs, db = v[:q], v[q:]
    if metric == "euclidean":
        return np.linalg.norm(db[None, :, :] - qs[:, None, :], axis=2)
    if metric == "manhattan":
        return np.abs(db[None, :, :] - qs[:, None, :]).sum(axis=2)
    if metric == "cosine":
        return 1 - (qs @ db.T) / (np.linalg.norm(qs, axis=1)[:, None] * np.linalg.norm(db, axis=1)[None, :])
    return 1 - (db[None, :, :] == qs[:, None, :]).mean(axis=2)


def separated_inputs(metric, q, n, dim, topk, seed):
    """f64 rows (queries first) whose topk + 1 smallest distances differ pairwise by more than 1e-9 in every query — asserted, not
    searched for: Hamming rows are built so (database row i differs from every query in exactly i + 1 of the leading places, the
    queries share those places), the other metrics draw continuous values, for which the margin is many orders above what can collide"""
    rng = np.random.default_rng(seed)
    if metric == "hamming":
        assert n <= dim
        lead = rng.integers(0, 2, size=dim).astype(np.float64)
        queries = np.tile(lead, (q, 1))
        db = np.tile(lead, (n, 1))
        for i, row in enumerate(rng.permutation(n)):
            db[row, : i + 1] = 1 - lead[: i + 1]
        v = np.concatenate([queries, db])
    else:
        v = rng.uniform(0.25, 3.0, size=(q + n, dim))
    d = np.sort(f64_distances(metric, v, q), axis=1)[:, : min(topk + 1, n)]
    assert (np.diff(d, axis=1) > 1e-9).all(), "the inputs of this test must separate their nearest distances"
    return v


# ---------------------------------------------------------------------------------------------------------------- the model's parts
@pytest.mark.parametrize("metric,n,dim", [("euclidean", 5, 4), ("hamming", 6, 3), ("manhattan", 1, 2)])
def test_is_equal_and_select_by_indicator_templates_are_the_oracles_cells(O, metric, n, dim):
    """the closing cells of an oracle nearest_vector: n is_equal(min, d_i) blocks, then dim select_by_indicator walks (Hamming over
    0 / 1 rows: several indicators set, the walk ends on the last of them)"""
    rng = np.random.default_rng(n * 10 + dim)
    v = rng.uniform(0.25, 3.0, size=(n + 1, dim))
    if metric == "hamming":                              # the query, then rows at 2/3, 1/3, 1, 1/3, 2/3, 1/3: the minimum three times
        v = np.asarray([[0, 0, 0], [1, 1, 0], [0, 0, 1], [1, 1, 1], [1, 0, 0], [0, 1, 1], [0, 1, 0]], dtype=np.float64)
    qv = O.quantize(v, P)
    c = O.Ctx(store=True, keygen=True)
    ind, res = c.nearest_vector(metric, qv[0], qv[1:], P=P, L=L)
    assert c.err == 0
    adv, sel = TM.to_ints(c.advice()), c.selectors().astype(np.uint8) & 1
    cd = O.Ctx(store=True, keygen=True)
    d = TM.to_ints(np.stack([cd.distance(metric, qv[1 + i], qv[0], P=P, L=L) for i in range(n)]))
    cq = O.Ctx(store=True, keygen=True)
    m = O.fr_from_ints([d[0]])[0]
    for i in range(1, n):
        m = cq.op("qmin", m, O.fr_from_ints([d[i]])[0], P=P, L=L)
    (m,) = TM.to_ints(m)
    at = len(cd) + len(cq)
    assert len(c) == at + 12 * n + dim * (1 + 3 * n)
    bits = []
    for i in range(n):
        cells, gates, z = TM.is_equal(m, d[i])
        assert cells == adv[at:at + 12] and gates == list(sel[at:at + 12]), i
        bits.append(z)
        at += 12
    assert bits == TM.to_ints(ind) and sum(bits) >= 1
    if metric == "hamming":
        assert bits == [0, 1, 0, 1, 0, 1]
    db = [TM.to_ints(qv[1 + i]) for i in range(n)]
    for j in range(dim):
        cells, gates, out = TM.select_by_indicator([db[i][j] for i in range(n)], bits)
        assert cells == adv[at:at + 1 + 3 * n] and gates == list(sel[at:at + 1 + 3 * n]), j
        assert out == TM.to_ints(res[j])[0]
        at += 1 + 3 * n
    assert at == len(adv)


@pytest.mark.parametrize("a,b", [(0.5, 1.25), (1.25, 0.5), (-2.0, 0.75), (1.5, 1.5)])
def test_select_template_is_the_last_eight_cells_of_an_oracle_qmin(O, a, b):
    """qmin(a, b) ends in select(a, b, is_neg(a - b))"""
    qa, qb = O.quantize(np.asarray([a]), P)[0], O.quantize(np.asarray([b]), P)[0]
    c = O.Ctx(store=True, keygen=True)
    out = c.op("qmin", qa, qb, P=P, L=L)
    adv, sel = TM.to_ints(c.advice()), c.selectors().astype(np.uint8) & 1
    (ia,), (ib,) = TM.to_ints(qa), TM.to_ints(qb)
    s = adv[-3]                                           # the selector cell as the oracle computed it
    assert s == int(a < b)
    cells, gates, o = TM.select(ia, ib, s)
    assert cells == adv[-8:] and gates == list(sel[-8:]) and o == TM.to_ints(out)[0] == (ia if a < b else ib)


@pytest.mark.parametrize("k", [8, 9])
def test_row_walk_gives_the_oracles_break_points(O, k):
    rng = np.random.default_rng(k)
    qv = O.quantize(rng.uniform(0.25, 3.0, size=(5, 3)), P)
    c = O.Ctx(store=True, keygen=True, plan_k=k)
    c.assign_witnesses(qv)
    c.nearest_vector("euclidean", qv[0], qv[1:], P=P, L=L)
    c.nearest_vector("manhattan", qv[1], qv[:3], P=P, L=L)
    want = c.break_points()
    assert len(want) >= 5
    assert np.array_equal(TM.row_walk(c.selectors(), k), want)


@pytest.mark.parametrize("metric,q,n,dim", [("euclidean", 3, 5, 4), ("cosine", 2, 4, 3), ("manhattan", 2, 1, 2), ("hamming", 2, 5, 4)])
def test_model_with_one_round_is_the_oracles_nearest_vector_run(O, metric, q, n, dim):
    """assign the queries, assign the database, nearest_vector per query, merkle_commitment: advice, lookup, selectors, break points"""
    rng = np.random.default_rng(q * 100 + n * 10 + dim)
    v = rng.integers(0, 2, size=(q + n, dim)).astype(np.float64) if metric == "hamming" else rng.uniform(0.25, 3.0, size=(q + n, dim))
    qv = O.quantize(v, P)
    c = O.Ctx(store=True, keygen=True, plan_k=10)
    c.assign_witnesses(qv[:q])
    c.assign_witnesses(qv[q:])
    outs = [c.nearest_vector(metric, qv[i], qv[q:], P=P, L=L) for i in range(q)]
    root = c.merkle_commitment(qv[q:])
    assert c.err == 0
    m = TM.topk_model(O, metric, qv[:q], qv[q:], 1, P, L, plan_k=10, merkle=True)
    assert np.array_equal(m["advice"], c.advice()) and np.array_equal(m["lookup"], c.lookup())
    assert np.array_equal(m["selectors"], c.selectors().astype(np.uint8) & 1)
    assert np.array_equal(m["break_points"], c.break_points()) and len(m["break_points"]) >= 3
    assert np.array_equal(m["indicators"][:, 0], np.stack([o[0] for o in outs])) and np.array_equal(m["results"][:, 0], np.stack([o[1] for o in outs]))
    assert np.array_equal(m["root"], root)


# ---------------------------------------------------------------------------------------------------------------- the constraint map
@pytest.mark.parametrize("metric,q,n,dim,topk", [("euclidean", 2, 5, 4, 3), ("cosine", 2, 4, 3, 4), ("manhattan", 3, 3, 2, 2), ("hamming", 1, 4, 3, 1)])
def test_block_built_map_is_the_whole_circuit_trace(metric, q, n, dim, topk):
    cm, (ind, res) = CS.trace_nearest_topk(metric, q, n, dim, topk, P, L)
    bm, (bind, bres) = CS.build_nearest_topk(metric, q, n, dim, topk, P, L)
    same_map(cm, bm)
    assert np.array_equal(np.asarray(ind), bind) and np.array_equal(np.asarray(res), bres)
    assert bind.shape == (q, topk, n) and bres.shape == (q, topk, dim)
    # M is a constant of the circuit: one fixed-column value, tied to one cell of every mask block
    big = TM.mask_value(P)
    holds = np.flatnonzero((cm.const_idx >= 0) & (np.asarray(cm.consts + [0], dtype=object)[cm.const_idx] == big))
    assert holds.size == q * (topk - 1) * n and not cm.asserted[holds].any()


@pytest.mark.parametrize("metric,q,n,dim", [("euclidean", 3, 5, 4), ("manhattan", 2, 1, 2)])
def test_one_round_is_the_batch_map(metric, q, n, dim):
    bm, (bind, bres) = CS.build_nearest_topk(metric, q, n, dim, 1, P, L)
    b1, (ind1, res1) = CS.build_nearest_batch(metric, q, n, dim, P, L)
    same_map(b1, bm)
    assert np.array_equal(bind[:, 0], ind1) and np.array_equal(bres[:, 0], res1)
    cm, _ = CS.trace_nearest_topk(metric, q, n, dim, 1, P, L)
    c1, _ = CS.trace_nearest_batch(metric, q, n, dim, P, L)
    same_map(c1, cm)


def test_builder_contract_and_arguments():
    whole, _ = CS.build_nearest_topk("euclidean", 2, 4, 3, 2, P, L)
    B, (ind, res), used = CS.build_nearest_topk("euclidean", 2, 4, 3, 2, P, L, builder=CS._Builder, extra_cells=77, finish=False)
    assert used == whole.n_cells and B.copy_of.shape[0] == used + 77
    cm = B.finish()
    assert np.array_equal(cm.copy_of[:used], whole.copy_of) and np.array_equal(cm.copy_of[used:], np.arange(used, used + 77))
    for topk in (0, 5):
        with pytest.raises(ValueError):
            CS.build_nearest_topk("euclidean", 2, 4, 3, topk, P, L)


@pytest.mark.parametrize("metric", METRICS)
def test_map_accepts_the_models_witness_and_notices_altered_cells(O, metric):
    q, n, dim, topk = 2, 5, 6 if metric == "hamming" else 3, 3
    v = separated_inputs(metric, q, n, dim, topk, seed=11)
    qv = O.quantize(v, P)
    m = TM.topk_model(O, metric, qv[:q], qv[q:], topk, P, L)
    bm, (ind, res) = CS.build_nearest_topk(metric, q, n, dim, topk, P, L)
    assert m["advice"].shape[0] == bm.n_cells and m["lookup"].shape[0] == len(bm.lookup_src)
    vals, lk = np.asarray(TM.to_ints(m["advice"]), dtype=object), np.asarray(TM.to_ints(m["lookup"]), dtype=object)
    rep = bm.check_witness(vals, lk, flags=m["selectors"])
    assert not any(rep.values()), rep
    assert [vals[x] for x in ind.reshape(-1)] == TM.to_ints(m["indicators"]) and [vals[x] for x in res.reshape(-1)] == TM.to_ints(m["results"])
    starts = np.flatnonzero(bm.gate)

    def gate_violations(w):
        return int(np.count_nonzero((w[starts] + w[starts + 1] * w[starts + 2] - w[starts + 3]) % CS.R))

    def violations(cell):
        alt = vals.copy()
        alt[cell] = (alt[cell] + 1) % CS.R
        rep = bm.check_witness(alt, lk)
        return rep["copies_unequal"] + rep["constants_wrong"] + rep["asserts_violated"] + rep["lookup_copies_unequal"], gate_violations(alt)

    assert gate_violations(vals) == 0
    for qi in (0, q - 1):
        for r in (1, topk - 1):
            reg, before = m["regions"][(qi, r)], m["regions"][(qi, r - 1)]
            # a mask output (the entry round r works on): the round's qmin chain and is_equal copy it, its own gate computes it
            out = before["mask"] + 8 * 1 + 7
            assert bm.copy_of[out] == out and int((bm.copy_of == out).sum()) >= 3
            assert min(violations(out)) >= 1
            # the constant M inside that mask block
            assert vals[before["mask"] + 8 + 3] == TM.mask_value(P) and violations(before["mask"] + 8 + 3)[0] >= 1
            # an indicator of round r: the selects of the round copy it (and the round's mask, where there is one)
            users = int((bm.copy_of == ind[qi, r, 0]).sum())
            assert users == dim + (1 if r + 1 < topk else 0) and violations(int(ind[qi, r, 0]))[0] >= dim
            assert reg["is_equal"] <= ind[qi, r, 0] < reg["select"]
            # a result of round r: the last cell of its running select, its own gate
            assert reg["select"] <= res[qi, r, dim - 1] and violations(int(res[qi, r, dim - 1]))[1] >= 1


# ---------------------------------------------------------------------------------------------------------------- what it computes
@pytest.mark.parametrize("metric,q,n,dim,topk", [("euclidean", 3, 9, 4, 4), ("cosine", 2, 7, 5, 7), ("manhattan", 4, 12, 3, 5), ("hamming", 2, 6, 8, 3)])
def test_rounds_name_the_vectors_f64_sorting_names(O, metric, q, n, dim, topk):
    v = separated_inputs(metric, q, n, dim, topk, seed=n * 10 + dim)
    qv = O.quantize(v, P)
    m = TM.topk_model(O, metric, qv[:q], qv[q:], topk, P, L)
    d = f64_distances(metric, v, q)
    for qi in range(q):
        order = np.argsort(d[qi], kind="stable")
        for r in range(topk):
            assert list(m["indicator_bits"][qi, r]) == [int(i == order[r]) for i in range(n)], (qi, r)
            assert np.array_equal(m["results"][qi, r], qv[q + order[r]]), (qi, r)


def test_fewer_distinct_distances_than_rounds_end_on_an_all_masked_array(O):
    """Hamming, three database rows of two distinct distances, t = 3: round 0 takes the tie (both indicators, the result is the last of
    them), round 1 the remaining row, round 2 runs on [M, M, M] and sets every indicator"""
    v = np.asarray([[0, 0, 0, 0], [0, 0, 0, 1], [1, 1, 1, 1], [1, 0, 0, 0]], dtype=np.float64)
    qv = O.quantize(v, P)
    m = TM.topk_model(O, "hamming", qv[:1], qv[1:], 3, P, L)
    assert m["indicator_bits"][0].tolist() == [[1, 0, 1], [0, 1, 0], [1, 1, 1]]
    assert np.array_equal(m["results"][0, 0], qv[3]) and np.array_equal(m["results"][0, 1], qv[2]) and np.array_equal(m["results"][0, 2], qv[3])
    vals = TM.to_ints(m["advice"])
    at = m["regions"][(0, 1)]["mask"]
    assert [vals[at + 8 * i + 7] for i in range(3)] == [TM.mask_value(P)] * 3


def test_library_exports_the_topk_entry_points():
    lib_path = os.path.join(ROOT, "halo2_vectordb_amd", "libvdb_hip.so")
    if not os.path.exists(lib_path):
        import __graft_entry__ as g
        g.build()
    lib = ctypes.CDLL(lib_path)
    names = ("vdb_wit_nearest_topk_size", "vdb_wit_nearest_topk", "vdb_wit_nearest_topk_dev")
    for name in names:
        assert hasattr(lib, name), name
    header = open(os.path.join(ROOT, "include", "vdb.h")).read()
    assert "VDB_NEAREST_TOPK_MAX_INSTANCES" in header and "int vdb_wit_nearest_topk_dev(" in header
    from halo2_vectordb_amd import _lib, api, pipeline
    assert all(name in _lib._SIGNATURES for name in names)
    assert callable(api.wit_nearest_topk) and hasattr(pipeline, "TopKQueryHotPath")
