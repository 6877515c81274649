"""Values-only nearest on the GPU (include/vdb.h vdb_nearest_values*, api.nearest_values, pipeline.AnnIndex.assign): the minimum of the
circuit's fixed-point distances and the last index at it are tests/ann_assign_model.py's bit for bit (tests/test_ann_assign_cpu.py holds
that model against the oracle's nearest_vector first), AnnIndex.assign answers as AnnIndex.probe does row by row, the launch count
depends on neither the number of queries nor the size of the database, and refused arguments launch nothing."""
import numpy as np
import pytest

import ann_assign_model as AM
from test_ann_assign_cpu import DIM, METRICS, L, P, pool
from topk_model import to_ints

pytestmark = pytest.mark.gpu
QS, NS = (1, 3, 65), (1, 2, 63, 64, 65, 130)      # one block and several; fewer lanes than a wave, one wave exactly, strides with a ragged tail


@pytest.fixture(scope="module")
def api():
    from halo2_vectordb_amd import api as a
    a.init(0)
    return a


@pytest.fixture(scope="module")
def tables(O):
    """per metric: the quantized 65 queries and 130 vectors and the model's 65 x 130 distances, computed once; a case over Q queries
    and n vectors is the table's corner [:Q, :n] (a distance does not depend on the rest of the database)"""
    queries, vectors = pool(21, max(QS), max(NS))
    qq, qv = O.quantize(queries, P), O.quantize(vectors, P)
    return {m: (qq, qv, AM.distance_table(O, m, qq, qv, P, L)) for m in METRICS}


@pytest.mark.parametrize("metric", METRICS)
def test_nearest_values_is_the_models(api, tables, metric):
    qq, qv, table = tables[metric]
    tied = 0
    for Q in QS:
        for n in NS:
            want_idx, want_dist = AM.fold(table[:Q, :n], P)
            idx, dist = api.nearest_values(metric, qq[:Q], qv[:n], P, L)
            assert np.array_equal(idx, want_idx), (Q, n, idx, want_idx)
            assert np.array_equal(dist, want_dist), (Q, n)
            tied += sum(sum(np.array_equal(table[j, i], want_dist[j]) for i in range(n)) > 1 for j in range(Q))
    assert tied > 0                                # the repeats of the longer databases tie; the model's rule (the last) was in question
    if metric == "cosine":                         # a doubled query lies a few units below zero, the rest above
        signs = [AM.is_neg(x, P) for x in to_ints(table[0])]
        assert any(signs) and not all(signs)
    # the raw 256-bit order of the (Montgomery) words is not the signed order: the raw minimum is another entry somewhere
    raw = [min(range(130), key=lambda i: tuple(int(w) for w in table[j, i][::-1])) for j in range(65)]
    assert any(not np.array_equal(table[j, raw[j]], AM.fold(table[j:j + 1], P)[1][0]) for j in range(65))


@pytest.mark.parametrize("metric", METRICS)
def test_minimum_at_either_end_and_three_ties_the_last_wins(api, O, metric):
    """the query itself planted in a database of rows that differ from it in every coordinate (no other row comes as near under any of
    the four metrics: at distance 0 under three of them, and the only parallel row under cosine): at index 0, at n - 1, and three
    times — the last copy in a higher lane than the others, then in a lower one (entries 7 and 40 against 67 = lane 3)"""
    query = np.array([[2.0, 3.0, 5.0]])
    others = np.random.default_rng(33).integers(6, 40, size=(130, DIM)).astype(np.float64)
    others[:, 0] += others[:, 1]                                     # never parallel to (2, 3, 5): first coordinate above the second
    qq = O.quantize(query, P)
    for n, planted in ((65, (0,)), (130, (0,)), (65, (64,)), (130, (129,)), (130, (5, 69, 100)), (130, (7, 40, 67)), (3, (0, 1, 2))):
        rows = others[:n].copy()
        rows[list(planted)] = query[0]
        qv = O.quantize(rows, P)
        want_idx, want_dist = AM.nearest_values_model(O, metric, qq, qv, P, L)
        assert int(want_idx[0]) == planted[-1], (n, planted)         # confirmed on the CPU before the GPU is asked
        idx, dist = api.nearest_values(metric, qq, qv, P, L)
        assert int(idx[0]) == planted[-1] and np.array_equal(dist, want_dist), (n, planted, idx)


def _index(O, metric):
    """five centroids on a grid and twelve members; the rows to route hold every centroid, midpoints of two centroids (exact ties under
    Euclidean and Manhattan: dyadic coordinates) and random rows"""
    from halo2_vectordb_amd.pipeline import AnnIndex
    cent = np.array([[1.0, 1.0, 1.0], [3.0, 1.0, 1.0], [1.0, 3.0, 1.0], [3.0, 3.0, 2.0], [2.0, 2.0, 4.0]])
    rng = np.random.default_rng(44)
    db = rng.integers(1, 5, size=(12, DIM)).astype(np.float64)
    ids = np.array([0, 1, 2, 3, 4, 0, 1, 2, 3, 4, 4, 4])
    rows = np.concatenate([cent, (cent[[0, 0, 1, 2]] + cent[[1, 2, 3, 3]]) / 2, rng.integers(1, 9, size=(8, DIM)) / 2.0])
    return AnnIndex(12, DIM, 5, db, ids, cent, P=P, L=L, metric=metric), cent, rows


@pytest.mark.parametrize("metric", ("euclidean", "manhattan", "cosine"))
def test_assign_is_probe_row_by_row_against_the_resident_centroids(api, O, metric):
    ix, cent, rows = _index(O, metric)
    try:
        got, dist = ix.assign(rows, distances=True)
        assert got.shape == (rows.shape[0],) and np.array_equal(got, ix.assign(rows))
        assert got.tolist() == [ix.probe(r) for r in rows]
        want_idx, want_dist = AM.nearest_values_model(O, metric, O.quantize(rows, P), O.quantize(cent, P), P, L)
        assert np.array_equal(got, want_idx) and np.array_equal(dist, want_dist)
        if metric != "cosine":                     # the midpoint of centroids 0 and 1 is tied between them: the last of the two
            assert got[:5].tolist() == [0, 1, 2, 3, 4] and got[5] == 1
        assert ix.assign(np.zeros((0, DIM))).shape == (0,)
    finally:
        ix.free()


def test_launch_count_depends_on_neither_Q_nor_n_and_refused_arguments_launch_nothing(api, tables):
    from halo2_vectordb_amd._lib import check
    lib = api.init()
    qq, qv, table = tables["euclidean"]
    bufs = [api.DeviceBuffer(x) for x in (qq.nbytes, qv.nbytes, 65 * 4, 65 * 32)]
    try:
        bufs[0].upload(qq)
        bufs[1].upload(qv)
        run = lambda Q, n, dim=DIM, dist=bufs[3].ptr: check(lib.vdb_nearest_values_dev(P, L, 0, bufs[0].ptr, bufs[1].ptr, Q, n, dim, bufs[2].ptr, dist))
        run(1, 2)                                                    # the chip's tables exist from here on
        counts = {}
        for Q, n in ((1, 2), (65, 130)):
            api.sync()
            api.profile_begin(deferred=True)
            run(Q, n)
            api.sync()
            counts[Q, n] = {name: int(v["launches"]) for name, v in api.profile_end().items()}
            want_idx, want_dist = AM.fold(table[:Q, :n], P)
            assert np.array_equal(bufs[2].download((Q,), dtype=np.uint32), want_idx) and np.array_equal(bufs[3].download((Q, 4)), want_dist)
        assert counts[1, 2] == counts[65, 130] == dict(k_dist_values=1, k_dist_tail_values=1, k_dist_head=1, k_dist_tail=1, k_nv_argmin=1), counts
        run(65, 130, dist=None)                                      # the distances are optional
        assert np.array_equal(bufs[2].download((65,), dtype=np.uint32), AM.fold(table, P)[0])
        api.sync()
        api.profile_begin(deferred=True)
        for Q, n, dim in ((0, 2, DIM), (1, 0, DIM), (1, 2, 0), ((1 << 24) + 1, 1, DIM), (3, 1 << 23, DIM), (3, 2, 1 << 23)):
            with pytest.raises(api.VdbError) as e:
                run(Q, n, dim)
            assert e.value.code == -3, (Q, n, dim)
        with pytest.raises(api.VdbError) as e:                       # the host-array form refuses before it uploads
            check(lib.vdb_nearest_values(P, L, 0, api._p(qq), api._p(qv), 0, 2, DIM, api._p(np.zeros(1, dtype=np.uint32)), None))
        assert e.value.code == -3
        with pytest.raises(api.VdbError) as e:
            check(lib.vdb_nearest_values_dev(P, L, 9, bufs[0].ptr, bufs[1].ptr, 1, 2, DIM, bufs[2].ptr, None))
        assert e.value.code == -3                                    # an unknown metric
        api.sync()
        assert api.profile_end() == {}
    finally:
        for b in bufs:
            b.free()
