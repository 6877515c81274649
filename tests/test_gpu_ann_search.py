"""The batch search on the GPU (include/vdb.h vdb_ann_search_dev / vdb_ann_search_probed_dev; api.ann_search, AnnIndex.search and
search_exact): the t nearest of every query are tests/ann_probe_model.rounds_fold's rounds bit for bit — a serial Python fold over
the oracle's distances that knows nothing of tiles, pieces or merges — for every tile shape, ragged chunk and piece split; exhausted
rounds state (M, last); the result is the existing entries' where they run; the index form states probe_many's clusters and the
rounds over each query's concatenated members; refused arguments launch nothing."""
import numpy as np
import pytest

import ann_assign_model as AM
from ann_probe_model import rounds_fold
from test_ann_assign_cpu import DIM, METRICS, L, P, pool
from test_gpu_ann_assign import _index
from topk_model import mask_value, to_limbs

pytestmark = pytest.mark.gpu
QMAX, NMAX = 17, 130


@pytest.fixture(scope="module")
def api():
    from halo2_vectordb_amd import api as a
    a.init(0)
    return a


@pytest.fixture(scope="module")
def tables(O):
    """per metric: the quantized 17 queries and 130 vectors and the model's 17 x 130 distances, computed once; a case over Q queries
    and n vectors is the corner [:Q, :n]"""
    queries, vectors = pool(21, QMAX, NMAX)
    qq, qv = O.quantize(queries, P), O.quantize(vectors, P)
    return {m: (qq, qv, AM.distance_table(O, m, qq, qv, P, L)) for m in METRICS}


@pytest.mark.parametrize("n", (1, 2, 16, 17, 63, 64, 65, 130))     # C = 16, 32, 64; ragged chunks; at span 48 several pieces, the last ragged
@pytest.mark.parametrize("Q", (1, QMAX))                            # one ragged tile; two tiles at R = 16
@pytest.mark.parametrize("metric", METRICS)
def test_dense_search_is_the_rounds_of_the_fold(api, tables, metric, Q, n):
    qq, qv, table = tables[metric]
    if n == NMAX:                                                   # ties: the last-index rule is exercised
        assert all(len({table[j, i].tobytes() for i in range(n)}) < n for j in range(Q))
    tmax = min(n, 64)
    want_idx, want_dist = rounds_fold(table[:Q, :n], tmax, P)       # the rounds of a smaller t are its first t
    for t in sorted({1, min(2, n), min(5, n), tmax}):
        for span in (0, 48):
            idx, dist = api.ann_search(metric, qq[:Q], qv[:n], t, P, L, span=span)
            assert np.array_equal(idx, want_idx[:, :t]), (t, span, idx, want_idx[:, :t])
            assert np.array_equal(dist, want_dist[:, :t]), (t, span)


def test_exhausted_classes_state_the_mask_and_the_last_index(api, O):
    M = to_limbs([mask_value(P)])[0]
    query = O.quantize(np.array([[2.0, 3.0, 5.0]]), P)
    three = np.array([[1.0, 1.0, 2.0], [4.0, 1.0, 1.0], [2.0, 5.0, 3.0]])
    for rows, t in ((np.repeat(three[:1], 5, axis=0), 3), (three[np.arange(130) % 3], 5)):
        qv = O.quantize(rows, P)
        want_idx, want_dist = rounds_fold(AM.distance_table(O, "euclidean", query, qv, P, L), t, P)
        n, classes = rows.shape[0], min(3, len({r.tobytes() for r in rows}))
        assert all(np.array_equal(want_dist[0, r], M) and want_idx[0, r] == n - 1 for r in range(classes, t))     # held on the CPU first
        assert sorted(want_idx[0, :classes].tolist()) == list(range(n - classes, n))
        for span in (0, 16):
            idx, dist = api.ann_search("euclidean", query, qv, t, P, L, span=span)
            assert np.array_equal(idx, want_idx) and np.array_equal(dist, want_dist), (n, span, idx)


@pytest.mark.parametrize("metric", ("euclidean", "cosine"))
def test_ragged_dim_chunk(api, O, metric):
    rng = np.random.default_rng(17)
    qq, qv = (O.quantize(rng.integers(1, 6, size=(m, 17)).astype(np.float64), P) for m in (2, 20))
    want = rounds_fold(AM.distance_table(O, metric, qq, qv, P, L), 4, P)
    got = api.ann_search(metric, qq, qv, 4, P, L)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


@pytest.mark.parametrize("metric", METRICS)
def test_agrees_with_the_existing_entries(api, tables, metric):
    qq, qv, _ = tables[metric]
    for got, want in ((api.ann_search(metric, qq, qv, 1, P, L), api.ann_assign(metric, qq, qv, P, L)),
                      (api.ann_search(metric, qq, qv[:65], 7, P, L, span=32), api.nearest_topk_values(metric, qq, qv[:65], 7, P, L))):
        assert np.array_equal(got[0].reshape(want[0].shape), want[0]) and np.array_equal(got[1].reshape(want[1].shape), want[1])


@pytest.mark.parametrize("metric", ("euclidean", "manhattan", "cosine"))
def test_index_search_is_probe_many_and_the_rounds_over_the_probed_members(api, O, metric):
    ix, cent, rows = _index(O, metric)                              # its rows hold every centroid and midpoints of two
    try:
        queries = rows[[0, 3, 5, 6, 8, 9, 12, 16]]
        qq = O.quantize(queries, P)
        got = ix.search(queries, probes=2, topk=3)
        want_cl, _ = rounds_fold(AM.distance_table(O, metric, qq, O.quantize(cent, P), P, L), 2, P)
        assert np.array_equal(got["clusters"], want_cl)
        assert all(got["clusters"][j].tolist() == ix.probe_many(q, 2).tolist() for j, q in enumerate(queries))
        slots = ix.d_slots.download((ix.n,), dtype=np.uint32)
        for j in range(len(queries)):
            members = np.concatenate([ix.members(int(c)) for c in want_cl[j]])
            place = np.concatenate([np.arange(ix.offsets[c], ix.offsets[c + 1]) for c in want_cl[j]])
            want_idx, want_dist = rounds_fold(AM.distance_table(O, metric, qq[j:j + 1], members, P, L), 3, P)
            assert np.array_equal(got["candidates"][j], want_idx[0]) and np.array_equal(got["dist"][j], want_dist[0]), j
            assert np.array_equal(got["slots"][j], slots[place[want_idx[0]]])
        grouped = ix.d_grouped.download((ix.n, DIM, 4))
        exact_slots, exact_dist = ix.search_exact(queries, 3)
        want_idx, want_dist = rounds_fold(AM.distance_table(O, metric, qq, grouped, P, L), 3, P)
        assert np.array_equal(exact_dist, want_dist) and np.array_equal(exact_slots, slots[want_idx])
        with pytest.raises(ValueError, match="query 1: fewer than"):
            ix.search(rows[[4, 0]], probes=1, topk=3)                # centroid 4's cluster holds four members, centroid 0's two
    finally:
        ix.free()


@pytest.mark.parametrize("metric", ("euclidean", "manhattan"))
def test_a_query_equidistant_from_every_centroid_is_refused(api, metric):
    from halo2_vectordb_amd.pipeline import AnnIndex
    cent = np.array([[5.0, 3.0, 3.0], [1.0, 3.0, 3.0], [3.0, 5.0, 3.0], [3.0, 1.0, 3.0], [3.0, 3.0, 5.0]])
    ix = AnnIndex(10, DIM, 5, np.concatenate([cent, cent + 0.5]), np.arange(10) % 5, cent, P=P, L=L, metric=metric)
    try:
        assert ix.search(cent[:2], probes=2, topk=2)["clusters"][:, 0].tolist() == [0, 1]
        with pytest.raises(ValueError, match="query 2: the clusters probed are not pairwise distinct"):
            ix.search(np.concatenate([cent[:2], [[3.0, 3.0, 3.0]]]), probes=2, topk=2)
    finally:
        ix.free()


def test_refused_arguments_launch_nothing_and_a_zero_pair_is_a_domain_error(api, tables):
    from halo2_vectordb_amd._lib import check
    lib = api.init()
    qq, qv, table = tables["euclidean"]
    bufs = [api.DeviceBuffer(x) for x in (qq.nbytes, qv.nbytes, QMAX * 64 * 4, QMAX * 64 * 32)]
    try:
        bufs[0].upload(qq)
        bufs[1].upload(qv)
        run = lambda Q, n, dim, t: check(lib.vdb_ann_search_dev(P, L, 0, bufs[0].ptr, bufs[1].ptr, Q, n, dim, t, 0, bufs[2].ptr, bufs[3].ptr))
        run(QMAX, NMAX, DIM, 2)                                      # the chip's tables exist from here on
        assert np.array_equal(bufs[2].download((QMAX, 2), dtype=np.uint32), rounds_fold(table, 2, P)[0])
        api.sync()
        api.profile_begin(deferred=True)
        for Q, n, dim, t in ((3, 9, DIM, 0), (3, 100, DIM, 65), (3, 9, DIM, 10), (0, 9, DIM, 1), (3, 0, DIM, 1), (3, 9, 0, 1)):
            with pytest.raises(api.VdbError) as e:
                run(Q, n, dim, t)
            assert e.value.code == -3, (Q, n, dim, t)
        api.sync()
        assert api.profile_end() == {}
    finally:
        for b in bufs:
            b.free()
    zero = np.zeros_like(qq[:2])
    with pytest.raises(api.VdbError) as e:                           # a zero query against a zero vector under cosine
        api.ann_search("cosine", np.concatenate([qq[:1], zero[:1]]), np.concatenate([qv[:4], zero[:1]]), 1, P, L)
    assert e.value.code == -5                                        # VDB_ERR_DOMAIN, as vdb_ann_assign_dev reports it
