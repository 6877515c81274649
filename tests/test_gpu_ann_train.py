"""Training the index on the GPU (include/vdb.h vdb_ann_assign_dev / vdb_ann_train_dev, api.ann_assign / ann_train, AnnIndex.train): the
fused assign is tests/ann_assign_model.py's bit for bit at the edges of its row tile, centroid chunk and dim chunk and the existing
entry point's wherever that one runs, it runs where n * K passes the old limit, a training run is the host loop over the existing entry
points bit for bit, and a converged index passes every routing and mean audit."""
import numpy as np
import pytest

import ann_assign_model as AM
from test_ann_assign_cpu import METRICS, L, P
from topk_model import to_ints

pytestmark = pytest.mark.gpu
CYC = 23                                             # centroid i >= 1 repeats centroid i + 23: ties inside a chunk of 64 and across chunks


@pytest.fixture(scope="module")
def api():
    from halo2_vectordb_amd import api as a
    a.init(0)
    return a


@pytest.fixture(scope="module")
def tiles(api):
    """(R, C) of the three tile shapes (C follows K) and DC, read from the plan"""
    plans = [api.ann_assign_plan("euclidean", 1 << 20, K, 1 << 12) for K in (2, 17, 1 << 20)]
    assert [p["C"] for p in plans] == [16, 32, 64]
    return [(p["R"], p["C"]) for p in plans], plans[0]["DC"]


def make(n, K, dim, seed=5):
    """f64 rows and centroids with coordinates in 1 .. 5: four distinct rows repeated; centroid 0 is row 0 and the last centroid row 1 (the
    minimum at either end), centroids 3 .. 6 the rows doubled (cosine: a few units below zero), centroid i >= 1 repeats every CYC"""
    rng = np.random.default_rng(seed + dim)
    base_r, base_c = rng.integers(1, 6, size=(4, dim)).astype(np.float64), rng.integers(1, 6, size=(CYC + 1, dim)).astype(np.float64)
    base_c[3:7] = 2.0 * base_r
    rows = base_r[np.arange(n) % 4]
    cents = base_c[1 + (np.arange(K) - 1) % CYC]
    cents[0], cents[K - 1] = base_r[0], base_r[1 % n]
    return rows, cents


def shapes(axis, tiles):
    (tile, DC), small = tiles, (2, 2, 3)
    if axis == "rows":
        return [(n, K, 3) for n in (1, 2) for K in (2,)] + [(n, K, 3) for K, (R, _) in zip((2, 17, 33), tile) for n in (R - 1, R, R + 1, 2 * R + 1)]
    if axis == "K":
        return [(2, K, 3) for _, C in tile for K in (C - 1, C, C + 1, 2 * C + 1)] + [(2, 1, 3), small]
    if axis == "dim":
        return [(2, 2, d) for d in (1, 3, DC - 1, DC + 1, 2 * DC + 1)]
    return [(2 * tile[2][0] + 1, 2 * tile[2][1] + 1, 2 * DC + 1)]


@pytest.mark.parametrize("axis", ("rows", "K", "dim", "large"))
@pytest.mark.parametrize("metric", METRICS)
def test_fused_assign_is_the_models(api, O, tiles, metric, axis):
    for n, K, dim in shapes(axis, tiles):
        rows, cents = make(n, K, dim)
        qr, qc = O.quantize(rows, P), O.quantize(cents, P)
        table = AM.distance_table(O, metric, qr, qc, P, L)
        want_idx, want_dist = AM.fold(table, P)
        idx, dist = api.ann_assign(metric, qr, qc, P, L)
        assert np.array_equal(idx, want_idx), (n, K, dim, idx, want_idx)
        assert np.array_equal(dist, want_dist), (n, K, dim)
    if axis == "large":                              # what the inputs must hold, on the model: (n, K, dim) = (33, 129, 33)
        C = tiles[0][2][1]
        if metric != "cosine":                       # (under cosine the doubled rows are as near as the rows themselves)
            assert int(want_idx[0]) == 0 and int(want_idx[1]) == K - 1
        at_min = [[i for i in range(K) if np.array_equal(table[j, i], want_dist[j])] for j in range(n)]
        assert any(len(m) > 1 and m[-1] // C == m[-2] // C for m in at_min) and any(len(m) > 1 and m[0] // C != m[-1] // C for m in at_min)
        if metric == "cosine":
            signs = [AM.is_neg(x, P) for x in to_ints(table[:4].reshape(-1, 4))]
            assert any(signs) and not all(signs)


def test_a_zero_row_under_cosine_is_the_existing_calls_domain_error(api, O):
    """a zero row meets a zero centroid: the product of the two roots quantizes to zero and qdiv's denominator with it (a zero row
    against non-zero centroids raises nothing in either call: qsqrt(0) is about 2^-25, and the product with a norm of a few units is
    not zero)"""
    rows, cents = make(5, 70, 3)
    rows[3], cents[3] = 0.0, 0.0
    codes = []
    for call in (api.nearest_values, api.ann_assign):
        with pytest.raises(api.VdbError) as e:
            call("cosine", O.quantize(rows, P), O.quantize(cents, P), P, L)
        codes.append(e.value.code)
    assert codes[0] == codes[1] == -5, codes         # VDB_ERR_DOMAIN


def _dev_calls(api, qr, qc):
    """-> (old, new, free): vdb_nearest_values_dev and vdb_ann_assign_dev over the uploaded rows and centroids -> (code, idx, dist)"""
    lib, (n, dim), K = api.init(), qr.shape[:2], qc.shape[0]
    bufs = [api.DeviceBuffer(b) for b in (qr.nbytes, qc.nbytes, n * 4, n * 32)]
    bufs[0].upload(qr)
    bufs[1].upload(qc)

    def run(fn, metric, n_=n, K_=K, dim_=dim):
        bufs[2].upload(np.full(n, 0xdeadbeef, dtype=np.uint32))
        code = fn(P, L, api.METRICS[metric], bufs[0].ptr, bufs[1].ptr, n_, K_, dim_, bufs[2].ptr, bufs[3].ptr)
        return code, bufs[2].download((n,), dtype=np.uint32), bufs[3].download((n, 4))
    return (lambda *a, **k: run(lib.vdb_nearest_values_dev, *a, **k)), (lambda *a, **k: run(lib.vdb_ann_assign_dev, *a, **k)), \
        (lambda: [b.free() for b in bufs])


@pytest.mark.parametrize("metric", METRICS)
def test_fused_assign_is_the_existing_entry_point_at_a_medium_shape(api, metric):
    rng = np.random.default_rng(77)
    qr, qc = api.quantize(rng.integers(1, 200, size=(1024, 128)) / 8.0, P), api.quantize(rng.integers(1, 200, size=(32, 128)) / 8.0, P)
    old, new, free = _dev_calls(api, qr, qc)
    try:
        (c0, i0, d0), (c1, i1, d1) = old(metric), new(metric)
        assert c0 == c1 == 0 and np.array_equal(i0, i1) and np.array_equal(d0, d1) and len(set(i0.tolist())) > 8
    finally:
        free()


@pytest.mark.parametrize("metric", ("manhattan", "euclidean"))
def test_beyond_the_old_limit_and_the_refusals(api, metric):
    n, K, dim = (1 << 17) + 1, 129, 2
    rng = np.random.default_rng(78)
    qr, qc = api.quantize(rng.integers(1, 64, size=(n, dim)) / 4.0, P), api.quantize(rng.integers(1, 64, size=(K, dim)) / 4.0, P)
    sample = np.sort(rng.choice(n, size=4096, replace=False))
    sample[-1] = n - 1                                               # the lone row of the last tile
    old, new, free = _dev_calls(api, qr, qc)
    try:
        code, idx, dist = new(metric)
        assert code == 0 and idx.max() < K
        assert old(metric)[0] == -3                                  # n * K just above 2^24: the existing entry still refuses
        for bad in (dict(n_=0), dict(K_=0), dict(dim_=0), dict(K_=(1 << 24) + 1), dict(dim_=(1 << 24) + 1), dict(n_=1 << 32)):
            code, untouched, _ = new(metric, **bad)
            assert code == -3 and (untouched == 0xdeadbeef).all(), bad
    finally:
        free()
    old, _, free = _dev_calls(api, qr[sample], qc)
    try:
        code, want_idx, want_dist = old(metric)
        assert code == 0 and np.array_equal(idx[sample], want_idx) and np.array_equal(dist[sample], want_dist)
    finally:
        free()


def host_train(api, metric, rows, cent, cap):
    """the loop of vdb_ann_train_dev over the existing entry points: nearest_values, numpy's grouping, ann_cluster_means (which refuses an
    empty cluster: those keep their centroid)"""
    cent, ids, run, K = cent.copy(), None, 0, cent.shape[0]
    while run < cap:
        new = api.nearest_values(metric, rows, cent, P, L)[0]
        if ids is not None and np.array_equal(new, ids):
            break
        ids, run = new, run + 1
        sizes = np.bincount(ids, minlength=K)
        live = np.flatnonzero(sizes)
        cent[live] = api.ann_cluster_means(rows[np.argsort(ids, kind="stable")], np.concatenate([[0], np.cumsum(sizes[live])]), P, L)
    return ids, cent, sizes, run


@pytest.mark.parametrize("cap", (1, 12))
@pytest.mark.parametrize("metric", ("euclidean", "cosine"))
@pytest.mark.parametrize("shape", ((40, 3, 3), (130, 5, 65)))
def test_train_is_the_host_loop_over_the_existing_entry_points(api, shape, metric, cap):
    n, K, dim = shape
    rows = api.quantize(np.random.default_rng(n).integers(1, 40, size=(n, dim)) / 2.0, P)
    want = host_train(api, metric, rows, rows[:K], cap)
    got = api.ann_train(metric, rows, rows[:K], cap, P, L)
    for g, w in zip(got, want):
        assert np.array_equal(g, w), (g, w)
    assert got[3] == cap if cap == 1 else 1 < got[3] <= cap


def test_an_empty_cluster_keeps_its_centroid_and_the_index_refuses_it(api):
    from halo2_vectordb_amd.pipeline import AnnIndex
    vec = np.random.default_rng(3).integers(1, 40, size=(40, 3)) / 2.0
    init = np.concatenate([vec[:2], [[900.0, 900.0, 900.0]]])
    rows, cent = api.quantize(vec, P), api.quantize(init, P)
    want = host_train(api, "euclidean", rows, cent, 12)
    got = api.ann_train("euclidean", rows, cent, 12, P, L)
    for g, w in zip(got, want):
        assert np.array_equal(g, w), (g, w)
    assert got[2][2] == 0 and np.array_equal(got[1][2], cent[2]) and got[3] < 12
    with pytest.raises(ValueError, match="cluster 2 "):
        AnnIndex.train(vec, 3, iterations=12, init=init, P=P, L=L)


def test_a_trained_index_passes_every_routing_and_mean_audit(api):
    from halo2_vectordb_amd.pipeline import AnnAuditHotPath, AnnIndex, AnnMeanHotPath
    from halo2_vectordb_amd.rounds import ProverRounds
    from test_gpu_rounds import TAU
    rng = np.random.default_rng(9)
    vec = np.concatenate([b + rng.integers(0, 5, size=(8, 3)) for b in ((2, 2, 2), (40, 4, 20), (6, 50, 30))]).astype(np.float64)
    vec = vec[rng.permutation(24)]
    ix = AnnIndex.train(vec, 3, iterations=32, P=P, L=L)
    try:
        assert ix.converged and 1 <= ix.iterations_run < 32 and ix.sizes.sum() == 24
        assert np.array_equal(ix.means(), ix.qcent) and np.array_equal(ix.assign(vec), ix.cluster_ids)
        for c in range(3):
            for cls in (AnnAuditHotPath, AnnMeanHotPath):
                hp, pr = cls(ix, c, k=13, P=P, L=L, tau=TAU), None
                try:
                    pr = ProverRounds(hp.setup()).keygen()
                    assert pr.keygen_report.violations() == 0, (cls.__name__, c, pr.keygen_report.as_dict())
                finally:
                    if pr is not None:
                        pr.free()
                    hp.free()
    finally:
        ix.free()
