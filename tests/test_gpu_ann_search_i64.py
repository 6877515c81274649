"""The batch search over packed rows on the GPU (include/vdb.h vdb_fp_pack_i64_dev, vdb_ann_search_i64_dev,
vdb_ann_search_probed_i64_dev; api.pack_i64, api.ann_search(packed=True), AnnIndex.search / search_exact (packed=True)): a field word
packs to its signed value or is refused; over signed, fractional rows the packed search states tests/ann_probe_model.rounds_fold's
rounds over the oracle's distances bit for bit, and the field form's; at words of 62 to 63 bits and at other P it states the field
form's; the index form agrees key by key; refused arguments launch nothing."""
import numpy as np
import pytest

import ann_assign_model as AM
from ann_probe_model import rounds_fold
from test_ann_assign_cpu import DIM, METRICS, L, P
from test_gpu_ann_assign import _index
from topk_model import R, to_ints, to_limbs

pytestmark = pytest.mark.gpu
QMAX, NMAX, TOP = 17, 130, (1 << 63) - 1


@pytest.fixture(scope="module")
def api():
    from halo2_vectordb_amd import api as a
    a.init(0)
    return a


@pytest.fixture(scope="module")
def tables(O):
    """(metric, dim) -> the quantized 17 queries and 130 vectors and the model's 17 x 130 distances, computed once each: signed rows with
    thirds (a product's low P bits are not zero, and it may be negative), 3 distinct queries and 12 distinct vectors repeated (ties)"""
    cache = {}

    def get(metric, dim):
        if (metric, dim) not in cache:
            rng = np.random.default_rng(dim)
            q, v = (rng.integers(-5, 6, size=(m, dim)) + rng.integers(0, 3, size=(m, dim)) / 3 for m in (3, 12))
            q[~q.any(axis=1)] = v[~v.any(axis=1)] = 1.0             # no zero row: cosine divides by the norms
            qq, qv = O.quantize(q[np.arange(QMAX) % 3], P), O.quantize(v[np.arange(NMAX) % 12], P)
            cache[metric, dim] = (qq, qv, AM.distance_table(O, metric, qq, qv, P, L))
            terms = [AM.signed(a, P) * AM.signed(b, P) for i in range(12) for a, b in zip(to_ints(qv[i]), to_ints(qq[0]))]
            assert any(p < 0 and p % (1 << P) for p in terms), "no negative product with low bits: the floor would go untested"
        return cache[metric, dim]
    return get


def test_pack_states_the_signed_value(api, O):
    vals = [0, 1, -1, TOP, -TOP] + [AM.signed(x, P) for x in to_ints(O.quantize(np.array([[-2.5, 1 / 3, -1e3 / 7, 30000.25]]), P))]
    assert api.pack_i64(to_limbs(vals)).tolist() == vals


@pytest.mark.parametrize("word", (1 << 63, R - (1 << 63), R // 2))
def test_a_word_outside_the_domain_is_refused(api, word):
    with pytest.raises(api.VdbError) as e:
        api.pack_i64(to_limbs([5, word, -5]))
    assert e.value.code == -5


@pytest.mark.parametrize("Q,n", ((1, 1), (1, 17), (QMAX, 65), (QMAX, NMAX)))   # C = 16, 32, 64; ragged chunks; two tiles
@pytest.mark.parametrize("dim", (3, 64, 65, 130))                                  # under a chunk, one, ragged, three with a ragged last
@pytest.mark.parametrize("metric", METRICS)
def test_dense_search_is_the_rounds_of_the_fold_and_the_field_form(api, tables, metric, dim, Q, n):
    qq, qv, table = tables(metric, dim)
    if n > 12:                                                       # ties: the last-index rule is exercised
        assert len({table[0, i].tobytes() for i in range(n)}) < n
    tmax = min(n, 64)
    want_idx, want_dist = rounds_fold(table[:Q, :n], tmax, P)
    for t in sorted({1, min(5, n), tmax}):
        for span in (0, 48):
            idx, dist = api.ann_search(metric, qq[:Q], qv[:n], t, P, L, span=span, packed=True)
            assert np.array_equal(idx, want_idx[:, :t]) and np.array_equal(dist, want_dist[:, :t]), (t, span, idx, want_idx[:, :t])
        field = api.ann_search(metric, qq[:Q], qv[:n], t, P, L, packed=False)
        assert np.array_equal(idx, field[0]) and np.array_equal(dist, field[1]), t


@pytest.mark.parametrize("dim", (3, 65))
@pytest.mark.parametrize("prec", (32, 48, 63))
@pytest.mark.parametrize("metric", ("euclidean", "cosine", "manhattan"))
def test_wide_words_state_the_field_form(api, metric, prec, dim):
    """coordinates of 62 to 63 bits, the first pair at opposite extremes (|x - y| = 2^64 - 2): the carries of the 128-bit products, sums
    and shifts.  Both forms run one tail on one head sum, so a difference is the head's."""
    rng = np.random.default_rng(prec + dim)
    wide = lambda m: [[int(s) * int(v) for s, v in zip(rng.choice((-1, 1), dim), rng.integers(1 << 62, TOP, size=dim, endpoint=True))] for _ in range(m)]
    q, v = wide(3), wide(20)
    q[0], v[0] = [TOP] * dim, [-TOP] * dim
    qq, qv = (np.stack([to_limbs(row) for row in rows]) for rows in (q, v))
    got, want = (api.ann_search(metric, qq, qv, 5, prec, L, span=16, packed=k) for k in (True, False))
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


@pytest.mark.parametrize("metric", ("euclidean", "manhattan", "cosine"))
def test_index_search_agrees_key_by_key(api, O, metric):
    ix, _, rows = _index(O, metric)
    try:
        queries = rows[[0, 3, 5, 6, 8, 9, 12, 16]]
        got, want = ix.search(queries, probes=2, topk=3, packed=True), ix.search(queries, probes=2, topk=3)
        assert sorted(got) == sorted(want) and all(np.array_equal(got[k], want[k]) for k in want)
        got, want = ix.search_exact(queries, 3, packed=True), ix.search_exact(queries, 3)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
        assert ix.d_packed is ix._packed()                           # the packed copy is made once
    finally:
        ix.free()


def test_refused_arguments_launch_nothing_and_domain_errors(api, tables):
    from halo2_vectordb_amd._lib import check
    from halo2_vectordb_amd.pipeline import AnnIndex
    lib = api.init()
    qq, qv, table = tables("euclidean", DIM)
    bufs = [api.DeviceBuffer(x) for x in (qq.nbytes, qv.nbytes, QMAX * DIM * 8, NMAX * DIM * 8, QMAX * 64 * 4, QMAX * 64 * 32)]
    try:
        bufs[0].upload(qq)
        bufs[1].upload(qv)
        api.pack_i64_dev(bufs[0], QMAX * DIM, bufs[2])
        api.pack_i64_dev(bufs[1], NMAX * DIM, bufs[3])
        run = lambda Q, n, dim, t: check(lib.vdb_ann_search_i64_dev(P, L, 0, bufs[2].ptr, bufs[3].ptr, Q, n, dim, t, 0, bufs[4].ptr, bufs[5].ptr))
        run(QMAX, NMAX, DIM, 2)                                      # the chip's tables exist from here on
        assert np.array_equal(bufs[4].download((QMAX, 2), dtype=np.uint32), rounds_fold(table, 2, P)[0])
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
    zero = np.zeros_like(qq[:1])
    with pytest.raises(api.VdbError) as e:                           # a zero query against a zero vector under cosine
        api.ann_search("cosine", np.concatenate([qq[:1], zero]), np.concatenate([qv[:4], zero]), 1, P, L, packed=True)
    assert e.value.code == -5
    cent = np.array([[1.0, 1.0, 1.0], [3.0, 1.0, 70000.0]])          # 70000 2^48 is above 2^63
    ix = AnnIndex(2, DIM, 2, cent, np.arange(2), cent, P=P, L=L)
    try:
        with pytest.raises(ValueError, match="not packable"):
            ix.search(cent[:1], packed=True)
    finally:
        ix.free()
