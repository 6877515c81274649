"""The values model of nearest_values (tests/ann_assign_model.py) held against the oracle's own nearest_vector, before the GPU is
compared with the model (tests/test_gpu_ann_assign.py): the fold's minimum picks the vector nearest_vector returns, the index is its last
set indicator, under ties, with the minimum at either end, and where negative and positive fixed-point distances mix."""
import numpy as np
import pytest

import ann_assign_model as AM
from topk_model import to_ints

P, L, DIM = 48, 12, 3
METRICS = ("euclidean", "cosine", "manhattan", "hamming")


def pool(seed, n_q, n_v, distinct_q=4, distinct_v=40):
    """f64 rows with coordinates in 1 .. 5 (no zero vector: cosine divides by the norms; few values: Hamming finds equal elements and
    different rows sit at equal Euclidean and Manhattan distances): `n_q` queries drawn from `distinct_q` rows, `n_v` vectors of which the
    first `distinct_v` are distinct draws — among them every query row doubled, parallel to it: the cosine distance of such a pair is a
    few units below zero — and the rest repeat them, so that longer databases hold exact ties"""
    rng = np.random.default_rng(seed)
    q_rows = rng.integers(1, 6, size=(distinct_q, DIM)).astype(np.float64)
    v_rows = rng.integers(1, 6, size=(distinct_v, DIM)).astype(np.float64)
    v_rows[3:3 + distinct_q] = 2.0 * q_rows
    queries = q_rows[rng.integers(0, distinct_q, size=n_q)]
    queries[:min(n_q, distinct_q)] = q_rows[:n_q]
    vectors = np.concatenate([v_rows, v_rows[rng.integers(0, distinct_v, size=max(n_v - distinct_v, 0))]])[:n_v]
    return queries, vectors


def test_signed_order_is_not_the_raw_order():
    R = AM.R
    assert AM.is_neg(R - 5, P) and not AM.is_neg(5, P) and AM.signed(R - 5, P) == -5
    table = AM.to_limbs([7, R - 5, 3, R - 9, 3]).reshape(1, 5, 4)
    idx, dist = AM.fold(table, P)
    assert int(idx[0]) == 3 and to_ints(dist) == [R - 9]                      # -9 is the minimum, though it is the largest raw value
    idx, _ = AM.fold(AM.to_limbs([4, 3, 9, 3, 8, 3, 5]).reshape(1, 7, 4), P)
    assert int(idx[0]) == 5                                                   # three ties: the last


@pytest.mark.parametrize("metric", METRICS)
def test_values_model_is_nearest_vectors_answer(O, metric):
    queries, vectors = pool(11, 4, 48)
    qq, qv = O.quantize(queries, P), O.quantize(vectors, P)
    table = AM.distance_table(O, metric, qq, qv, P, L)
    idx, dist = AM.fold(table, P)
    for j in range(4):
        c = O.Ctx(store=False)
        ind, res = c.nearest_vector(metric, qq[j], qv, P=P, L=L)
        assert c.err == 0
        set_bits = np.flatnonzero(ind.any(axis=1))
        assert int(idx[j]) == int(set_bits[-1]) and np.array_equal(res, qv[idx[j]])
        assert all(np.array_equal(table[j, i], dist[j]) for i in set_bits)
    if metric == "cosine":     # a parallel vector's distance lies below zero, every other above: the fold must order them as signed values
        signs = [AM.is_neg(x, P) for x in to_ints(table[0])]
        assert any(signs) and not all(signs) and AM.is_neg(to_ints(dist)[0], P)
