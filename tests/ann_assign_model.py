"""The values model of nearest_values (api.nearest_values, AnnIndex.assign; include/vdb.h vdb_nearest_values): what nearest_vector ends
in, without its cells.

Per query: d_i = the oracle's `Ctx.distance(metric, vector_i, query)` (src/gadget/vectordb.rs:138's argument order), the minimum is the
serial fold m = qmin(m, d_i) of vectordb.rs:141-145 with qmin(a, b) = is_neg(a - b) ? a : b and is_neg(x) = x >= 2^(2P + 1) over the
canonical integer — the signed fixed-point order, in which a negative value is a field element just below the modulus — and the index
is the last i whose d_i equals that minimum, the last set indicator of nearest_vector's is_equal(min, d_i).  The model knows nothing of
the GPU's kernels: no wavefront, no reduction order.
"""
import numpy as np

from topk_model import R, to_ints, to_limbs  # noqa: F401 (the tests build tables with to_limbs)


def is_neg(x, P):
    return x % R >= 1 << (2 * P + 1)


def signed(x, P):
    """the fixed-point integer a field element stands for"""
    return x - R if is_neg(x, P) else x


def distance_table(O, metric, queries, vectors, P, L):
    """(q, n, 4): distance(vector_i, query_j) of the quantized `queries` (q, dim, 4) and `vectors` (n, dim, 4), one oracle call per
    distinct pair of rows (a distance is a function of its two operands alone; the oracle's square roots cost a millisecond each)"""
    q, n = queries.shape[0], vectors.shape[0]
    out = np.zeros((q, n, 4), dtype=np.uint64)
    c = O.Ctx(store=False)
    seen = {}
    for j in range(q):
        for i in range(n):
            key = (vectors[i].tobytes(), queries[j].tobytes())
            if key not in seen:
                seen[key] = c.distance(metric, vectors[i], queries[j], P=P, L=L)
            out[j, i] = seen[key]
    assert c.err == 0, "the reference would have panicked on these inputs"
    return out


def fold(table, P):
    """`table` (q, n, 4) of distances -> (idx (q,) uint32, dist (q, 4)): the qmin fold of every row and the last entry that equals it"""
    q, n = table.shape[0], table.shape[1]
    idx, dist = np.zeros(q, dtype=np.uint32), np.zeros((q, 4), dtype=np.uint64)
    for j in range(q):
        d = to_ints(table[j])
        m = d[0]
        for x in d[1:]:
            m = m if is_neg(m - x, P) else x
        last = max(i for i in range(n) if d[i] == m)
        idx[j], dist[j] = last, table[j, last]
    return idx, dist


def nearest_values_model(O, metric, queries, vectors, P, L):
    return fold(distance_table(O, metric, queries, vectors, P, L), P)
