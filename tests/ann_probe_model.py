"""The Python model of the query over the p nearest clusters that returns the t nearest candidates (include/vdb.h vdb_wit_ann_probe;
pipeline.AnnProbeQueryHotPath), composed of the models the single-probe query already stands on: topk_model.topk_model for the two
searches (at p and t rounds), ann_model._merkle / _mark_constants for the p + 1 trees and their shared zero cell,
topk_model.select_by_indicator for the p selections and the oracle's sponge.  At p = t = 1 it is ann_model.query_model cell for cell
(tests/test_ann_probe_cpu.py holds that first)."""
import numpy as np

import ann_model as AN
import topk_model as TM


def round_winners(indicator_bits):
    """the index a round's select_by_indicator states: the last set indicator of every round of (rounds, n) 0/1 bits"""
    return [int(np.flatnonzero(np.asarray(row))[-1]) for row in indicator_bits]


def centroid_rounds(O, metric, query, centroids, p, P, L):
    """the clusters p rounds of top-k over the centroids state, in round order"""
    a = TM.topk_model(O, metric, query[None], centroids, p, P, L, inputs=False)
    return round_winners(a["indicator_bits"][0])


def rounds_fold(table, p, P):
    """the winners of p rounds of top-k as values (api.nearest_topk_values), from `table` (q, n, 4) of distances: per round
    ann_assign_model.fold over what the earlier rounds left — the minimum of the qmin fold and the LAST entry at it — after which every
    entry equal to the minimum becomes M = 2^(2P) - 1.  -> (idx (q, p) uint32, dist (q, p, 4))"""
    import ann_assign_model as AS
    q, n = table.shape[0], table.shape[1]
    cur, M = table.copy(), TM.to_limbs([TM.mask_value(P)])[0]
    idx, dist = np.zeros((q, p), dtype=np.uint32), np.zeros((q, p, 4), dtype=np.uint64)
    for r in range(p):
        idx[:, r], dist[:, r] = AS.fold(cur, P)
        for j in range(q):
            cur[j][(cur[j] == dist[j, r]).all(axis=1)] = M
    return idx, dist


def probe_model(O, metric, query, centroids, members_list, cluster_roots, topk, P, L, plan_k=None):
    """the circuit on quantized query (dim, 4), centroids (K, dim, 4), members_list: the p probed clusters' rows (n_r, dim, 4) in round
    order, cluster_roots (K, 4) -> dict(advice, lookup, flags, selectors, break_points, n_in, centroid_indicators (p, K, 4),
    candidate_indicators (t, N, 4), results (t, dim, 4), public (t dim + 1, 4), regions, selected (p ints), members_roots (p ints),
    zero_cell, centroids_root, index_root)"""
    K, dim, p, t = centroids.shape[0], centroids.shape[1], len(members_list), topk
    cand = np.concatenate([np.asarray(m).reshape(-1, dim, 4) for m in members_list])
    N = cand.shape[0]
    s = TM._Stream()
    s.adv += [query.reshape(-1, 4), centroids.reshape(-1, 4), cand.reshape(-1, 4), cluster_roots.reshape(-1, 4)]
    n_in = dim + K * dim + N * dim + K
    s.sel.append(np.zeros(n_in, dtype=np.uint8))
    s.n = n_in
    reg = {"nearest_c": s.n}
    a = TM.topk_model(O, metric, query[None], centroids, p, P, L, inputs=False)
    s.adv.append(a["advice"]); s.sel.append(a["selectors"]); s.lk.append(a["lookup"]); s.n += a["advice"].shape[0]
    reg["merkle_c"] = s.n
    croot, loaded = AN._merkle(O, s, centroids, False)
    has_zero, zero_cell = loaded, (s.n - 1 - ((1 << (K - 1).bit_length()) - 1) * _node_cells() if loaded else None)
    reg["nearest_m"] = s.n
    b = TM.topk_model(O, metric, query[None], cand, t, P, L, inputs=False)
    s.adv.append(b["advice"]); s.sel.append(b["selectors"]); s.lk.append(b["lookup"]); s.n += b["advice"].shape[0]
    reg["merkle_m"], mroots, own_zero = [], [], []
    for m in members_list:
        reg["merkle_m"].append(s.n)
        mroot, loaded = AN._merkle(O, s, np.asarray(m), has_zero)
        own_zero.append(loaded)
        if loaded:
            zero_cell = s.n - 1 - ((1 << (len(m) - 1).bit_length()) - 1) * _node_cells()
        has_zero = has_zero or loaded
        mroots.append(TM.to_ints(mroot[None])[0])
    reg["select"], picked = [], []
    roots_int = TM.to_ints(cluster_roots)
    for r in range(p):
        reg["select"].append(s.n)
        cells, gates, out = TM.select_by_indicator(roots_int, TM.to_ints(a["indicators"][0, r]))
        s.ints(cells, gates)
        picked.append(out)
    reg["sponge"] = s.n
    words = np.concatenate([croot[None], cluster_roots])
    c = O.Ctx(store=True, keygen=True)
    index_root = c.merkle_commitment(words[None])
    assert c.err == 0
    s.adv.append(c.advice()); s.sel.append(c.selectors().astype(np.uint8)); s.n += len(c)
    advice, flags = np.concatenate(s.adv), np.concatenate(s.sel)
    lookup = np.concatenate([x for x in s.lk if x.shape[0]] or [np.zeros((0, 4), dtype=np.uint64)])
    assert advice.shape[0] == flags.shape[0] == s.n
    sel = flags & 1
    flags, vals = sel.copy(), TM.to_ints(advice)
    assert AN._mark_constants(flags, vals, reg["merkle_c"], dim, K, (1 << (K - 1).bit_length()) > K) == reg["nearest_m"]
    for r, m in enumerate(members_list):
        end = reg["merkle_m"][r + 1] if r + 1 < p else reg["select"][0]
        assert AN._mark_constants(flags, vals, reg["merkle_m"][r], dim, len(m), own_zero[r]) == end
    assert AN._mark_constants(flags, vals, reg["sponge"], K + 1) == s.n
    results = b["results"][0]
    return dict(advice=advice, lookup=lookup, flags=flags, selectors=sel, break_points=TM.row_walk(sel, plan_k) if plan_k is not None else None,
                n_in=n_in, centroid_indicators=a["indicators"][0], candidate_indicators=b["indicators"][0], results=results,
                public=np.concatenate([results.reshape(-1, 4), index_root[None]]), regions=reg, selected=picked, members_roots=mroots,
                zero_cell=zero_cell, centroids_root=croot, index_root=index_root,
                centroid_rounds=round_winners(a["indicator_bits"][0]), candidate_rounds=round_winners(b["indicator_bits"][0]))


def _node_cells():
    from halo2_vectordb_amd import circuit_sym as CS
    return CS.merkle_leaf_layout(1)["node_cells"]


# ---------------------------------------------------------------------------------------------------------------- the test shapes
P, L, DIM = 48, 12, 4
ZERO_CHAIN = (9, 4, [2, 0, 3, 1, 0, 3, 2, 0, 3])             # n, K, ids: K a power of two; the rounds probe sizes 2, 3, 3
# case -> (shape of tests/test_gpu_ann.py's SHAPES or "zero-chain", p, t, the clusters the rounds state, their sizes)
CASES = {
    "1-1": ("1-1", 2, 2, [0, 1], [1, 1]),                    # no padding anywhere, one-leaf trees, p = K, t = N
    "1-4-7": ("1-4-7", 2, 3, [2, 0], [7, 1]),                # the centroids' tree loads the zero cell, the 7-tree copies it
    "1-4-7 all": ("1-4-7", 3, 12, [2, 0, 1], [7, 1, 4]),     # every cluster probed, every candidate leaves
    "wave": ("wave", 2, 3, [4, 2], [65, 1]),                 # the candidates cross the 64-lane tile of k_nv_rounds / k_nv_select
    "zero-chain": ("zero-chain", 3, 4, [2, 0, 3], [2, 3, 3]),   # the first padded members' tree emits the zero cell, the next copies it
}
_cases = {}


def case(O, name):
    """the inputs of test case `name` with test_gpu_ann.py's seeds (db 40, centroids 41, query 42, Euclidean), what the table above says
    of them asserted: dict(f: the f64 rows, db, ids, cent, query, K, p, t, rounds, sizes, members (p arrays), roots (K, 4), ix)"""
    if name not in _cases:
        from test_gpu_ann import SHAPES, _rows
        shape, p, t, rounds, sizes = CASES[name]
        n, K, ids = ZERO_CHAIN if shape == "zero-chain" else SHAPES[shape]
        ids = np.asarray(ids)
        f = dict(db=_rows(40, n), cent=_rows(41, K), query=_rows(42, 1)[0])
        db, cent, query = O.quantize(f["db"], P), O.quantize(f["cent"], P), O.quantize(f["query"], P)
        assert centroid_rounds(O, "euclidean", query, cent, p, P, L) == rounds, name
        members = [AN.select_cluster(db, ids, c)[0] for c in rounds]
        assert [len(m) for m in members] == sizes, name
        assert AN.distances_distinct(O, "euclidean", query, cent, P, L) and AN.distances_distinct(O, "euclidean", query, np.concatenate(members), P, L)
        ix = AN.index_model(O, db, ids, cent)
        _cases[name] = dict(f=f, db=db, ids=ids, cent=cent, query=query, n=n, K=K, p=p, t=t, rounds=rounds, sizes=sizes, members=members,
                            roots=ix["roots"][1:1 + K], ix=ix)
    return _cases[name]


_models = {}


def case_model(O, name, plan_k=None):
    """probe_model of case `name`, computed once and shared (nobody changes it)"""
    if (name, plan_k) not in _models:
        c = case(O, name)
        _models[name, plan_k] = probe_model(O, "euclidean", c["query"], c["cent"], c["members"], c["roots"], c["t"], P, L, plan_k=plan_k)
    return _models[name, plan_k]
