"""The Python model of the approximate-nearest-neighbour index and of the query circuit (include/vdb.h vdb_ann_index_build_dev,
vdb_wit_ann_query), in the manner of topk_model.py: oracle contexts for distance, qmin and merkle_commitment (the sponge over K + 1 words is
Ctx.merkle_commitment of one vector), topk_model's integer templates for is_equal and select_by_indicator and its row walk for the break
points.  The index is built cluster by cluster: select_cluster, then poseidon_merkle_root."""
import numpy as np

import merkle_update_model as MU
import topk_model as TM


def select_cluster(db, ids, c):
    """the rows of `db` whose cluster id is c, in database order, and their slots"""
    slots = np.flatnonzero(np.asarray(ids) == c)
    return np.ascontiguousarray(db[slots]), slots


def index_model(O, db, ids, centroids):
    """dict(grouped, slots, offsets (K + 1), roots (K + 2, 4): [centroids' root | cluster roots | index root], forest: the K + 1 trees,
    each (2 lp, 4) in vdb_merkle_tree_build_dev's layout, the centroids' last)"""
    K = centroids.shape[0]
    parts = [select_cluster(db, ids, c) for c in range(K)]
    assert all(len(s) for _, s in parts), "an empty cluster has no commitment"
    roots = [O.poseidon_merkle_root(centroids)] + [O.poseidon_merkle_root(m) for m, _ in parts]
    words = np.stack(roots)
    roots.append(O.poseidon_merkle_root(words[None]))            # the leaf hash of one vector of K + 1 words
    forest = [MU.flat_levels(MU.build_tree(O, m)) for m, _ in parts] + [MU.flat_levels(MU.build_tree(O, centroids))]
    return dict(grouped=np.concatenate([m for m, _ in parts]), slots=np.concatenate([s for _, s in parts]).astype(np.uint32),
                offsets=np.concatenate([[0], np.cumsum([len(s) for _, s in parts])]).astype(np.uint64), roots=np.stack(roots), forest=forest)


def distances_distinct(O, metric, query, vectors, P, L):
    """the fixed-point distances of `vectors` to `query` are pairwise distinct"""
    c = O.Ctx(store=False, keygen=False)
    d = TM.to_ints(np.stack([c.distance(metric, v, query, P=P, L=L) for v in vectors]))
    return len(set(d)) == len(d)


def _merkle(O, s, vectors, has_zero):
    """merkle_commitment(vectors) appended to the stream; Context::load_zero caches its cell: when an earlier block of the circuit has
    loaded it, the padding's zero cell (right behind the leaves' sponges) is not emitted again.  -> (root, the trace loaded the zero cell)"""
    n = vectors.shape[0]
    c = O.Ctx(store=True, keygen=True)
    root = c.merkle_commitment(vectors)
    assert c.err == 0
    adv, flags = c.advice(), c.selectors().astype(np.uint8)
    padded = (1 << (n - 1).bit_length()) > n
    if padded and has_zero:
        lp = 1 << (n - 1).bit_length()
        node = 2 * 2238 + 18 + 12
        z = adv.shape[0] - 1 - (lp - 1) * node
        assert not adv[z].any() and not (flags[z] & 1)
        adv, flags = np.delete(adv, z, axis=0), np.delete(flags, z)
    s.adv.append(adv)
    s.sel.append(flags)
    s.n += adv.shape[0]
    return root, padded and not has_zero


def _mark_constants(flags, vals, at, words, n=1, has_zero_cell=False):
    """the constant bit the kernels write on the constant cells of every permutation of merkle_commitment over n vectors of `words` words
    whose trace starts at cell `at` (the oracle keeps no constant bit; the method of test_merkle_update_cpu.kernel_like_flags)"""
    from halo2_vectordb_amd import circuit_sym as CS, copymap as CM
    lay = CS.merkle_leaf_layout(words)

    def mark(at, n_in):
        t = CM._Tracer(None)
        t.next_is_const = lambda: vals[at + len(t.src)] == 0 and vals[at + len(t.src) + 3] == vals[at + len(t.src) + 1] * vals[at + len(t.src) + 2] % CS.R
        CM._trace_permutation(t, n_in)
        size = CM.perm_cells(n_in)
        assert len(t.src) == size and np.array_equal(np.asarray(t.gate, dtype=np.uint8), flags[at:at + size] & 1)
        flags[at:at + size] |= np.asarray(t.cst, dtype=np.uint8) << 1
        return at + size

    for _ in range(n):
        for n_in in lay["n_ins"]:
            at = mark(at, n_in)
    lp = 1 << (n - 1).bit_length()
    if has_zero_cell:
        flags[at] |= 2
        at += 1
    for _ in range(lp - 1):
        at = mark(mark(at, 2), 0)
    return at


def query_model(O, metric, query, centroids, members, cluster_roots, P, L, plan_k=None):
    """the circuit on quantized query (dim, 4), centroids (K, dim, 4), members (n_c, dim, 4), cluster_roots (K, 4) -> dict(advice, lookup,
    flags, selectors, break_points, n_in, centroid_indicator, member_indicator, result, public (dim + 1, 4), regions, selected, members_root)"""
    K, dim, n_c = centroids.shape[0], centroids.shape[1], members.shape[0]
    s = TM._Stream()
    s.adv += [query.reshape(-1, 4), centroids.reshape(-1, 4), members.reshape(-1, 4), cluster_roots.reshape(-1, 4)]
    n_in = dim + K * dim + n_c * dim + K
    s.sel.append(np.zeros(n_in, dtype=np.uint8))
    s.n = n_in
    reg = {"nearest_c": s.n}
    a = TM.topk_model(O, metric, query[None], centroids, 1, P, L, inputs=False)
    s.adv.append(a["advice"]); s.sel.append(a["selectors"]); s.lk.append(a["lookup"]); s.n += a["advice"].shape[0]
    reg["merkle_c"] = s.n
    croot, zero = _merkle(O, s, centroids, False)
    reg["nearest_m"] = s.n
    b = TM.topk_model(O, metric, query[None], members, 1, P, L, inputs=False)
    s.adv.append(b["advice"]); s.sel.append(b["selectors"]); s.lk.append(b["lookup"]); s.n += b["advice"].shape[0]
    reg["merkle_m"] = s.n
    mroot, _ = _merkle(O, s, members, zero)
    reg["select"] = s.n
    ind_c = TM.to_ints(a["indicators"][0, 0])
    cells, gates, picked = TM.select_by_indicator(TM.to_ints(cluster_roots), ind_c)
    s.ints(cells, gates)
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
    pad_c, pad_m = (1 << (K - 1).bit_length()) > K, (1 << (n_c - 1).bit_length()) > n_c
    assert _mark_constants(flags, vals, reg["merkle_c"], dim, K, pad_c) == reg["nearest_m"]
    assert _mark_constants(flags, vals, reg["merkle_m"], dim, n_c, pad_m and not pad_c) == reg["select"]
    assert _mark_constants(flags, vals, reg["sponge"], K + 1) == s.n
    return dict(advice=advice, lookup=lookup, flags=flags, selectors=sel, break_points=TM.row_walk(sel, plan_k) if plan_k is not None else None,
                n_in=n_in, centroid_indicator=a["indicators"][0, 0], member_indicator=b["indicators"][0, 0], result=b["results"][0, 0],
                public=np.concatenate([b["results"][0, 0], index_root[None]]), regions=reg, selected=picked, members_root=TM.to_ints(mroot[None])[0],
                centroids_root=croot, index_root=index_root)
