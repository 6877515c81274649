"""The approximate-nearest-neighbour query circuit without a GPU: tests/ann_model.py held against the oracle's own cells, the model's
index roots against Ctx.merkle_commitment of each cluster, circuit_sym.build_ann_query on the host builder against the model (cell counts,
the sel = mroot tie, the public cells, a wrong cluster noticed), and build_nearest_topk's shapes through place_nearest."""
import numpy as np
import pytest

import ann_model as AN
import topk_model as TM
from halo2_vectordb_amd import circuit_sym as CS
from test_merkle_update_cpu import fetchers

P, L = 48, 12
IDS = [2, 0, 1, 2, 2, 1, 2, 0, 2, 1, 2, 2]                 # cluster sizes 2, 3, 7


def _setup(O, seed=5, n=12, dim=4, K=3, ids=IDS):
    rng = np.random.default_rng(seed)
    db = O.quantize(rng.integers(0, 219, size=(n, dim)).astype(np.float64), P)
    cent = O.quantize(rng.integers(0, 219, size=(K, dim)).astype(np.float64), P)
    query = O.quantize(rng.integers(0, 219, size=(dim,)).astype(np.float64), P)
    return db, np.asarray(ids), cent, query


def _winner(O, query, cent):
    a = TM.topk_model(O, "euclidean", query[None], cent, 1, P, L, inputs=False)
    return int(np.flatnonzero(a["indicators"][0, 0].any(axis=1))[-1])


def test_index_roots_are_the_commitments_of_each_cluster(O):
    db, ids, cent, _ = _setup(O)
    ix = AN.index_model(O, db, ids, cent)
    c = O.Ctx(store=True, keygen=True)
    assert np.array_equal(ix["roots"][0], c.merkle_commitment(cent))
    for k in range(3):
        members, slots = AN.select_cluster(db, ids, k)
        assert list(slots) == [i for i, x in enumerate(IDS) if x == k]
        assert np.array_equal(ix["roots"][1 + k], O.Ctx(store=True, keygen=True).merkle_commitment(members))
        assert np.array_equal(ix["forest"][k][2 * (1 << (len(slots) - 1).bit_length()) - 2], ix["roots"][1 + k])
    assert np.array_equal(ix["roots"][4], O.Ctx(store=True, keygen=True).merkle_commitment(ix["roots"][:4][None]))
    assert np.array_equal(ix["grouped"][:2], db[[1, 7]]) and list(ix["offsets"]) == [0, 2, 5, 12]


def test_model_parts_are_the_oracles_cells(O):
    """the two searches are the oracle's nearest_vector cell for cell; the selection is its select_by_indicator"""
    db, ids, cent, query = _setup(O)
    ix = AN.index_model(O, db, ids, cent)
    w = _winner(O, query, cent)
    members, _ = AN.select_cluster(db, ids, w)
    m = AN.query_model(O, "euclidean", query, cent, members, ix["roots"][1:4], P, L, plan_k=13)
    r = m["regions"]
    for vectors, lo, hi, ind in ((cent, r["nearest_c"], r["merkle_c"], "centroid_indicator"), (members, r["nearest_m"], r["merkle_m"], "member_indicator")):
        c = O.Ctx(store=True, keygen=True)
        oind, ores = c.nearest_vector("euclidean", query, vectors, P=P, L=L)
        assert np.array_equal(c.advice(), m["advice"][lo:hi]) and np.array_equal(c.selectors().astype(np.uint8) & 1, m["selectors"][lo:hi])
        assert np.array_equal(oind, m[ind])
    assert np.array_equal(ores, m["result"])
    assert m["selected"] == m["members_root"] == TM.to_ints(ix["roots"][1 + w][None])[0]
    assert np.array_equal(m["public"][-1], ix["roots"][-1])
    assert AN.distances_distinct(O, "euclidean", query, cent, P, L) and AN.distances_distinct(O, "euclidean", query, members, P, L)


@pytest.mark.parametrize("K,n,ids", [(3, 12, IDS), (2, 2, [1, 0]), (1, 5, [0] * 5), (4, 6, [0, 1, 2, 3, 3, 3])])
def test_map_counts_tie_and_public_cells(O, K, n, ids):
    db, ids, cent, query = _setup(O, seed=9 + K, n=n, K=K, ids=ids)
    ix = AN.index_model(O, db, ids, cent)
    w = _winner(O, query, cent)
    members, _ = AN.select_cluster(db, ids, w)
    m = AN.query_model(O, "euclidean", query, cent, members, ix["roots"][1:1 + K], P, L)
    ff, fv, vals = fetchers(m)
    cm, public, info = CS.build_ann_query("euclidean", K, members.shape[0], 4, P, L, ff, fv)
    lay = info["layout"]
    assert cm.n_cells == m["advice"].shape[0] == lay["total"] and len(cm.lookup_src) == m["lookup"].shape[0] and lay["n_in"] == m["n_in"]
    assert {k: lay[k] for k in m["regions"]} == m["regions"]
    assert cm.copy_of[info["selected"]] == info["members_root"] < info["selected"] == lay["sponge"] - 1
    rep = cm.check_witness(vals, TM.to_ints(m["lookup"]), m["flags"])
    assert not any(rep.values()), rep
    assert [vals[c] for c in public] == TM.to_ints(m["public"]) and len(public) == 5
    assert np.array_equal(np.asarray(cm.gate), m["selectors"].astype(bool))
    # the sponge absorbs the centroids' root and the assigned cluster roots; its words are copies of those cells
    words = np.flatnonzero((cm.copy_of == info["centroids_root"]) & (np.arange(cm.n_cells) >= lay["sponge"]))
    assert len(words) == 1
    for k in range(K):
        assert ((cm.copy_of == lay["roots"] + k) & (np.arange(cm.n_cells) >= lay["sponge"])).sum() == 1


@pytest.mark.parametrize("K,n,ids", [(3, 12, IDS), (2, 2, [1, 0]), (1, 5, [0] * 5), (4, 6, [0, 1, 2, 3, 3, 3])])
def test_map_is_the_probe_maps_at_one_cluster_and_one_neighbour(O, K, n, ids):
    """build_ann_query is a view of build_ann_probe at sizes = [n_c], p = t = 1: the same map and public cells, the info without the round axes"""
    db, ids, cent, query = _setup(O, seed=9 + K, n=n, K=K, ids=ids)
    members, _ = AN.select_cluster(db, ids, _winner(O, query, cent))
    n_c = members.shape[0]
    m = AN.query_model(O, "euclidean", query, cent, members, AN.index_model(O, db, ids, cent)["roots"][1:1 + K], P, L)
    ff, fv, _ = fetchers(m)
    cm, public, info = CS.build_ann_query("euclidean", K, n_c, 4, P, L, ff, fv)
    pm, ppublic, pinfo = CS.build_ann_probe("euclidean", K, [n_c], 4, 1, 1, P, L, ff, fv)
    for key in ("copy_of", "gate", "lookup_src"):
        assert np.array_equal(np.asarray(getattr(cm, key)), np.asarray(getattr(pm, key))), key
    assert public == ppublic
    assert (info["centroid_indicator"].shape, info["member_indicator"].shape, info["result"].shape) == ((K,), (n_c,), (4,))
    assert np.array_equal(info["centroid_indicator"], pinfo["centroid_indicators"][0]) and np.array_equal(info["result"], pinfo["results"][0])
    assert np.array_equal(info["member_indicator"], pinfo["candidate_indicators"][0])


def test_wrong_cluster_and_altered_root_break_the_map(O):
    db, ids, cent, query = _setup(O)
    ix = AN.index_model(O, db, ids, cent)
    w = _winner(O, query, cent)
    wrong = (w + 1) % 3
    members, _ = AN.select_cluster(db, ids, wrong)
    m = AN.query_model(O, "euclidean", query, cent, members, ix["roots"][1:4], P, L)
    ff, fv, vals = fetchers(m)
    cm, _, info = CS.build_ann_query("euclidean", 3, members.shape[0], 4, P, L, ff, fv)
    rep = cm.check_witness(vals, TM.to_ints(m["lookup"]), m["flags"])
    assert rep["copies_unequal"] == 1 and vals[info["selected"]] != vals[info["members_root"]]
    members, _ = AN.select_cluster(db, ids, w)
    roots = ix["roots"][1:4].copy()
    roots[w] = O.fr_add(roots[w:w + 1], O.fr_from_ints([1]))[0]
    m = AN.query_model(O, "euclidean", query, cent, members, roots, P, L)
    ff, fv, vals = fetchers(m)
    cm, _, _ = CS.build_ann_query("euclidean", 3, members.shape[0], 4, P, L, ff, fv)
    assert cm.check_witness(vals, TM.to_ints(m["lookup"]), m["flags"])["copies_unequal"] >= 1
    assert not np.array_equal(m["public"][-1], ix["roots"][-1])
    cent2 = cent.copy()
    cent2[0, 0] = O.fr_add(cent2[0, :1], O.fr_from_ints([1]))[0]
    assert not np.array_equal(AN.index_model(O, db, ids, cent2)["roots"][-1], ix["roots"][-1])


@pytest.mark.parametrize("metric,q,n,dim,topk", [("euclidean", 2, 4, 3, 2), ("euclidean", 1, 5, 2, 1), ("manhattan", 2, 3, 2, 3), ("cosine", 1, 1, 2, 1)])
def test_build_nearest_topk_through_place_nearest_is_the_whole_trace(metric, q, n, dim, topk):
    from test_batch_query_cpu import same_map
    whole, (wind, wres) = CS.trace_nearest_topk(metric, q, n, dim, topk, P, L)
    bm, (bind, bres) = CS.build_nearest_topk(metric, q, n, dim, topk, P, L)
    same_map(whole, bm)
    assert np.array_equal(np.asarray(wind), bind) and np.array_equal(np.asarray(wres), bres)
