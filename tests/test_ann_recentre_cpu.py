"""The recentre of one cluster without a GPU (circuit_sym.build_ann_recentre; tests/ann_recentre_model.py): the host-built map against the
model's stream, the new root against the index rebuilt with row c replaced, the chain of K recentres against the index built on the
means, the binding of the header's cluster, of a member, of the new vector, of the cluster roots and of the centroids' tree, and every cell
altered alone."""
import numpy as np
import pytest

import alteration_model as AM
import ann_mean_model as MM
import ann_recentre_model as RM
import merkle_update_model as MU
import topk_model as TM
from halo2_vectordb_amd import circuit_sym as CS
from test_alteration_cpu import sweep
from test_ann_audit_cpu import broken_copies, index_roots
from test_ann_mean_cpu import _qdiv_alone, data, plus_one
from test_merkle_update_cpu import fetchers

P, L = 48, 12
# K, n_c, dim, c: depth 1 and depth 3; a padded (3, 5) and a full (2) centroids' tree; n_c = 1 has no chain; n_c = 3 pads the members' tree
SHAPES = [(2, 2, 3, 1), (3, 1, 2, 2), (5, 3, 1, 0), (2, 3, 2, 0)]
_cache = {}


def index_of(O, K, n_c, dim, c, seed=80, at_mean=False):
    """an index with arbitrary centroids (at_mean: centroid c already the mean of its members): cluster c holds the members, every other
    cluster one row, its own centroid -> (quantized centroids, members, clusters, roots (K + 2, 4))"""
    cent_f, mem_f = data(seed, K, n_c, dim)
    cent, mem = O.quantize(cent_f, P), O.quantize(mem_f, P)
    if at_mean:
        cent[c] = MM.means(O, mem, P, L)
    clusters = [mem if j == c else cent[j:j + 1].copy() for j in range(K)]
    return cent, mem, clusters, index_roots(O, cent, clusters)


def case(O, K, n_c, dim, c, seed=80):
    """-> (model, centroids, members, clusters, roots (K + 2, 4), the centroids' tree after the write), computed once per case and shared"""
    key = (K, n_c, dim, c, seed)
    if key not in _cache:
        cent, mem, clusters, roots = index_of(O, K, n_c, dim, c, seed)
        tree = MU.build_tree(O, cent)
        _cache[key] = (RM.recentre_model(O, tree, mem, roots[:K + 1], c, P, L), cent, mem, clusters, roots, tree)
    return _cache[key]


def built(m, K, n_c, dim):
    ff, fv, vals = fetchers(m)
    cm, public, info = CS.build_ann_recentre(K, n_c, dim, P, L, ff, fv)
    return cm, public, info, vals


@pytest.mark.parametrize("K,n_c,dim,c", SHAPES)
def test_host_built_map_against_the_models_stream(O, K, n_c, dim, c):
    m, cent, mem, clusters, roots, tree = case(O, K, n_c, dim, c)
    cm, public, info, vals = built(m, K, n_c, dim)
    rep = cm.check_witness(vals, TM.to_ints(m["lookup"]), m["flags"])
    assert not any(rep.values()), rep
    assert [vals[x] for x in public] == TM.to_ints(m["public"]) and len(public) == 3
    assert np.array_equal(m["public"][0], roots[-1]) and TM.to_ints(m["public"][1:2]) == [c]
    lay = CS.ann_recentre_layout(K, n_c, dim, P, L)
    assert (lay["total"], lay["total_l"], lay["n_in"]) == (m["advice"].shape[0], m["lookup"].shape[0], m["n_in"])
    assert all(lay[k] == v for k, v in m["regions"].items()), (m["regions"], lay)
    assert (lay["units"]["qd"].n, lay["units"]["qd"].n_lk) == (m["qdiv_cells"], m["qdiv_lk"])
    assert lay["depth"] == len(tree) - 1 and lay["update_layout"]["total"] == m["update"]["advice"].shape[0]
    # the ties the circuit adds are the model's, and nothing else ties those cells (a cell copies one cell)
    assert info["mean"] == m["mean"] and info["new_vector"] == m["new_vector"] and info["len"] == m["regions"]["len"]
    assert (info["picked"], info["members_root"]) == (m["picked_cell"], m["mroot_cell"])
    assert (info["update_public"][0], info["update_public"][1], info["update_public"][-1]) == (m["old_root_cell"], m["idx_cell"], m["new_root_cell"])
    assert len(m["ties"]) == dim + 3
    for cell, src in m["ties"]:
        assert cm.copy_of[cell] == src, (cell, src)
    # G absorbs copies: word 0 the update block's new root, words 1 .. K the header's cluster roots; block F's selects do not appear
    g = cm.copy_of[lay["sponge_new"]:lay["total"]]
    outside = sorted(int(x) for x in g[g < lay["sponge_new"]])
    assert outside == sorted([m["new_root_cell"]] + [lay["roots"] + j for j in range(K)])
    assert lay["sponge_new"] == lay["centroid_update"] + lay["update_layout"]["total"]
    assert vals[lay["len"]] == n_c << P and cm.consts[cm.const_idx[lay["len"]]] == n_c << P
    # the new root is the root of the index rebuilt with row c replaced by the members' mean
    cent2 = cent.copy()
    cent2[c] = MM.means(O, mem, P, L)
    assert np.array_equal(m["new_centroid"], cent2[c])
    assert np.array_equal(m["public"][2], index_roots(O, cent2, clusters)[-1])
    assert np.array_equal(MU.flat_levels(tree), MU.flat_levels(MU.build_tree(O, cent2)))
    assert not np.array_equal(m["public"][2], m["public"][0])


def test_a_centroid_already_at_the_mean_keeps_the_root(O):
    K, n_c, dim, c = 2, 2, 3, 1
    cent, mem, clusters, roots = index_of(O, K, n_c, dim, c, at_mean=True)
    m = RM.recentre_model(O, MU.build_tree(O, cent), mem, roots[:K + 1], c, P, L)
    assert np.array_equal(m["public"][2], m["public"][0]) and np.array_equal(m["public"][0], roots[-1])
    cm, public, info, vals = built(m, K, n_c, dim)
    assert not any(cm.check_witness(vals, TM.to_ints(m["lookup"]), m["flags"]).values())


def test_k_recentres_in_a_row_end_on_the_index_built_on_the_means(O):
    """arbitrary centroids, clusters of 1 .. 3 members: the model applied for c = 0 .. K - 1, each on the roots and the tree the one before
    left, ends on the root of the index built on index_means; every link's old root is the root before it"""
    K, dim = 3, 2
    rng = np.random.default_rng(81)
    cent = O.quantize(rng.integers(-109, 110, (K, dim)).astype(np.float64), P)
    clusters = [O.quantize(rng.integers(-109, 110, (n, dim)).astype(np.float64), P) for n in (2, 1, 3)]
    roots = index_roots(O, cent, clusters)
    tree, at = MU.build_tree(O, cent), roots[-1]
    for c in range(K):
        m = RM.recentre_model(O, tree, clusters[c], roots[:K + 1], c, P, L)
        assert np.array_equal(m["public"][0], at)
        at = m["public"][2]
        roots = np.concatenate([m["new_centroids_root"][None], roots[1:K + 1], at[None]])
    offsets = np.concatenate([[0], np.cumsum([x.shape[0] for x in clusters])])
    means = MM.index_means(O, np.concatenate(clusters), offsets, P, L)
    assert np.array_equal(roots, index_roots(O, means, clusters))


def test_header_cluster_member_new_vector_cluster_roots_and_tree_are_bound(O):
    K, n_c, dim, c = 2, 2, 3, 1
    m0, cent, mem, clusters, roots, _ = case(O, K, n_c, dim, c)
    r = roots[:K + 1]
    fresh = lambda: MU.build_tree(O, cent)
    # a header c' != c: the members are cluster c's, the selection picks cluster_root_c' -> mroot = picked breaks, and nothing else
    m = RM.recentre_model(O, fresh(), mem, r, 0, P, L)
    cm, _, info, vals = built(m, K, n_c, dim)
    assert broken_copies(cm, vals) == [m["mroot_cell"]] and cm.copy_of[m["mroot_cell"]] == m["picked_cell"]
    # one altered member, in a word whose quotient keeps its bits: mroot = picked breaks alone
    keeps = []
    for j in range(dim):
        mem2 = mem.copy()
        mem2[0, j] = plus_one(O, mem2[0, j])
        if MM.means_int(mem2, P) == MM.means_int(mem, P):
            keeps.append(mem2)
    assert keeps, "a word whose sum plus one has the same quotient"
    m = RM.recentre_model(O, fresh(), keeps[0], r, c, P, L)
    cm, _, info, vals = built(m, K, n_c, dim)
    assert broken_copies(cm, vals) == [m["mroot_cell"]]
    assert np.array_equal(m["public"], m0["public"])
    # a new-vector word off by one breaks that word's tie alone
    for j in range(dim):
        nv = m0["new_centroid"].copy()
        nv[j] = plus_one(O, nv[j])
        m = RM.recentre_model(O, fresh(), mem, r, c, P, L, new_vector=nv)
        cm, _, info, vals = built(m, K, n_c, dim)
        assert broken_copies(cm, vals) == [m["new_vector"][j]] and cm.copy_of[m["new_vector"][j]] == m["mean"][j]
        assert not np.array_equal(m["public"][2], m0["public"][2])
    # another cluster's root altered: every copy holds, both public roots are others
    roots2 = r.copy()
    roots2[1] = plus_one(O, roots2[1])
    m = RM.recentre_model(O, fresh(), mem, roots2, c, P, L)
    cm, public, info, vals = built(m, K, n_c, dim)
    assert broken_copies(cm, vals) == []
    assert not np.array_equal(m["public"][0], m0["public"][0]) and not np.array_equal(m["public"][2], m0["public"][2])
    # the levels of another tree: old root = centroids_root breaks, alone
    other = cent.copy()
    other[0, 0] = plus_one(O, other[0, 0])
    m = RM.recentre_model(O, MU.build_tree(O, other), mem, r, c, P, L)
    cm, _, info, vals = built(m, K, n_c, dim)
    assert broken_copies(cm, vals) == [m["old_root_cell"]] and cm.copy_of[m["old_root_cell"]] == 1


@pytest.mark.parametrize("K,n_c,dim,c", SHAPES[:2])
def test_every_cell_altered_alone(O, K, n_c, dim, c):
    m, cent, mem, clusters, roots, _ = case(O, K, n_c, dim, c)
    cm, public, info, vals = built(m, K, n_c, dim)
    free = sweep(f"ann recentre K {K} n_c {n_c} c {c} dim {dim}", cm, vals, TM.to_ints(m["lookup"]), public, L, m["flags"])
    lay = info["layout"]
    bounds = [("head", lay["update"]), ("assigned", lay["len"]), ("len", lay["chain"]), ("chain", lay["div"]), ("qdiv", lay["merkle_m"]),
              ("tree", lay["centroid_update"]), ("path", lay["sponge_new"]), ("sponge", lay["total"])]
    kinds = {}
    for x in free:
        kinds.setdefault(next(name for name, end in bounds if x < end), []).append(x)
    print({k: len(v) for k, v in kinds.items()})
    assert set(kinds) <= {"head", "qdiv"}, kinds                 # none lies in what this circuit adds
    tied = {x for pair in m["ties"] for x in pair}
    assert not tied & set(free)
    # the head keeps its one free inverse: indicator c's is_zero has a zero operand
    inv_c = lay["indicator"] + (8 + 12 * (c - 1) + 4 if c else 0) + 2
    assert kinds.get("head", []) == [inv_c] and AM.explain(cm, vals, inv_c) == AM.IS_ZERO_INVERSE
    # what a qdiv block leaves free is what qdiv, emitted alone on the same operands, leaves free: the same offsets, the same reason
    q_n = lay["units"]["qd"].n
    v = O.Ctx(store=False, keygen=False)
    ln = TM.to_limbs([n_c << P])[0]
    for j in range(dim):
        s = mem[0, j]
        for i in range(1, n_c):
            s = v.op("qadd", mem[i, j], s, P=P, L=L)
        lo = lay["div"] + j * q_n
        got = [(x - lo, AM.explain(cm, vals, x)) for x in kinds.get("qdiv", []) if lo <= x < lo + q_n]
        assert got == _qdiv_alone(O, s, ln), j
    assert all(AM.explain(cm, vals, x) is not None for x in free)


def test_layout_refusals_exports_and_the_heads_keys():
    from halo2_vectordb_amd import _lib, api, pipeline
    lib = _lib.load()
    for name in ("vdb_wit_ann_recentre_size", "vdb_wit_ann_recentre", "vdb_wit_ann_recentre_dev", "vdb_ann_index_recentre_dev"):
        assert hasattr(lib, name), name
    assert callable(api.wit_ann_recentre) and hasattr(pipeline, "AnnRecentreHotPath") and hasattr(pipeline.AnnIndex, "recentred_with")
    for K, n_c, dim in ((1, 2, 4), (0, 2, 4), (2, 0, 4), (2, 1, 0)):
        with pytest.raises(ValueError):
            CS.ann_recentre_layout(K, n_c, dim, P, L)
    with pytest.raises(ValueError):
        CS.ann_recentre_layout(2, 1 << 8, 1, 8, 4)           # quantization(n_c) = 2^16 is not below 2^(2 P)
    assert CS.ann_recentre_layout(2, (1 << 8) - 1, 1, 8, 4)["total_l"] > 0
    assert CS.ann_recentre_instances(7, 0, 9) == [7, 0, 9]
    head = ("c", "centroids_root", "roots", "n_in", "indicator", "sponge", "select", "sponge_old", "update")
    for K, n_c, dim in ((2, 1, 1), (3, 5, 4), (65, 2, 1)):
        lay, update = CS.ann_recentre_layout(K, n_c, dim, P, L), CS.ann_update_layout(K, 1, dim, 1)
        for k in head:
            assert lay[k] == update[k], k
        assert lay["members"] == lay["update"] and lay["merkle_m"] - lay["div"] == dim * lay["units"]["qd"].n
        assert lay["centroid_update"] - lay["merkle_m"] == CS.merkle_cells(n_c, dim)
        assert lay["total"] - lay["sponge_new"] == lay["sponge"]["leaf_cells"]
