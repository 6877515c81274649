"""The cover of the database by the index without a GPU (circuit_sym.build_ann_cover; tests/ann_cover_model.py): the host-built map against
the model's stream, the two public roots against the oracle's commitments, the tie list, what a foreign leaf, a repeated leaf, a leaf
moved across a cluster border and an altered header root break, and every cell altered alone."""
import numpy as np
import pytest

import alteration_model as AM
import ann_cover_model as CM
import topk_model as TM
from halo2_vectordb_amd import circuit_sym as CS
from test_alteration_cpu import sweep
from test_ann_audit_cpu import broken_copies, index_roots
from test_ann_mean_cpu import plus_one
from test_merkle_update_cpu import fetchers

P, L, DIM = 48, 8, 3
# (1): no node, no Z, one factor a side; (1, 2): a padded database tree, a cluster without a node, a full cluster; (3, 1, 5): padding in
# the database tree and in two clusters; (4, 4): no padding anywhere, no Z
SHAPES = [(1,), (1, 2), (3, 1, 5), (4, 4)]
_cache = {}


def database_f64(sizes, seed=90):
    """rows on a signed integer grid whose clusters interleave in slot order -> (rows (n, DIM) f64, cluster ids (n,), centroids (K, DIM) f64)"""
    rng = np.random.default_rng(seed + len(sizes))
    n, K = sum(sizes), len(sizes)
    ids = rng.permutation(np.repeat(np.arange(K), sizes))
    return rng.integers(-109, 110, (n, DIM)).astype(np.float64), ids, rng.integers(-109, 110, (K, DIM)).astype(np.float64)


def database(O, sizes, seed=90):
    """database_f64 quantized -> (rows (n, DIM, 4), cluster ids (n,), centroids (K, DIM, 4))"""
    rows, ids, cent = database_f64(sizes, seed)
    return O.quantize(rows, P), ids, O.quantize(cent, P)


def leaves_of(O, rows, ids, K):
    """-> (a: the leaf digests in slot order, b: in grouped order (stable), the clusters' rows)"""
    a = O.poseidon_hash_many(rows)
    order = np.argsort(ids, kind="stable")
    return a, np.ascontiguousarray(a[order]), [np.ascontiguousarray(rows[ids == c]) for c in range(K)]


def case(O, sizes):
    """-> (model, rows, ids, centroids, a, b, clusters), computed once per shape and shared; nothing changes it"""
    if sizes not in _cache:
        rows, ids, cent = database(O, sizes)
        a, b, clusters = leaves_of(O, rows, ids, len(sizes))
        _cache[sizes] = (CM.cover_model(O, a, b, sizes, O.poseidon_merkle_root(cent)), rows, ids, cent, a, b, clusters)
    return _cache[sizes]


def built(m, sizes):
    ff, fv, vals = fetchers(m)
    cm, public, info = CS.build_ann_cover(sizes, ff, fv)
    return cm, public, info, vals


def clean(cm, vals, m, public):
    rep = cm.check_witness(vals, [], m["flags"])
    assert not any(rep.values()), rep
    honest = AM.recount(cm, vals, np.asarray([], dtype=object), L, public, [vals[c] for c in public])
    assert AM.violations(honest) == 0, honest


@pytest.mark.parametrize("sizes", SHAPES)
def test_host_built_map_against_the_models_stream(O, sizes):
    m, rows, ids, cent, a, b, clusters = case(O, sizes)
    K, n = len(sizes), sum(sizes)
    cm, public, info, vals = built(m, sizes)
    clean(cm, vals, m, public)                               # every gate, copy and constant
    lay = CS.ann_cover_layout(sizes)
    assert (lay["total"], lay["total_l"], lay["n_in"]) == (m["advice"].shape[0], 0, m["n_in"])
    assert all(lay[k] == v for k, v in m["regions"].items()), (m["regions"], lay)
    assert (lay["zero"] is None) == (sizes in ((1,), (4, 4)))
    # the public row: the oracle's merkle_commitment root of the rows in slot order, and the index root
    assert [vals[x] for x in public] == TM.to_ints(m["public"]) and len(public) == 2
    assert public == [m["droot_cell"], m["iroot_cell"]] == CS.ann_cover_instances(m["droot_cell"], m["iroot_cell"])
    assert np.array_equal(m["public"][0], O.poseidon_merkle_root(rows))
    assert np.array_equal(m["public"][1], index_roots(O, cent, clusters)[-1])
    # the ties the circuit adds are the model's: K roots to the header, one product to the other
    assert info["roots"] == m["root_cells"] and (info["last_a"], info["last_b"], info["gamma"]) == (m["last_a"], m["last_b"], m["gamma_cell"])
    assert len(m["ties"]) == K + 1
    for cell, src in m["ties"]:
        assert cm.copy_of[cell] == src, (cell, src)
    # what else copies: the trees' inputs copy I and Z, D's words the header, G's words droot and D's digest, the products' operands
    # gamma, I and each other; nothing but the K + 1 ties above points from a tree, a sponge or an accumulator back at the header or
    # across the two sides
    tied = np.flatnonzero(cm.copy_of != np.arange(cm.n_cells))
    to_header = [int(x) for x in tied if 1 <= cm.copy_of[x] <= K and x < lay["sponge"]]
    assert to_header == sorted(m["root_cells"])
    assert [int(x) for x in tied if x >= lay["sub_b"] and lay["sub_a"] <= cm.copy_of[x] < lay["sub_b"]] == [m["last_b"]]
    gam = np.flatnonzero(cm.copy_of == m["gamma_cell"])
    assert gam[gam >= lay["sub_a"]].tolist() == [lay["sub_a"] + 4 * i + 3 for i in range(n)] + [lay["sub_b"] + 4 * i + 3 for i in range(n)]
    # a cluster of one member has no node: its root is its leaf cell
    offs = np.concatenate([[0], np.cumsum(sizes)])
    for c in range(K):
        if sizes[c] == 1:
            assert m["root_cells"][c] == lay["b"] + offs[c]


def altered(O, sizes, change):
    """the model and the map over b changed by `change(b)` -> (m0, m, cm, vals)"""
    m0, rows, ids, cent, a, b, clusters = case(O, sizes)
    b2 = b.copy()
    change(b2)
    m = CM.cover_model(O, a, b2, sizes, O.poseidon_merkle_root(cent))
    cm, public, info, vals = built(m, sizes)
    return m0, m, cm, vals


@pytest.mark.parametrize("sizes", SHAPES)
def test_a_cluster_leaf_that_is_not_in_the_database_breaks_the_product_tie_alone(O, sizes):
    foreign = O.poseidon_hash_many(O.quantize(np.full((1, DIM), 7.5), P))[0]

    def change(b):
        b[-1] = foreign
    m0, m, cm, vals = altered(O, sizes, change)
    assert broken_copies(cm, vals) == [m["last_b"]] and cm.copy_of[m["last_b"]] == m["last_a"]
    assert np.array_equal(m["public"][0], m0["public"][0]) and not np.array_equal(m["public"][1], m0["public"][1])


@pytest.mark.parametrize("sizes", SHAPES[1:])
def test_a_repeated_cluster_leaf_breaks_the_product_tie_alone(O, sizes):
    """the set of digests is a subset of the database's, the multiset is not: multiplicity counts"""
    def change(b):
        b[-1] = b[0]
    m0, m, cm, vals = altered(O, sizes, change)
    assert broken_copies(cm, vals) == [m["last_b"]]


@pytest.mark.parametrize("sizes", SHAPES[1:])
def test_a_leaf_moved_across_a_cluster_border_keeps_the_tie_and_changes_the_index_root(O, sizes):
    """the last member of cluster 0 and the first of cluster 1 change places: the same multiset under other cluster roots"""
    at = sizes[0]

    def change(b):
        b[[at - 1, at]] = b[[at, at - 1]]
    m0, m, cm, vals = altered(O, sizes, change)
    assert broken_copies(cm, vals) == []
    assert np.array_equal(m["public"][0], m0["public"][0]) and not np.array_equal(m["public"][1], m0["public"][1])
    assert vals[m["last_b"]] == vals[m["last_a"]]


@pytest.mark.parametrize("sizes", SHAPES)
def test_an_altered_header_root_breaks_its_root_tie_alone(O, sizes):
    m0, rows, ids, cent, a, b, clusters = case(O, sizes)
    for c in range(len(sizes)):
        hdr = m0["roots"].copy()
        hdr[c] = plus_one(O, hdr[c])
        m = CM.cover_model(O, a, b, sizes, O.poseidon_merkle_root(cent), header_roots=hdr)
        cm, public, info, vals = built(m, sizes)
        assert broken_copies(cm, vals) == [m["root_cells"][c]] and cm.copy_of[m["root_cells"][c]] == 1 + c
        assert not np.array_equal(m["public"][1], m0["public"][1])


@pytest.mark.parametrize("sizes", SHAPES[:3])
def test_every_cell_altered_alone(O, sizes):
    """no is_zero anywhere in the circuit: no cell is free"""
    m, *_ = case(O, sizes)
    cm, public, info, vals = built(m, sizes)
    free = sweep(f"ann cover sizes {sizes}", cm, vals, [], public, L, m["flags"])
    assert free == [], free


def test_layout_refusals_and_exports():
    from halo2_vectordb_amd import _lib, api, pipeline
    lib = _lib.load()
    for name in ("vdb_wit_ann_cover_size", "vdb_wit_ann_cover", "vdb_wit_ann_cover_dev", "vdb_ann_index_db_tree_dev"):
        assert hasattr(lib, name), name
    assert callable(api.wit_ann_cover) and callable(api.ann_index_db_tree)
    assert hasattr(pipeline, "AnnCoverHotPath") and hasattr(pipeline.AnnIndex, "database_tree")
    for sizes in ((), (0,), (2, 0, 1)):
        with pytest.raises(ValueError):
            CS.ann_cover_layout(sizes)
    assert CS.ann_cover_instances(7, 9) == [7, 9]
    node = CS.merkle_leaf_layout(2)["leaf_cells"]
    assert node == CM.NODE == CS.merkle_leaf_layout(5)["node_cells"]
    # the n = 300 shape of the GPU tests: 1,019 nodes, about 4.6 M cells
    lay = CS.ann_cover_layout((1, 40, 64, 65, 130))
    assert (lay["n"], lay["lp"], lay["lps"]) == (300, 512, [1, 64, 64, 128, 256])
    assert (lay["sponge"] - lay["tree_d"]) // node == 511 + 0 + 63 + 63 + 127 + 255 and lay["total"] == 4610537
    # place_tree over one digest places nothing
    assert CS.place_tree(None, [17], 40, node) == (17, 40)
