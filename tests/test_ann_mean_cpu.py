"""The mean audit of one cluster without a GPU (circuit_sym.build_ann_mean; tests/ann_mean_model.py): the model's means against the oracle's
k-means and against Python integers, the host-built map against the model's stream, the binding of a centroid word, of the header's
cluster, of a member and of the cluster roots, and every cell altered alone."""
import numpy as np
import pytest

import alteration_model as AM
import ann_mean_model as MM
import topk_model as TM
from halo2_vectordb_amd import circuit_sym as CS
from test_alteration_cpu import sweep
from test_ann_audit_cpu import broken_copies, index_roots
from test_merkle_update_cpu import fetchers

P, L = 48, 12
SHAPES = [(2, 2, 3, 1), (1, 3, 1, 0), (3, 1, 2, 2)]      # K, n_c, dim, c
_cache = {}


def data(seed, K, n_c, dim):
    """rows on a signed integer grid, so that a word's sum is negative, zero or positive -> (centroids of the other clusters, members) f64"""
    rng = np.random.default_rng(seed)
    return rng.integers(-109, 110, (K, dim)).astype(np.float64), rng.integers(-109, 110, (n_c, dim)).astype(np.float64)


def index_of(O, K, n_c, dim, c, seed=70):
    """a self-consistent index: cluster c holds the members and centroid c is their mean; every other cluster holds one row, its own
    centroid (the mean of one row is the row) -> (quantized centroids, members, roots (K + 2, 4))"""
    cent_f, mem_f = data(seed, K, n_c, dim)
    cent, mem = O.quantize(cent_f, P), O.quantize(mem_f, P)
    cent[c] = MM.means(O, mem, P, L)
    return cent, mem, index_roots(O, cent, [mem if j == c else cent[j:j + 1] for j in range(K)])


def case(O, K, n_c, dim, c, seed=70):
    """-> (model, centroids, members, roots (K + 1, 4), the index root), computed once per case and shared; nothing changes it"""
    key = (K, n_c, dim, c, seed)
    if key not in _cache:
        cent, mem, roots = index_of(O, K, n_c, dim, c, seed)
        _cache[key] = (MM.mean_model(O, cent, mem, roots[:K + 1], c, P, L), cent, mem, roots[:K + 1], roots[-1])
    return _cache[key]


def built(m, K, n_c, dim):
    ff, fv, vals = fetchers(m)
    cm, public, info = CS.build_ann_mean(K, n_c, dim, P, L, ff, fv)
    return cm, public, info, vals


def plus_one(O, x):
    return O.fr_add(np.asarray(x)[None], O.fr_from_ints([1]))[0]


def test_models_means_are_the_oracles_kmeans_centroids_and_the_integer_quotients(O):
    """one Lloyd iteration under Manhattan, whose zero distance is provable (the first K rows start as their own centroids): the
    oracle's centroids are the model's means of the clusters its indicators name"""
    n, K, dim = 9, 3, 2
    rng = np.random.default_rng(5)
    qv = O.quantize(rng.integers(-109, 110, (n, dim)).astype(np.float64), P)
    c = O.Ctx(store=False, keygen=False)
    cent, ind = c.kmeans("manhattan", qv, K, 1, P=P, L=L)
    assert c.err == 0
    ids = np.argmax(ind.any(axis=2), axis=1)
    assert sorted(set(ids.tolist())) == list(range(K)) and (ind.any(axis=2).sum(axis=1) == 1).all()
    sizes = []
    for k in range(K):
        members = qv[ids == k]
        sizes.append(members.shape[0])
        got = MM.means(O, members, P, L)
        assert np.array_equal(got, cent[k]), k
        assert TM.to_ints(got) == MM.means_int(members, P), k
    assert max(sizes) >= 3, sizes


@pytest.mark.parametrize("n,vals", [(3, [[-5], [2], [1]]), (3, [[5], [-2], [-2]]), (2, [[7], [-7]]), (7, [[100], [1], [1], [1], [1], [1], [1]]),
                                    (7, [[-100], [-1], [-1], [-1], [-1], [-1], [-1]]), (1, [[-3]])])
def test_means_round_towards_zero_for_both_signs(O, n, vals):
    """negative, zero and positive sums, inexact quotients, a count that is no power of two: qdiv divides the magnitudes and puts the
    sign back, so -2/3 and 2/3 both lose their fraction towards zero"""
    mem = O.quantize(np.asarray(vals, dtype=np.float64), P)
    got = TM.to_ints(MM.means(O, mem, P, L))
    assert got == MM.means_int(mem, P)
    s = sum(v[0] for v in vals)
    want = (abs(s) << P) // n
    assert got == [(MM.R - want) % MM.R if s < 0 else want]


@pytest.mark.parametrize("K,n_c,dim,c", SHAPES)
def test_host_built_map_against_the_models_stream(O, K, n_c, dim, c):
    m, cent, mem, roots, index_root = case(O, K, n_c, dim, c)
    cm, public, info, vals = built(m, K, n_c, dim)
    rep = cm.check_witness(vals, TM.to_ints(m["lookup"]), m["flags"])
    assert not any(rep.values()), rep
    assert [vals[x] for x in public] == TM.to_ints(m["public"]) and len(public) == 2
    assert np.array_equal(m["public"][0], index_root) and TM.to_ints(m["public"][1:]) == [c]
    assert m["mean_ok"].tolist() == [1] * dim
    lay = CS.ann_mean_layout(K, n_c, dim, P, L)
    assert (lay["total"], lay["total_l"], lay["n_in"]) == (m["advice"].shape[0], m["lookup"].shape[0], m["n_in"])
    assert all(lay[k] == v for k, v in m["regions"].items()), (m["regions"], lay)
    assert (lay["units"]["qd"].n, lay["units"]["qd"].n_lk) == (m["qdiv_cells"], m["qdiv_lk"])
    # the ties the circuit adds are the model's, and nothing else ties those cells
    assert info["own"] == m["own"] and info["mean"] == m["mean"] and info["len"] == m["regions"]["len"]
    assert (info["picked"], info["centroids_root"], info["members_root"]) == (m["picked_cell"], m["croot_cell"], m["mroot_cell"])
    for cell, src in m["ties"]:
        assert cm.copy_of[cell] == src, (cell, src)
    assert vals[lay["len"]] == n_c << P and cm.consts[cm.const_idx[lay["len"]]] == n_c << P


def test_a_centroid_word_moved_by_one_breaks_that_words_tie_alone(O):
    K, n_c, dim, c = 2, 2, 3, 1
    cent, mem, _ = index_of(O, K, n_c, dim, c)
    for j in range(dim):
        cent2 = cent.copy()
        cent2[c, j] = plus_one(O, cent2[c, j])
        roots = index_roots(O, cent2, [mem if k == c else cent2[k:k + 1] for k in range(K)])      # self-consistent: the trees are the new rows'
        m = MM.mean_model(O, cent2, mem, roots[:K + 1], c, P, L)
        cm, public, info, vals = built(m, K, n_c, dim)
        want = [1] * dim
        want[j] = 0
        assert m["mean_ok"].tolist() == want
        assert broken_copies(cm, vals) == [m["mean"][j]] and cm.copy_of[m["mean"][j]] == m["own"][j]
        rep = cm.check_witness(vals, TM.to_ints(m["lookup"]), m["flags"])
        assert rep.pop("copies_unequal") == 1 and not any(rep.values()), rep


def test_header_cluster_member_and_cluster_roots_are_bound(O):
    K, n_c, dim, c = 2, 2, 3, 1
    m0, cent, mem, roots, index_root = case(O, K, n_c, dim, c)
    # a header c' != c: the members are cluster c's, the selection picks cluster_root_c' -> mroot = picked breaks (and centroid c' is
    # not their mean, so mean = own copies break too)
    m = MM.mean_model(O, cent, mem, roots, 0, P, L)
    cm, _, info, vals = built(m, K, n_c, dim)
    broken = broken_copies(cm, vals)
    assert m["mroot_cell"] in broken and set(broken) <= {m["mroot_cell"]} | set(m["mean"])
    # one altered member, in a word whose quotient keeps its bits: mroot = picked breaks alone
    keeps = []
    for j in range(dim):
        mem2 = mem.copy()
        mem2[0, j] = plus_one(O, mem2[0, j])
        if MM.means_int(mem2, P) == MM.means_int(mem, P):
            keeps.append(mem2)
    assert keeps, "a word whose sum plus one has the same quotient"
    m = MM.mean_model(O, cent, keeps[0], roots, c, P, L)
    cm, _, info, vals = built(m, K, n_c, dim)
    assert broken_copies(cm, vals) == [m["mroot_cell"]] and cm.copy_of[m["mroot_cell"]] == m["picked_cell"]
    assert m["mean_ok"].tolist() == [1] * dim
    # another cluster's root altered: every copy holds, the index root is another
    roots2 = roots.copy()
    roots2[1] = plus_one(O, roots2[1])
    m = MM.mean_model(O, cent, mem, roots2, c, P, L)
    cm, public, info, vals = built(m, K, n_c, dim)
    assert broken_copies(cm, vals) == [] and not np.array_equal(m["public"][0], index_root)
    # ... and cluster c's own root altered breaks mroot = picked
    roots2 = roots.copy()
    roots2[1 + c] = plus_one(O, roots2[1 + c])
    m = MM.mean_model(O, cent, mem, roots2, c, P, L)
    cm, _, info, vals = built(m, K, n_c, dim)
    assert broken_copies(cm, vals) == [m["mroot_cell"]]


def _qdiv_alone(O, a, b):
    """the offsets inside its block of the cells that qdiv(a, b), emitted alone after its assigned operands, leaves unnoticed, each with
    alteration_model's reason"""
    c, s = O.Ctx(store=True, keygen=True), CS.Sym(P, L)
    c.assign_witnesses(np.stack([a, b])[None])
    c.op("qdiv", a, b, P=P, L=L)
    s.qdiv(*s.assign_witnesses(2))
    assert c.err == 0
    cm = CS._whole(s, 2)
    vals = np.asarray(TM.to_ints(c.advice()), dtype=object)
    assert cm.n_cells == len(vals)
    free = AM.unnoticed(cm, vals, np.asarray(TM.to_ints(c.lookup()), dtype=object), [])
    return [(x - 2, AM.explain(cm, vals, x)) for x in free]


@pytest.mark.parametrize("K,n_c,dim,c", SHAPES[:2])
def test_every_cell_altered_alone(O, K, n_c, dim, c):
    m, cent, mem, roots, _ = case(O, K, n_c, dim, c)
    cm, public, info, vals = built(m, K, n_c, dim)
    free = sweep(f"ann mean K {K} n_c {n_c} c {c} dim {dim}", cm, vals, TM.to_ints(m["lookup"]), public, L, m["flags"])
    lay = info["layout"]
    bounds = [("head", lay["update"]), ("assigned", lay["own"]), ("own", lay["len"]), ("len", lay["chain"]), ("chain", lay["div"]),
              ("qdiv", lay["merkle_c"]), ("tree", lay["total"])]
    kinds = {}
    for x in free:
        kinds.setdefault(next(name for name, end in bounds if x < end), []).append(x)
    print({k: len(v) for k, v in kinds.items()})
    assert set(kinds) <= {"head", "qdiv"}, kinds
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


def test_layout_refusals_and_exports():
    from halo2_vectordb_amd import _lib
    lib = _lib.load()
    for name in ("vdb_wit_ann_mean_size", "vdb_wit_ann_mean", "vdb_wit_ann_mean_dev", "vdb_ann_cluster_means", "vdb_ann_cluster_means_dev"):
        assert hasattr(lib, name), name
    for K, n_c, dim in ((0, 1, 4), (1, 0, 4), (1, 1, 0)):
        with pytest.raises(ValueError):
            CS.ann_mean_layout(K, n_c, dim, P, L)
    with pytest.raises(ValueError):
        CS.ann_mean_layout(1, 1 << 8, 1, 8, 4)              # quantization(n_c) = 2^16 is not below 2^(2 P)
    assert CS.ann_mean_layout(1, (1 << 8) - 1, 1, 8, 4)["total_l"] > 0
    assert CS.ann_mean_instances(7, 0) == [7, 0]


@pytest.mark.parametrize("K,n_c,dim", [(1, 1, 1), (2, 3, 2), (3, 5, 4), (65, 2, 1)])
def test_the_two_audits_share_one_cluster_frame(K, n_c, dim):
    """K = 65: the first K above one 64-lane block of indicators; K = 1: no is_equal block; (2, 3, 2): a padded centroid tree that is
    full (zero_c false) beside a padded member tree"""
    audit, mean = CS.ann_audit_layout("euclidean", K, n_c, dim, P, L), CS.ann_mean_layout(K, n_c, dim, P, L)
    head = ("c", "centroids_root", "roots", "n_in", "indicator", "sponge", "select", "sponge_old", "update")
    frame = head + ("centroids", "members", "zero_c")     # every key the two share up to and including `members`
    assert {k for k in audit if k in mean} - set(frame) == {"units", "merkle_c", "merkle_m", "total", "total_l"}
    for k in frame:
        assert audit[k] == mean[k], k
    update = CS.ann_update_layout(K, 1, dim, 1)
    for k in head:
        assert audit[k] == update[k], k
    assert audit["centroids"] == audit["update"] and audit["members"] == audit["centroids"] + K * dim
    assert audit["routed"] == mean["own"] == audit["members"] + n_c * dim
    for lay in (audit, mean):
        assert lay["merkle_m"] - lay["merkle_c"] == CS.merkle_cells(K, dim)
        assert lay["total"] - lay["merkle_m"] == CS.merkle_cells(n_c, dim, lay["zero_c"])
    assert audit["zero_c"] == (K not in (1, 2))
