"""The audit of one cluster's routing without a GPU (circuit_sym.build_ann_audit; tests/ann_audit_model.py): the host-built map against the
model's stream at every shape and metric, the binding of a misrouted member, of the header's cluster, of the centroids and of the cluster
roots, the tie rule (a member equidistant from two centroids is accepted under either), and every cell altered alone."""
import numpy as np
import pytest

import alteration_model as AM
import ann_audit_model as AA
import ann_model as AN
import ann_update_model as AU
import merkle_update_model as MU
import topk_model as TM
from halo2_vectordb_amd import circuit_sym as CS
from test_alteration_cpu import sweep
from test_merkle_update_cpu import fetchers

P, L, DIM = 48, 12, 4
SHAPES = [(1, 1, 0), (2, 2, 1), (3, 5, 2), (3, 5, 0), (5, 70, 3), (65, 2, 64)]      # K, n_c, c
CASES = [("euclidean",) + s for s in SHAPES] + [(m, 3, 5, 2) for m in ("manhattan", "cosine", "hamming")]
_cache = {}


def index_roots(O, cent, clusters):
    """[centroids' root | cluster roots | index root] of an index whose cluster j holds the rows clusters[j]"""
    roots = [O.poseidon_merkle_root(cent)] + [O.poseidon_merkle_root(m) for m in clusters]
    roots.append(O.poseidon_merkle_root(np.stack(roots)[None]))
    return np.stack(roots)


def case(O, metric, K, n_c, c, seed=60):
    """-> (model, quantized centroids, members, roots (K + 1, 4), the index root): cluster c holds the recipe's members, every other
    cluster one row, its own centroid.  Computed once per case and shared; nothing changes it."""
    key = (metric, K, n_c, c, seed)
    if key not in _cache:
        cent_f, mem_f = AA.data(seed, K, n_c, c)
        cent, mem = O.quantize(cent_f, P), O.quantize(mem_f, P)
        d = AA.distances(O, metric, cent, mem, P, L)
        assert all(di[c] == min(di) for di in d), "the own centroid attains the minimum"
        if metric != "hamming":
            assert all(len(set(di)) == K for di in d), "the K distances of every member are pairwise distinct"
        roots = index_roots(O, cent, [mem if j == c else cent[j:j + 1] for j in range(K)])
        _cache[key] = (AA.audit_model(O, metric, cent, mem, roots[:K + 1], c, P, L), cent, mem, roots[:K + 1], roots[-1])
    return _cache[key]


def built(m, metric, K, n_c):
    ff, fv, vals = fetchers(m)
    cm, public, info = CS.build_ann_audit(metric, K, n_c, DIM, P, L, ff, fv)
    return cm, public, info, vals


def broken_copies(cm, vals):
    tied = np.flatnonzero(cm.copy_of != np.arange(cm.n_cells))
    return [int(x) for x in tied[np.asarray(vals[tied] != vals[cm.copy_of[tied]], dtype=bool)]]


@pytest.mark.parametrize("metric,K,n_c,c", CASES)
def test_host_built_map_against_the_models_stream(O, metric, K, n_c, c):
    m, cent, mem, roots, index_root = case(O, metric, K, n_c, c)
    cm, public, info, vals = built(m, metric, K, n_c)
    rep = cm.check_witness(vals, TM.to_ints(m["lookup"]), m["flags"])
    assert not any(rep.values()), rep
    assert [vals[x] for x in public] == TM.to_ints(m["public"]) and len(public) == 2
    assert np.array_equal(m["public"][0], index_root) and TM.to_ints(m["public"][1:]) == [c]
    assert m["routed"].tolist() == [1] * n_c
    lay = CS.ann_audit_layout(metric, K, n_c, DIM, P, L)
    assert (lay["total"], lay["total_l"], lay["n_in"]) == (m["advice"].shape[0], m["lookup"].shape[0], m["n_in"])
    assert all(lay[k] == v for k, v in m["regions"].items()), (m["regions"], lay)
    assert all(lay[k] == m[k] for k in ("per_member", "per_member_l", "chain_off", "pick_off"))
    # the ties the circuit adds are the model's, and nothing else ties those cells
    assert info["own"] == m["own"] and info["m"] == m["m"]
    assert (info["picked"], info["centroids_root"], info["members_root"]) == (m["picked_cell"], m["croot_cell"], m["mroot_cell"])
    for cell, src in m["ties"]:
        assert cm.copy_of[cell] == src, (cell, src)


@pytest.mark.parametrize("K,c", [(1, 0), (2, 1), (3, 2), (3, 0), (5, 3), (65, 64)])
def test_the_heads_map_is_the_index_updates_cell_for_cell(O, K, c):
    """blocks A - D are placed by the function the update's map uses; held here against build_ann_update on an update model's stream over
    the same K and c (a two-member cluster, one replacement)"""
    rng = np.random.default_rng(K)
    q = lambda n: O.quantize(rng.integers(0, 219, size=(n, DIM)).astype(np.float64), P)
    cent, two, new = q(K), q(2), q(1)
    roots = index_roots(O, cent, [two if j == c else cent[j:j + 1] for j in range(K)])
    mu = AU.update_model(O, roots[:K + 1], c, MU.build_tree(O, two), [0], new, 0)
    um, _, uinfo = CS.build_ann_update(K, 1, DIM, 1, *fetchers(mu)[:2])
    m = case(O, "euclidean", K, {1: 1, 2: 2, 3: 5, 5: 70, 65: 2}[K], c)[0]
    cm, _, info, _ = built(m, "euclidean", K, m["routed"].shape[0])
    head = info["layout"]["update"]
    assert head == uinfo["layout"]["update"] == m["regions"]["centroids"]
    for name in ("copy_of", "gate", "asserted"):
        assert np.array_equal(getattr(cm, name)[:head], getattr(um, name)[:head]), name
    value = lambda x: [None if i < 0 else x.consts[i] for i in x.const_idx[:head]]
    assert value(cm) == value(um)
    assert info["indicators"] == uinfo["indicators"] and info["picked"] == uinfo["picked"] and info["index_root"] == uinfo["index_root_old"]


def test_a_misrouted_member_breaks_its_own_copy_alone(O):
    K, n_c, c, bad = 3, 5, 2, 3
    _, cent, mem, _, _ = case(O, "euclidean", K, n_c, c)
    noise = np.random.default_rng(7).integers(-3, 4, DIM)
    cent_f, mem_f = AA.data(60, K, n_c, c)
    mem_f[bad] = np.clip(cent_f[0] + noise, 0, 218)
    mem2 = O.quantize(mem_f, P)
    assert np.array_equal(np.delete(mem2, bad, axis=0), np.delete(mem, bad, axis=0))
    roots = index_roots(O, cent, [mem2 if j == c else cent[j:j + 1] for j in range(K)])
    m = AA.audit_model(O, "euclidean", cent, mem2, roots[:K + 1], c, P, L)
    cm, public, info, vals = built(m, "euclidean", K, n_c)
    assert m["routed"].tolist() == [1, 1, 1, 0, 1]
    assert broken_copies(cm, vals) == [m["own"][bad]] and cm.copy_of[m["own"][bad]] == m["m"][bad]
    rep = cm.check_witness(vals, TM.to_ints(m["lookup"]), m["flags"])
    assert rep.pop("copies_unequal") == 1 and not any(rep.values()), rep


def test_header_cluster_centroid_word_and_cluster_root_are_bound(O):
    K, n_c, c = 3, 5, 2
    m0, cent, mem, roots, index_root = case(O, "euclidean", K, n_c, c)
    # a header c' != c: the members are cluster c's, the selection picks cluster_root_c' -> picked = mroot breaks (and the members are not
    # nearest to centroid c', so their own = m copies break too)
    m = AA.audit_model(O, "euclidean", cent, mem, roots, 0, P, L)
    cm, _, info, vals = built(m, "euclidean", K, n_c)
    broken = broken_copies(cm, vals)
    assert m["mroot_cell"] in broken and set(broken) <= {m["mroot_cell"]} | set(m["own"])
    # one altered centroid word: croot = centroids_root breaks, nothing else does (the members stay nearest to centroid c)
    cent2 = cent.copy()
    cent2[0, 0] = O.fr_add(cent2[0, :1], O.fr_from_ints([1]))[0]
    m = AA.audit_model(O, "euclidean", cent2, mem, roots, c, P, L)
    cm, _, info, vals = built(m, "euclidean", K, n_c)
    assert broken_copies(cm, vals) == [m["croot_cell"]] and cm.copy_of[m["croot_cell"]] == 1
    # one altered cluster root (another cluster's): every copy holds, the index root is another
    roots2 = roots.copy()
    roots2[1] = O.fr_add(roots2[1:2], O.fr_from_ints([1]))[0]
    m = AA.audit_model(O, "euclidean", cent, mem, roots2, c, P, L)
    cm, public, info, vals = built(m, "euclidean", K, n_c)
    assert broken_copies(cm, vals) == [] and not np.array_equal(m["public"][0], index_root)
    # ... and cluster c's own root altered breaks picked = mroot
    roots2 = roots.copy()
    roots2[1 + c] = O.fr_add(roots2[1 + c:2 + c], O.fr_from_ints([1]))[0]
    m = AA.audit_model(O, "euclidean", cent, mem, roots2, c, P, L)
    cm, _, info, vals = built(m, "euclidean", K, n_c)
    assert broken_copies(cm, vals) == [m["mroot_cell"]]


@pytest.mark.parametrize("metric,want", [("euclidean", 281474976708194), ("manhattan", 281474976710656)])
def test_a_member_equidistant_from_two_centroids_is_accepted_under_either(O, metric, want):
    cent = O.quantize(np.asarray([[0, 0, 0, 0], [2, 0, 0, 0], [9, 9, 9, 9]], dtype=np.float64), P)
    mem = O.quantize(np.asarray([[1, 0, 0, 0]], dtype=np.float64), P)
    (d,) = AA.distances(O, metric, cent, mem, P, L)
    assert d[0] == d[1] == want and d[2] > want
    for c, ok in ((0, True), (1, True), (2, False)):
        roots = index_roots(O, cent, [mem if j == c else cent[j:j + 1] for j in range(3)])
        m = AA.audit_model(O, metric, cent, mem, roots[:4], c, P, L)
        cm, public, info, vals = built(m, metric, 3, 1)
        rep = cm.check_witness(vals, TM.to_ints(m["lookup"]), m["flags"])
        assert (not any(rep.values())) == ok, (c, rep)
        assert m["routed"].tolist() == [int(ok)]
        if not ok:
            assert broken_copies(cm, vals) == [m["own"][0]]


def _alone(O, what, a, b):
    """the offsets inside its block of the cells that distance(a, b) / qmin(a, b), emitted alone after its assigned operands, leaves
    unnoticed, each with alteration_model's reason"""
    c, s = O.Ctx(store=True, keygen=True), CS.Sym(P, L)
    if what == "distance":
        c.assign_witnesses(np.stack([a, b]))
        c.distance("euclidean", a, b, P=P, L=L)
        s.distance("euclidean", s.assign_witnesses(DIM), s.assign_witnesses(DIM))
    else:
        c.assign_witnesses(np.stack([a, b])[None])
        c.op("qmin", a, b, P=P, L=L)
        s.qmin(*s.assign_witnesses(2))
    assert c.err == 0
    n_in = 2 * DIM if what == "distance" else 2
    cm = CS._whole(s, n_in)
    vals = np.asarray(TM.to_ints(c.advice()), dtype=object)
    assert cm.n_cells == len(vals)
    free = AM.unnoticed(cm, vals, np.asarray(TM.to_ints(c.lookup()), dtype=object), [])
    return [(x - n_in, AM.explain(cm, vals, x)) for x in free]


@pytest.mark.parametrize("K,n_c,c", [(2, 2, 1), (1, 5, 0)])
def test_every_cell_altered_alone(O, K, n_c, c):
    m, cent, mem, roots, _ = case(O, "euclidean", K, n_c, c)
    cm, public, info, vals = built(m, "euclidean", K, n_c)
    free = sweep(f"ann audit euclidean K {K} n_c {n_c} c {c} dim {DIM}", cm, vals, TM.to_ints(m["lookup"]), public, L, m["flags"])
    lay = info["layout"]
    kinds = {}
    for x in free:
        if x < lay["update"]:
            kind = "head"
        elif x < lay["routed"]:
            kind = "assigned"
        elif x < lay["merkle_c"]:
            off = (x - lay["routed"]) % lay["per_member"]
            kind = "distance" if off < lay["chain_off"] else "qmin" if off < lay["pick_off"] else "pick"
        else:
            kind = "tree"
        kinds.setdefault(kind, []).append(x)
    print({k: len(v) for k, v in kinds.items()})
    assert set(kinds) <= {"head", "distance", "qmin"}, kinds
    tied = {x for pair in m["ties"] for x in pair}
    assert not tied & set(free)
    # the head keeps its one free inverse: indicator c's is_zero has a zero operand
    inv_c = lay["indicator"] + (8 + 12 * (c - 1) + 4 if c else 0) + 2
    assert kinds.get("head", []) == [inv_c] and AM.explain(cm, vals, inv_c) == AM.IS_ZERO_INVERSE
    # what the distance and qmin blocks leave free is what the same gadget, emitted alone on the same operands, leaves free: the same
    # offsets inside the block, for the same reason
    d_n, q_n, per = lay["units"]["db"].n, lay["units"]["qm"].n, lay["per_member"]
    v = O.Ctx(store=False, keygen=False)
    for i in range(n_c):
        d = [v.distance("euclidean", cent[j], mem[i], P=P, L=L) for j in range(K)]
        base = lay["routed"] + i * per
        for j in range(K):
            got = [(x - base - j * d_n, AM.explain(cm, vals, x)) for x in kinds.get("distance", []) if base + j * d_n <= x < base + (j + 1) * d_n]
            assert got == _alone(O, "distance", cent[j], mem[i]), (i, j)
        acc = d[0]
        for j in range(1, K):
            lo = base + lay["chain_off"] + (j - 1) * q_n
            got = [(x - lo, AM.explain(cm, vals, x)) for x in kinds.get("qmin", []) if lo <= x < lo + q_n]
            assert got == _alone(O, "qmin", acc, d[j]), (i, j)
            acc = v.op("qmin", acc, d[j], P=P, L=L)
    assert all(AM.explain(cm, vals, x) is not None for x in free)


def test_layout_refusals_and_exports():
    from halo2_vectordb_amd import _lib
    lib = _lib.load()
    for name in ("vdb_wit_ann_audit_size", "vdb_wit_ann_audit", "vdb_wit_ann_audit_dev"):
        assert hasattr(lib, name), name
    for K, n_c, dim in ((0, 1, 4), (1, 0, 4), (1, 1, 0)):
        with pytest.raises(ValueError):
            CS.ann_audit_layout("euclidean", K, n_c, dim, P, L)
    assert CS.ann_audit_instances(7, 0) == [7, 0]
