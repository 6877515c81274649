"""The shapes of tests/test_gpu_witness_shapes.py on the CPU: the batches, the facts each shape has to reach (witness_shapes_model restates
witness.hip's launch formulas), and the helpers that test leans on held to the cell-level models first — the values-only walk of a batch
against update_model, the one-update model of a batch's last block against the whole batch's, the models without their per-cell flag
pass against the models with it, and the finder of k-means' cluster-size chain against the oracle's stream."""
import numpy as np
import pytest

import ann_delete_model as AD
import ann_update_model as AU
import merkle_ops_model as MO
import merkle_update_model as MU
import topk_model as TM
import witness_shapes_model as WS

P = 48
W, D = 0, 1


def rows(seed, n, dim):
    return np.random.default_rng(seed).integers(0, 219, size=(n, dim)).astype(np.float64)


# ---------------------------------------------------------------------------------------------------------------- A: path updates
# name: (n, dim, grow)
PATH_CASES = {"m65_depth1": (2, 1, 0), "m300_depth2": (3, 1, 0), "m70_dim5": (4, 5, 0), "ops_m130_mixed_grow1": (6, 1, 1)}


def path_batch(name):
    """-> (indices, kinds or None)"""
    n, dim, grow = PATH_CASES[name]
    rng = np.random.default_rng(sum(name.encode()))
    if name == "m65_depth1":
        return [int(i) for i in rng.integers(0, 2, size=65)], None
    if name == "m300_depth2":                                 # 290 writes into the three rows, the insert at 3, then replacements of it among others
        return [int(i) for i in rng.integers(0, 3, size=290)] + [3, 3, 0, 3, 2, 3, 1, 3, 3, 2], None
    if name == "m70_dim5":
        return [int(i) for i in rng.integers(0, 4, size=70)], None
    lp = MU.padded(n)[0] << grow
    return [int(i) for i in rng.integers(0, lp, size=130)], [int(k) for k in rng.integers(0, 2, size=130)]


def path_reaches(name):
    """the facts of the case's row in the table; -> the facts"""
    n, dim, grow = PATH_CASES[name]
    idx, kinds = path_batch(name)
    depth = MU.padded(n)[1] + grow
    f = WS.path_update_facts(idx, kinds, depth, dim)
    m = f["m"]
    if name == "m65_depth1":
        assert m == 65 and depth == 1 and set(idx) == {0, 1}
        assert f["index_blocks"] == 2 and f["index_last"] == [64], "block 1 of k_mku_index holds exactly the update that writes the new root"
        assert f["level_waves"] == 3 and f["level_mixed_waves"] == [1], "wave 1 of k_mku_level holds updates 64 (side 0) and 0 .. 62 (side 1)"
        assert all(f["from_batch"][1:]) and not f["from_batch"][0]
    elif name == "m300_depth2":
        assert m == 300 and depth == 2 and idx.index(3) == 290 and idx[291:].count(3) >= 2 and set(idx[:290]) == {0, 1, 2}
        assert f["fill_trips"] == 2 and f["touchers_blocks"] == 3 and m * depth == 600
        assert f["index_blocks"] == 5 and f["level_mixed_waves"] == [4]
    elif name == "m70_dim5":
        assert m == f["w"] == 70 and f["nperm"] == 3 and f["w"] * f["nperm"] > 64 and 64 % f["nperm"]
        assert f["leaf_blocks"] == 4 and f["leaf_states_blocks"] == 2 and f["leaf_straddles"] == [21, 42], "a write's permutations in two blocks"
    else:
        assert name == "ops_m130_mixed_grow1" and m == 130 and grow == 1 and depth == 4
        assert 64 < f["w"] < m and m - f["w"] > 1 and f["nperm"] == 1 and f["leaf_blocks"] == 2 and f["leaf_states_blocks"] == 2
        assert kinds[:64].count(W) < 64, "a write in block 1 of the leaf kernels is not the write of the same number: starts[v] / write_of decide"
        assert f["late_deletes"] and f["index_blocks"] == 3 and max(idx) >= MU.padded(n)[0], "deletes in block 1 and up; slots of the grown half"
    return f


_PATH = {}


def path_case(O, name):
    """-> dict(n, dim, grow, idx, kinds, db, new, small / grown: the tree before the batch in the device layout, before and after growth,
    m: the model, after: the model's tree after the batch in the device layout); computed once and left unchanged"""
    if name not in _PATH:
        n, dim, grow = PATH_CASES[name]
        idx, kinds = path_batch(name)
        w = len(idx) if kinds is None else kinds.count(W)
        db, new = O.quantize(rows(n, n, dim), P), O.quantize(rows(n + 1, w, dim), P)
        small = MU.build_tree(O, db)
        tree = MO.grow_tree(O, small, grow)
        grown = MU.flat_levels(tree)
        m = MU.update_model(O, tree, idx, new) if kinds is None else MO.ops_model(O, tree, idx, kinds, new, grow)
        _PATH[name] = dict(n=n, dim=dim, grow=grow, idx=idx, kinds=kinds, db=db, new=new, small=MU.flat_levels(small), grown=grown, m=m, after=MU.flat_levels(tree))
    return _PATH[name]


@pytest.mark.parametrize("name", sorted(PATH_CASES))
def test_path_batches_reach_what_they_are_there_for(name):
    path_reaches(name)


def test_values_walk_is_update_models_public_values_and_tree(O):
    s = path_case(O, "m65_depth1")
    tree = MU.build_tree(O, s["db"])
    pub = MU.walk_values(O, tree, s["idx"], s["new"])
    assert pub.shape == (3 * 65 + 2, 4) and np.array_equal(pub, s["m"]["public"]) and np.array_equal(MU.flat_levels(tree), s["after"])
    # ... and at depth 2 with an insert
    s = path_case(O, "m300_depth2")
    tree = MU.build_tree(O, s["db"])
    assert np.array_equal(MU.walk_values(O, tree, s["idx"], s["new"]), s["m"]["public"]) and np.array_equal(MU.flat_levels(tree), s["after"])


def last_block_model(O, db, idx, new):
    """the last update's block of a batch without the batch's stream: the tree after the updates before it from the values-only walk,
    then update_model of the last update alone -> (the block's cells, its gate bits, the 3 m + 2 public values, the tree after the
    batch in the device layout)"""
    tree = MU.build_tree(O, db)
    head = MU.walk_values(O, tree, idx[:-1], new[:-1])
    one = MU.update_model(O, tree, idx[-1:], new[-1:])
    public = np.concatenate([head[:-1], one["public"][1:]])
    return one["advice"][one["n_in"]:], one["selectors"][one["n_in"]:], public, MU.flat_levels(tree)


@pytest.mark.parametrize("name", ["m65_depth1", "m70_dim5"])
def test_last_block_of_a_batch_is_the_one_update_model_after_the_walk(O, name):
    s = path_case(O, name)
    block, gates, public, after = last_block_model(O, s["db"], s["idx"], s["new"])
    m = s["m"]
    assert m["regions"][-1]["block"] == m["advice"].shape[0] - block.shape[0]
    assert np.array_equal(block, m["advice"][-block.shape[0]:]) and np.array_equal(gates, m["selectors"][-block.shape[0]:])
    assert np.array_equal(public, m["public"]) and np.array_equal(after, s["after"])


# ---------------------------------------------------------------------------------------------------------------- B, C: the index-root frame
# name: (K, c, n_c, dim); the batch comes from ann_batch
ANN_UPDATES = {"annu_m85": (3, 1, 2, 1), "K300_c0": (300, 0, 3, 1), "K300_c299": (300, 299, 3, 1)}
ANND = ("annd_m33", 3, 1, 40, 1)


def ann_batch(name):
    if name == "annu_m85":
        return [int(i) for i in np.random.default_rng(85).integers(0, 2, size=85)]
    if name.startswith("K300"):
        return [0, 3]
    rng = np.random.default_rng(33)
    return [int(rng.integers(0, 40 - j)) for j in range(33)]


def ann_reaches(name):
    if name == ANND[0]:
        _, K, c, n_c, dim = ANND
        slots = ann_batch(name)
        _, lasts = AD.simulate(n_c, slots)
        idx, kinds = [i for pair in zip(slots, lasts) for i in pair], [2, 1] * len(slots)
        depth = MU.padded(n_c)[1]
        f = WS.path_update_facts(idx, kinds, depth, dim)
        assert f["m"] == 66 and f["w"] == 0 and f["index_blocks"] == 2 and f["index_last"] == [64, 65] and kinds[64:] == [2, 1], "a carried and an emptied leading cell in block 1"
        assert AD.shrink_of(n_c, len(slots)) == 3 and depth == 6
        assert WS.frame_facts(K, c, 4 * len(slots) + 3)["public_blocks"] == 1, "k_annd_public's second block needs m >= 64: deliberately unreached"
        return f
    K, c, n_c, dim = ANN_UPDATES[name]
    slots = ann_batch(name)
    grow = AU.smallest_grow(n_c, AU.track_fill(slots, n_c))
    assert grow == 0
    f = dict(WS.path_update_facts(slots, None, MU.padded(n_c)[1], dim), **WS.frame_facts(K, c, 3 * len(slots) + 3))
    if name == "annu_m85":
        assert f["m"] == 85 and set(slots) == {0, 1} and 3 * f["m"] + 3 == 258 and f["public_blocks"] == 2 and f["public_last_block"] == 1
        assert f["index_blocks"] == 2 and K + 2 > 0, "the update block runs past 64 updates at a base that is not 0"
    else:
        assert f["header_blocks"] == 2 and f["indicator_blocks"] == 5 and f["c_block"] == (0 if c == 0 else 4)
        assert f["sponge_perms"] == 151 and f["sponge_blocks"] == 3 and slots == [0, 3] and n_c == 3
        if c == 0:
            assert WS.SMALL_INV == 260 and K > 260, "indicator 259 takes -1/259 from the table, indicator 260 goes through the inverse list"
    return f


@pytest.mark.parametrize("name", sorted(ANN_UPDATES) + [ANND[0]])
def test_index_batches_reach_what_they_are_there_for(name):
    ann_reaches(name)


_ANN = {}


def ann_case(O, name):
    """-> the dict test_gpu_ann_update._update_dev / test_gpu_ann_delete._delete_dev take (K, c, n_c, dim, grow, slots, new, ix["roots"], grown /
    before: the cluster's tree before the batch in the device layout) with m: the model and after: its tree after the batch.  The
    roots are K + 1 random field elements with the cluster's tree root at 1 + c.  The two long batches skip the models' per-cell
    flag pass; the GPU test holds their update blocks' flags to something else."""
    if name not in _ANN:
        K, c, n_c, dim = ANND[1:] if name == ANND[0] else ANN_UPDATES[name]
        slots = ann_batch(name)
        members = O.quantize(rows(90 + K, n_c, dim), P)
        tree = MU.build_tree(O, members)
        before = MU.flat_levels(tree)
        roots = O.quantize(rows(91 + K, K + 1, 1), P)[:, 0].copy()
        roots[1 + c] = tree[-1][0]
        s = dict(K=K, c=c, n_c=n_c, dim=dim, grow=0, slots=slots, ix=dict(roots=roots), grown=before, before=before)
        if name == ANND[0]:
            s["m"] = AD.delete_model(O, roots, c, tree, slots, block_flags=False)
        else:
            s["new"] = O.quantize(rows(92 + K, len(slots), dim), P)
            s["m"] = AU.update_model(O, roots, c, tree, slots, s["new"], 0, block_flags=name != "annu_m85")
        s["after"] = MU.flat_levels(tree)
        _ANN[name] = s
    return _ANN[name]


def test_models_without_the_flag_pass_are_the_models_with_it_outside_their_blocks(O):
    import ann_model as AN
    from test_ann_delete_cpu import case as delete_case
    from test_ann_update_cpu import CASES, case as update_case
    for kind in ("update", "delete"):
        if kind == "update":
            name = "replace_append_append_grow"
            ids, c, slots, grow = CASES[name]
            full, db, ids, _, new, ix, _ = update_case(O, name)
            tree = MO.grow_tree(O, MU.build_tree(O, AN.select_cluster(db, ids, c)[0]), grow)
            lean = AU.update_model(O, ix["roots"][:-1], c, tree, slots, new, grow, block_flags=False)
        else:
            sizes, c, slots = AD.SHAPES["last_repeat"]
            full, db, ids, _, ix, _ = delete_case(O, sizes, c, slots)
            tree = MU.build_tree(O, AN.select_cluster(db, ids, c)[0])
            lean = AD.delete_model(O, ix["roots"][:-1], c, tree, slots, block_flags=False)
            assert full["s"] == 2 and lean["flags"][full["regions"]["shrink"] + 1] == 2
        lo, hi = full["regions"]["update"], full["regions"]["new_roots"]
        for key in ("advice", "selectors", "public"):
            assert np.array_equal(lean[key], full[key]), (kind, key)
        assert lean["regions"] == full["regions"]
        outside = np.ones(full["flags"].shape[0], dtype=bool)
        outside[lo:hi] = False
        assert np.array_equal(lean["flags"][outside], full["flags"][outside]) and (full["flags"][lo:hi] & 2).any(), kind
        assert np.array_equal(lean["flags"][lo:hi] & 1, full["flags"][lo:hi] & 1), kind


# ---------------------------------------------------------------------------------------------------------------- D: chain_fold_wave
# name: (n, dim, K, I)
KMEANS = {"N577": (577, 1, 2, 1), "N520": (520, 2, 3, 2)}
KM_L = 9


def kmeans_reaches(name):
    n, dim, K, I = KMEANS[name]
    f = WS.chain_facts(n)
    if name == "N577":
        assert f["per"] == 10 and f["chunks"][0] == [8, 2] and f["last_live"] == 57 and f["lanes"][57] == (570, 577) and f["chunks"][57] == [7]
        assert all(lo == hi for lo, hi in f["lanes"][58:]), "lanes 58 .. 63 hold no step"
    else:
        assert f["per"] == 9 and f["chunks"][0] == [8, 1] and K * dim == 6 and I == 2, "six chains of k_km_sum at stride 4 D; the second iteration reads the first's centroids"
    assert f["per"] > WS.KM_PF
    return f


_KM = {}


def kmeans_case(O, name):
    """-> (quantized vectors, the oracle's context, centroids, indicators); computed once and left unchanged"""
    if name not in _KM:
        n, dim, K, I = KMEANS[name]
        qv = O.quantize(np.random.default_rng(n).random((n, dim)) + 0.05, P)
        c = O.Ctx(store=True, keygen=True)
        cent, ind = c.kmeans("manhattan", qv, K, I, P=P, L=KM_L)
        assert c.err == 0
        _KM[name] = (qv, c, cent, ind)
    return _KM[name]


@pytest.mark.parametrize("name", sorted(KMEANS))
def test_kmeans_shapes_reach_a_second_chunk(name):
    kmeans_reaches(name)


def test_sizes_chain_is_found_in_the_oracles_stream(O):
    n, dim, K, I = KMEANS["N577"]
    qv, c, cent, ind = kmeans_case(O, "N577")
    adv = c.advice()
    at = WS.sizes_chain(adv, c.selectors(), n, K, P)
    counts = [sum(1 for v in TM.to_ints(ind[:, k]) if v) for k in range(K)]
    assert sum(counts) >= n and all(counts)
    last = at + 4 * (n - 2) * K
    assert TM.to_ints(adv[[last + 4 * k + 3 for k in range(K)]]) == [cnt << P for cnt in counts], "the chain ends in the cluster sizes"
    # a small shape, where the chain's place is known from the blocks around it: [1.0, 0 | n per-vector blocks | chain | ...]
    n2, K2 = 6, 2
    qv2 = O.quantize(np.random.default_rng(6).random((n2, 1)) + 0.05, P)
    c2 = O.Ctx(store=True, keygen=True)
    c2.kmeans("manhattan", qv2, K2, 1, P=P, L=KM_L)
    at2 = WS.sizes_chain(c2.advice(), c2.selectors(), n2, K2, P)
    assert (at2 - 2) % n2 == 0 and (at - 2) % n == 0 and (at2 - 2) // n2 == (at - 2) // n, "the same per-vector block size at both shapes"
