"""The Merkle path-update circuit as a checker (pipeline.UpdateHotPath; include/vdb.h vdb_wit_merkle_update), cell for cell.

The oracle has `merkle_commitment` and `assign_witnesses`; `merkle_commitment` of ONE vector of length L is exactly one
clear / update / squeeze stream and returns H(v), so it defines every hash block of the circuit: the leaf hash (L = dim) and the node hash
(L = 2).  The bare GateChip calls between them come from templates over Python integers:

    assert_bit(b)                   [0, b, b, b]                                                          gate at cell 0
    select(a, b, sel)               topk_model.select
    inner_product(a, Constant(c))   [a_0, a_1, c_1, s_1, a_2, c_2, s_2, ...] when c_0 = 1, else [0, a_0, c_0, s_0, ...]
                                    gates at the first cell and at every s_i but the last

and the break points from topk_model.row_walk.  tests/test_merkle_update_cpu.py holds each template against the oracle's own cells.
The updates are applied one after the other in Python, on a tree of Python lists: nothing here knows how the GPU batches them.
"""
import numpy as np

from topk_model import R, row_walk, select, to_ints, to_limbs

ZERO = np.zeros(4, dtype=np.uint64)


def assert_bit(b):
    return [0, b, b, b], [1, 0, 0, 0]


def inner_product_const(a, consts):
    """gate.inner_product(a, Constant(consts)) -> (cells, gate bits, output)"""
    n = len(a)
    if n and consts[0] == 1:
        cells, s, i0, ng = [a[0]], a[0], 1, n - 1
    else:
        cells, s, i0, ng = [0], 0, 0, n
    gates = [1 if ng > 0 else 0]
    for gi, i in enumerate(range(i0, n), start=1):
        s = (s + a[i] * consts[i]) % R
        cells += [a[i], consts[i] % R, s]
        gates += [0, 0, 1 if gi < ng else 0]
    return cells, gates, s


def padded(n):
    lp = 1
    while lp < n:
        lp <<= 1
    return lp, lp.bit_length() - 1


def build_tree(O, db):
    """levels[l][i]: Montgomery limbs of node i of level l (level 0: the leaf digests, the padding leaves zero)"""
    n = db.shape[0]
    lp, depth = padded(n)
    leaves = O.poseidon_hash_many(db)
    levels = [[leaves[i].copy() if i < n else ZERO.copy() for i in range(lp)]]
    for _ in range(depth):
        prev = levels[-1]
        pairs = np.stack([np.stack([prev[2 * i], prev[2 * i + 1]]) for i in range(len(prev) // 2)])
        levels.append(list(O.poseidon_hash_many(pairs)))
    return levels


def walk_values(O, levels, indices, new_vectors):
    """The batch as values alone, for batches far beyond what update_model can trace cell by cell: the updates applied one after the
    other on the tree `levels` (build_tree's lists; updated in place), every digest from O.poseidon_hash_many, no cell.
    -> the 3 m + 2 public values [old root | idx, old leaf, new leaf per update | new root]"""
    m, depth = new_vectors.shape[0], len(levels) - 1
    assert depth >= 1 and m == len(indices) >= 1
    new_leaves = O.poseidon_hash_many(np.ascontiguousarray(new_vectors))
    pub = [levels[depth][0].copy()]
    for j in range(m):
        idx = int(indices[j])
        pub += [to_limbs([idx])[0], levels[0][idx].copy(), new_leaves[j].copy()]
        levels[0][idx] = new_leaves[j].copy()
        for l in range(depth):
            node = (idx >> l) & ~1
            levels[l + 1][node >> 1] = O.poseidon_hash_many(np.stack([levels[l][node], levels[l][node + 1]])[None])[0]
    return np.stack(pub + [levels[depth][0].copy()])


def flat_levels(levels):
    """the device layout: the levels one after the other, 2 lp entries, the last zero"""
    return np.stack([x for lv in levels for x in lv] + [ZERO])


def _hash_ctx(O, words):
    c = O.Ctx(store=True, keygen=True)
    out = c.merkle_commitment(np.stack(words)[None])
    assert c.err == 0
    return c, out


def update_model(O, levels, indices, new_vectors, plan_k=None):
    """The closure on the tree `levels` (build_tree; updated in place), slot indices[j] taking new_vectors[j] (m, dim, 4), in order.
    -> dict(advice, selectors, break_points, n_in, public (3 m + 2, 4), roots: [(old root, new root) per update], regions: per update
    dict(block, levels: first cell of every level, index), inputs: dict(old_leaf, bits, sibs) first cells)"""
    m, dim = new_vectors.shape[0], new_vectors.shape[1]
    lp, depth = len(levels[0]), len(levels) - 1
    assert depth >= 1 and m >= 1 and all(0 <= i < lp for i in indices)
    old_leaves, bits_all, sibs_all, blocks, roots, regions, pub = [], [], [], [], [], [], []
    n_in = m * (dim + 1 + 2 * depth)
    at = n_in
    for j in range(m):
        idx = int(indices[j])
        adv, sel = [], []

        def ctx(c):
            adv.append(c.advice())
            sel.append(c.selectors().astype(np.uint8) & 1)

        def ints(cells, gates):
            adv.append(to_limbs(cells))
            sel.append(np.asarray(gates, dtype=np.uint8))

        reg = dict(block=at, levels=[])
        c, new_leaf = _hash_ctx(O, list(new_vectors[j]))
        ctx(c)
        old_leaf = levels[0][idx].copy()
        cur_old, cur_new = old_leaf, new_leaf
        bits, sibs, path = [], [], [new_leaf]
        for l in range(depth):
            reg["levels"].append(at + sum(a.shape[0] for a in adv))
            node = idx >> l
            b, sib = node & 1, levels[l][node ^ 1].copy()
            bits.append(b)
            sibs.append(sib)
            (si,), (co,), (cn,) = to_ints(sib), to_ints(cur_old), to_ints(cur_new)
            ints(*assert_bit(b))
            cells, gates, lo = select(si, co, b)
            ints(cells, gates)
            cells, gates, ro = select(co, si, b)
            ints(cells, gates)
            c, cur_old = _hash_ctx(O, list(to_limbs([lo, ro])))
            ctx(c)
            cells, gates, ln = select(si, cn, b)
            ints(cells, gates)
            cells, gates, rn = select(cn, si, b)
            ints(cells, gates)
            c, cur_new = _hash_ctx(O, list(to_limbs([ln, rn])))
            ctx(c)
            path.append(cur_new)
        reg["index"] = at + sum(a.shape[0] for a in adv)
        cells, gates, idx_val = inner_product_const(bits, [1 << l for l in range(depth)])
        ints(cells, gates)
        assert idx_val == idx
        assert np.array_equal(cur_old, levels[depth][0]), "the old path must end in the tree's current root"
        for l in range(depth + 1):
            levels[l][idx >> l] = path[l].copy()
        roots.append((cur_old, cur_new))
        old_leaves.append(old_leaf)
        bits_all += bits
        sibs_all += sibs
        pub += [to_limbs([idx])[0], old_leaf, new_leaf]
        blocks.append((np.concatenate(adv), np.concatenate(sel)))
        at += blocks[-1][0].shape[0]
        regions.append(reg)
    advice = np.concatenate([np.ascontiguousarray(new_vectors).reshape(-1, 4), np.stack(old_leaves), to_limbs(bits_all), np.stack(sibs_all)] + [b[0] for b in blocks])
    selectors = np.concatenate([np.zeros(n_in, dtype=np.uint8)] + [b[1] for b in blocks])
    assert advice.shape[0] == selectors.shape[0] == at
    return dict(advice=advice, selectors=selectors, break_points=row_walk(selectors, plan_k) if plan_k is not None else None, n_in=n_in,
                public=np.stack([roots[0][0]] + pub + [roots[-1][1]]), roots=roots, regions=regions,
                inputs=dict(old_leaf=m * dim, bits=m * dim + m, sibs=m * dim + m + m * depth))
