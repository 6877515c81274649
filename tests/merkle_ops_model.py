"""The extended Merkle update circuit as a checker (pipeline.UpdateHotPath(kinds, grow); include/vdb.h vdb_wit_merkle_update_ops and
vdb_merkle_tree_grow_dev), cell for cell: writes, deletes and a tree doubled `grow` times before the first update.

Every hash block is the stream of an oracle Ctx (merkle_update_model._hash_ctx), the GateChip calls between them are
merkle_update_model's templates.  What is new here is one cell and one block:

    ctx.load_constant(0)            [0]                      no gate; a fixed-column constant (a delete's new leaf, and Z_0)
    the growth block                [Z_0 | H(Z_l, Z_l), l = 0 .. depth - 2 | H(R_i, Z_{d+i}), i = 0 .. grow - 1]

with Z_l the digest of an empty subtree of height l and R_i the root after i doublings.  The updates are applied one after the other
on a tree of Python lists; nothing here knows how the GPU batches them or lays out its offset tables."""
import numpy as np

from merkle_update_model import ZERO, _hash_ctx, assert_bit, inner_product_const
from topk_model import row_walk, select, to_ints, to_limbs


def empty_digests(O, count):
    """Z_0 .. Z_{count-1} (Montgomery limbs) and the hash Ctx that made each Z_{l+1}"""
    z, ctxs = [ZERO.copy()], []
    for _ in range(count - 1):
        c, out = _hash_ctx(O, [z[-1], z[-1]])
        ctxs.append(c)
        z.append(out)
    return z, ctxs


def grow_tree(O, levels, grow):
    """vdb_merkle_tree_grow_dev on a tree of lists (merkle_update_model.build_tree): the padded leaf count doubled `grow` times, the new
    slots empty.  -> a new tree; `levels` is left as it is"""
    d = len(levels) - 1
    z, _ = empty_digests(O, d + grow + 1)
    lp = len(levels[0]) << grow
    out = []
    for l in range(d + grow + 1):
        width = lp >> l
        if l <= d:
            row = [x.copy() for x in levels[l]]
        else:
            row = [_hash_ctx(O, [out[l - 1][0], out[l - 1][1]])[1]]
        out.append(row + [z[l].copy() for _ in range(width - len(row))])
    return out


def ops_model(O, levels, indices, kinds, new_vectors, grow=0, plan_k=None):
    """The closure on the tree `levels` (already grown: depth d + grow; updated in place).  kinds[j]: 0 a write, 1 a delete (None: all
    writes); new_vectors (w, dim, 4): the rows of the writes in update order.
    -> dict(advice, selectors, constants: the single load_constant cells, perms: [(first cell, words absorbed)] of every permutation,
    break_points, n_in, public (3 m + 2, 4), regions: per update dict(block, new_leaf, levels, index), growth: dict(r0, z0, z: first
    cell of each Z hash, r: first cell of each R hash) or None)"""
    m = len(indices)
    kinds = [0] * m if kinds is None else [int(k) for k in kinds]
    dim = new_vectors.shape[1]
    lp, depth = len(levels[0]), len(levels) - 1
    d0 = depth - grow
    assert depth >= 1 and d0 >= 0 and m >= 1 and all(0 <= i < lp for i in indices) and set(kinds) <= {0, 1}
    w = kinds.count(0)
    assert new_vectors.shape[0] == w
    n_in = w * dim + m * (1 + 2 * depth) + (1 if grow else 0)
    adv, sel, constants, perms = [], [], [], []
    at = [n_in]

    def ctx(c, n_words):
        a = c.advice()
        # the sponge's permutations: every one but a padding-only last absorbs two words, an odd last one absorbs one
        pos, left = at[0], n_words
        while pos < at[0] + a.shape[0]:
            k = min(2, left)
            perms.append((pos, k))
            pos += (18 if k == 2 else 15 if k == 1 else 12) + 2238
            left -= k
        assert pos == at[0] + a.shape[0] and left == 0
        adv.append(a)
        sel.append(c.selectors().astype(np.uint8) & 1)
        at[0] += a.shape[0]

    def ints(cells, gates):
        adv.append(to_limbs(cells))
        sel.append(np.asarray(gates, dtype=np.uint8))
        at[0] += len(cells)

    def constant_zero():
        constants.append(at[0])
        ints([0], [0])
        return ZERO.copy()

    growth, r0, top = None, levels[d0][0].copy(), None
    if grow:
        growth = dict(r0=n_in - 1, z0=at[0], z=[], r=[])
        z = [constant_zero()]
        for l in range(depth - 1):
            growth["z"].append(at[0])
            c, out = _hash_ctx(O, [z[l], z[l]])
            ctx(c, 2)
            z.append(out)
        top = r0
        for i in range(grow):
            assert np.array_equal(levels[d0 + i][0], top) and np.array_equal(levels[d0 + i][1], z[d0 + i]), "the tree was not grown"
            growth["r"].append(at[0])
            c, top = _hash_ctx(O, [top, z[d0 + i]])
            ctx(c, 2)
        assert np.array_equal(top, levels[depth][0])

    old_leaves, bits_all, sibs_all, regions, pub, roots = [], [], [], [], [], []
    wn = 0
    for j in range(m):
        idx = int(indices[j])
        reg = dict(block=at[0], levels=[])
        if kinds[j]:
            reg["new_leaf"] = at[0]
            new_leaf = constant_zero()
        else:
            c, new_leaf = _hash_ctx(O, list(new_vectors[wn]))
            wn += 1
            ctx(c, dim)
            reg["new_leaf"] = None
        old_leaf = levels[0][idx].copy()
        cur_old, cur_new = old_leaf, new_leaf
        bits, path = [], [new_leaf]
        for l in range(depth):
            reg["levels"].append(at[0])
            node = idx >> l
            b, sib = node & 1, levels[l][node ^ 1].copy()
            bits.append(b)
            sibs_all.append(sib)
            (si,), (co,), (cn,) = to_ints(sib), to_ints(cur_old), to_ints(cur_new)
            ints(*assert_bit(b))
            cells, gates, lo = select(si, co, b)
            ints(cells, gates)
            cells, gates, ro = select(co, si, b)
            ints(cells, gates)
            c, cur_old = _hash_ctx(O, list(to_limbs([lo, ro])))
            ctx(c, 2)
            cells, gates, ln = select(si, cn, b)
            ints(cells, gates)
            cells, gates, rn = select(cn, si, b)
            ints(cells, gates)
            c, cur_new = _hash_ctx(O, list(to_limbs([ln, rn])))
            ctx(c, 2)
            path.append(cur_new)
        reg["index"] = at[0]
        cells, gates, idx_val = inner_product_const(bits, [1 << l for l in range(depth)])
        ints(cells, gates)
        assert idx_val == idx
        assert np.array_equal(cur_old, levels[depth][0]), "the old path must end in the tree's current root"
        for l in range(depth + 1):
            levels[l][idx >> l] = path[l].copy()
        roots.append((cur_old, cur_new))
        old_leaves.append(old_leaf)
        bits_all += bits
        pub += [to_limbs([idx])[0], old_leaf, new_leaf]
        regions.append(reg)
    inputs = [np.ascontiguousarray(new_vectors).reshape(-1, 4), np.stack(old_leaves), to_limbs(bits_all), np.stack(sibs_all)]
    if grow:
        inputs.append(r0[None])
    advice = np.concatenate(inputs + adv)
    selectors = np.concatenate([np.zeros(n_in, dtype=np.uint8)] + sel)
    assert advice.shape[0] == selectors.shape[0] == at[0]
    return dict(advice=advice, selectors=selectors, constants=constants, perms=perms,
                break_points=row_walk(selectors, plan_k) if plan_k is not None else None, n_in=n_in,
                public=np.stack([r0 if grow else roots[0][0]] + pub + [roots[-1][1]]), roots=roots, regions=regions, growth=growth)
