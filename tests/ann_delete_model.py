"""The index delete circuit as a checker (pipeline.AnnDeleteHotPath; include/vdb.h vdb_wit_ann_delete), cell for cell, composed from the
bricks the other models already have, in the way ann_update_model does it: header integers; topk_model's integer templates is_equal,
select and select_by_indicator; every hash block an oracle Ctx (merkle_update_model._hash_ctx); Ctx.merkle_commitment of one vector of
K + 1 words for the two sponges.  New here: the carried leaf (one plain witness cell where a delete has its constant 0) and block S.

    A - D  as ann_update_model
    E'     2 m path updates: update 2 j at slot_j with the leaf found at fill - 1 at that turn, update 2 j + 1 empties slot fill - 1
    S      [S_0 | Z_0 | H(Z_l, Z_l), l < d - 1 | H(S_i, Z_{d-s+i}), i < s]      only when the tree halves s >= 1 times
    F, G   as ann_update_model; F selects S_0 (s >= 1) or E''s final root

The deletes are applied one after the other on a tree of Python lists and on a plain list of members: nothing here tracks origins or
knows how the GPU lays out its tables."""
import numpy as np

import ann_model as AN
import merkle_update_model as MU
import topk_model as TM
from ann_update_model import window_ints
from merkle_update_model import ZERO, _hash_ctx, assert_bit, inner_product_const
from topk_model import select, to_ints, to_limbs

# name: (cluster sizes, c, slots)
SHAPES = {
    "shrink": ((5, 2, 3), 0, [1]),
    "last_repeat": ((5, 2, 3), 0, [4, 0, 0]),
    "flat": ((4, 2, 3), 0, [1]),
    "to_one": ((5, 2, 3), 1, [0]),
    "k1": ((3,), 0, [0]),
}


def ids_of(sizes):
    return np.repeat(np.arange(len(sizes)), sizes)


def simulate(n_c, slots):
    """the members of the cluster (by original slot) after the deletes, by brute force on a list -> (members, last_j per delete)"""
    members, last = list(range(n_c)), []
    assert 1 <= len(slots) < n_c, "the batch would empty the cluster"
    for s in slots:
        assert 0 <= s < len(members), "a slot at or above the fill"
        last.append(len(members) - 1)
        members[s] = members[-1]
        members.pop()
    return members, last


def shrink_of(n_c, m):
    return MU.padded(n_c)[1] - MU.padded(n_c - m)[1]


def compacted_database(db, ids, c, slots):
    """the database after the removal: the grouped rows in order, cluster c's in the arrangement the batch leaves -> (db, ids)"""
    ids = np.asarray(ids)
    K = int(ids.max()) + 1
    rows, out_ids = [], []
    for k in range(K):
        mem, _ = AN.select_cluster(db, ids, k)
        if k == c:
            mem = mem[simulate(mem.shape[0], slots)[0]]
        rows.append(mem)
        out_ids += [k] * mem.shape[0]
    return np.ascontiguousarray(np.concatenate(rows)), np.asarray(out_ids)


def path_ops_model(O, levels, slots):
    """block E' on the tree `levels` (lists per level; updated in place): per delete the carried update and the emptying one.
    -> merkle_ops_model.ops_model's dict (constants: the deletes' zero cells; carried: the carried-leaf cells), public (6 m + 2, 4)"""
    lp, depth = len(levels[0]), len(levels) - 1
    n_c = fill_of(levels)
    _, lasts = simulate(n_c, slots)
    indices, kinds = [], []
    for s, last in zip(slots, lasts):
        indices += [s, last]
        kinds += [2, 1]
    m = len(indices)
    n_in = m * (1 + 2 * depth)
    adv, sel, constants, carried, perms, at = [], [], [], [], [], [n_in]

    def ctx(c):
        a = c.advice()
        perms.append((at[0], 2))
        perms.append((at[0] + 18 + 2238, 0))
        assert a.shape[0] == 18 + 12 + 2 * 2238
        adv.append(a)
        sel.append(c.selectors().astype(np.uint8) & 1)
        at[0] += a.shape[0]

    def ints(cells, gates):
        adv.append(to_limbs(cells))
        sel.append(np.asarray(gates, dtype=np.uint8))
        at[0] += len(cells)

    old_leaves, bits_all, sibs_all, regions, pub, roots = [], [], [], [], [], []
    for j in range(m):
        idx = indices[j]
        reg = dict(block=at[0], levels=[], new_leaf=at[0])
        if kinds[j] == 2:
            new_leaf = levels[0][indices[j + 1]].copy()          # what sits at fill - 1 at this turn
            carried.append(at[0])
            adv.append(new_leaf[None]); sel.append(np.zeros(1, dtype=np.uint8)); at[0] += 1
        else:
            new_leaf = ZERO.copy()
            constants.append(at[0])
            ints([0], [0])
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
            ctx(c)
            cells, gates, ln = select(si, cn, b)
            ints(cells, gates)
            cells, gates, rn = select(cn, si, b)
            ints(cells, gates)
            c, cur_new = _hash_ctx(O, list(to_limbs([ln, rn])))
            ctx(c)
            path.append(cur_new)
        reg["index"] = at[0]
        cells, gates, idx_val = inner_product_const(bits, [1 << l for l in range(depth)])
        ints(cells, gates)
        assert idx_val == idx and np.array_equal(cur_old, levels[depth][0]), "the old path must end in the tree's current root"
        for l in range(depth + 1):
            levels[l][idx >> l] = path[l].copy()
        roots.append((cur_old, cur_new))
        old_leaves.append(old_leaf)
        bits_all += bits
        pub += [to_limbs([idx])[0], old_leaf, new_leaf]
        regions.append(reg)
    advice = np.concatenate([np.stack(old_leaves), to_limbs(bits_all), np.stack(sibs_all)] + adv)
    selectors = np.concatenate([np.zeros(n_in, dtype=np.uint8)] + sel)
    assert advice.shape[0] == selectors.shape[0] == at[0]
    return dict(advice=advice, selectors=selectors, constants=constants, carried=carried, perms=perms, n_in=n_in,
                public=np.stack([roots[0][0]] + pub + [roots[-1][1]]), roots=roots, regions=regions, indices=indices, kinds=kinds)


def fill_of(tree):
    """the members of the cluster: the leaves before the first empty one"""
    n = 0
    while n < len(tree[0]) and tree[0][n].any():
        n += 1
    assert not any(x.any() for x in tree[0][n:]), "the members are not dense"
    return n


def delete_model(O, roots, c, tree, slots, plan_k=None, block_flags=True):
    """The closure on `roots` (K + 1, 4) = [centroids' root | cluster roots] and the cluster's `tree` (lists per level; updated in place,
    kept at its old size).  block_flags=False leaves the flag bytes of blocks E' and S at their gate bits and reads the integers of the
    two sponges alone (ann_update_model.update_model).  -> dict(advice, selectors, flags, break_points, n_in, public (4 m + 3, 4),
    regions, update: path_ops_model's dict, indicators, picked, outs, s, s0, shrink_top, index_root_old, index_root_new,
    new_cluster_root, cut_tree: the tree cut to lp >> s)"""
    K, m = roots.shape[0] - 1, len(slots)
    assert 0 <= c < K
    depth = len(tree) - 1
    s = TM._Stream()
    r_int = TM.to_ints(roots)
    s.ints([c] + r_int, [0] * (K + 2))
    reg, cst = {"indicator": s.n}, []
    ind = []
    for j in range(K):
        cells, gates, z = TM.is_equal(c, j)
        if j == 0:
            cells, gates = cells[4:], gates[4:]
            cst += [s.n + 3, s.n + 4, s.n + 7]
        else:
            cst += [s.n + 1, s.n + 2, s.n + 7, s.n + 8, s.n + 11]
        s.ints(cells, gates)
        ind.append(z)
    reg["select"] = s.n
    cells, gates, picked = TM.select_by_indicator(r_int[1:], ind)
    s.ints(cells, gates)
    reg["sponge_old"] = s.n
    ctx = O.Ctx(store=True, keygen=True)
    root_old = ctx.merkle_commitment(roots[None])
    assert ctx.err == 0
    s.ctx(ctx)
    reg["update"] = s.n
    assert picked == TM.to_ints(tree[depth][0][None])[0], "the tree is not the cluster's"
    sh = shrink_of(fill_of(tree), m)
    u = path_ops_model(O, tree, slots)
    s.adv.append(u["advice"]); s.sel.append(u["selectors"]); s.n += u["advice"].shape[0]
    new_root = u["public"][-1]
    reg["shrink"] = s.n
    s0 = top = None
    if sh:
        s0 = top = tree[depth - sh][0].copy()
        cst.append(s.n + 1)
        s.ints(TM.to_ints(s0[None]) + [0], [0, 0])
        z = [ZERO.copy()]
        for l in range(depth - 1):
            cx, out = _hash_ctx(O, [z[l], z[l]])
            s.ctx(cx)
            z.append(out)
        for i in range(sh):
            cx, top = _hash_ctx(O, [top, z[depth - sh + i]])
            s.ctx(cx)
        new_root = s0
    (nr,) = TM.to_ints(new_root[None])
    reg["new_roots"] = s.n
    outs = []
    for j in range(K):
        cells, gates, out = TM.select(nr, r_int[1 + j], ind[j])
        cst.append(s.n + 1)
        s.ints(cells, gates)
        outs.append(out)
    reg["sponge_new"] = s.n
    words = np.concatenate([roots[:1], TM.to_limbs(outs)])
    ctx = O.Ctx(store=True, keygen=True)
    root_new = ctx.merkle_commitment(words[None])
    assert ctx.err == 0
    s.ctx(ctx)
    advice, sel = np.concatenate(s.adv), np.concatenate(s.sel) & 1
    assert advice.shape[0] == sel.shape[0] == s.n
    flags = sel.copy()
    vals = TM.to_ints(advice) if block_flags else window_ints(advice, [(reg["sponge_old"], reg["update"]), (reg["sponge_new"], s.n)])
    flags[cst] |= 2
    assert AN._mark_constants(flags, vals, reg["sponge_old"], K + 1) == reg["update"]
    assert AN._mark_constants(flags, vals, reg["sponge_new"], K + 1) == s.n
    if block_flags:
        from test_merkle_ops_cpu import kernel_like_flags
        flags[reg["update"]:reg["shrink"]] = kernel_like_flags(u)
    if sh and block_flags:                                       # block S's hashes: the constants of their permutations, as the update block's
        hashes = dict(advice=advice[reg["shrink"]:reg["new_roots"]], selectors=sel[reg["shrink"]:reg["new_roots"]], constants=[1],
                      perms=[(2 + h * 4506 + k * (18 + 2238), 2 - 2 * k) for h in range(depth - 1 + sh) for k in range(2)])
        flags[reg["shrink"]:reg["new_roots"]] = kernel_like_flags(hashes)
    up = u["public"]
    per = [np.stack([up[1 + 6 * j], up[2 + 6 * j], up[4 + 6 * j], up[3 + 6 * j]]) for j in range(m)]
    public = np.concatenate([root_old[None], TM.to_limbs([c])] + per + [root_new[None]])
    cut = [[x.copy() for x in tree[l][:len(tree[l]) >> sh]] for l in range(depth - sh + 1)]
    return dict(advice=advice, selectors=sel, flags=flags, break_points=TM.row_walk(sel, plan_k) if plan_k is not None else None, n_in=K + 2,
                public=public, regions=reg, update=u, indicators=ind, picked=picked, outs=outs, s=sh, s0=s0, shrink_top=top,
                index_root_old=root_old, index_root_new=root_new, new_cluster_root=new_root, cut_tree=cut)

