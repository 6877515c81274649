"""The index move circuit as a checker (pipeline.AnnMoveHotPath; include/vdb.h vdb_wit_ann_move), cell for cell, composed from the bricks
the other models already have, in the way ann_delete_model does it: header integers; topk_model's integer templates is_equal, select and
select_by_indicator; every hash block an oracle Ctx (merkle_update_model._hash_ctx); Ctx.merkle_commitment of one vector of K + 1 words
for the two sponges.  New here: a second indicator block over the roots after the removal, and an append whose new leaf is carried.

    A          [a | b | centroids_root | cluster roots]
    B_a, C_a   ind_a = idx_to_indicator(a, K); picked_a = select_by_indicator(cluster roots, ind_a)
    D          index_root_old = sponge([centroids_root | cluster roots])
    E', S      ann_delete_model's blocks on a's tree (path_ops_model, and block S when the tree halves)
    F_a        mid_j = select(a's new root, cluster_root_j, ind_a_j)
    B_b, C_b   ind_b = idx_to_indicator(b, K); picked_b = select_by_indicator(mid, ind_b)
    E_b        m appends at n_b + j on b's grown tree, each new leaf ONE witness cell holding the leaf move j took out of a
    F_b        out_j = select(b's new root, mid_j, ind_b_j)
    G          index_root_new = sponge([centroids_root | out_j])

The moves are applied one after the other on two trees of Python lists and two lists of members: nothing here tracks origins or knows
how the GPU lays out its tables."""
import numpy as np

import ann_delete_model as AD
import ann_model as AN
import merkle_ops_model as MO
import merkle_update_model as MU
import topk_model as TM
from merkle_update_model import ZERO, _hash_ctx, assert_bit, inner_product_const
from topk_model import select, to_ints, to_limbs

# name: (cluster sizes, a, b, slots)
SHAPES = {
    "shrink_grow": ((5, 4, 3), 0, 1, [1]),
    "flat": ((4, 3, 2), 0, 1, [0]),
    "repeat": ((5, 2), 0, 1, [4, 0, 0]),
    "to_one": ((2, 1), 0, 1, [0]),
    "backwards": ((3, 4, 5), 2, 0, [0, 2]),
}


def simulate(n_a, n_b, slots):
    """the members of the two clusters after the moves, by brute force on two lists: a's by original slot, b's as ("b", slot) for its
    own and ("a", original slot) for the arrivals -> (members of a, members of b, last_j per move)"""
    mem_a, mem_b, last = list(range(n_a)), [("b", i) for i in range(n_b)], []
    assert 1 <= len(slots) < n_a, "the batch would empty the source cluster"
    assert n_b >= 1
    for s in slots:
        assert 0 <= s < len(mem_a), "a slot at or above the fill"
        last.append(len(mem_a) - 1)
        mem_b.append(("a", mem_a[s]))
        mem_a[s] = mem_a[-1]
        mem_a.pop()
    return mem_a, mem_b, last


def shape_of(n_a, n_b, m):
    """(d_a, s, d_b of the grown tree, g)"""
    d_a, d_b0 = MU.padded(n_a)[1], MU.padded(n_b)[1]
    return d_a, d_a - MU.padded(n_a - m)[1], MU.padded(n_b + m)[1], MU.padded(n_b + m)[1] - d_b0


def moved_grouping(db, ids, a, b, slots):
    """the index after the moves over the SAME database: the grouped rows in order with a's members in the arrangement the batch leaves
    and the arrivals behind b's -> (grouped rows, their nondecreasing ids, the database slot of every grouped row)"""
    ids = np.asarray(ids)
    K = int(ids.max()) + 1
    parts = [AN.select_cluster(db, ids, k)[1] for k in range(K)]
    mem_a, mem_b, _ = simulate(len(parts[a]), len(parts[b]), slots)
    new = list(parts)
    new[a] = parts[a][mem_a]
    new[b] = np.asarray([parts[b][i] if w == "b" else parts[a][i] for w, i in mem_b])
    slots2 = np.concatenate(new).astype(np.int64)
    return np.ascontiguousarray(db[slots2]), np.repeat(np.arange(K), [len(x) for x in new]), slots2


def append_model(O, levels, indices, leaves, grow):
    """block E_b on the grown tree `levels` (lists per level; updated in place): update j writes the carried digest leaves[j] to slot
    indices[j].  merkle_ops_model.ops_model with ONE plain witness cell where a write has its leaf sponge.
    -> ops_model's dict, with carried: the carried-leaf cells"""
    m = len(indices)
    lp, depth = len(levels[0]), len(levels) - 1
    d0 = depth - grow
    assert depth >= 1 and d0 >= 0 and m >= 1 and all(0 <= i < lp for i in indices)
    n_in = m * (1 + 2 * depth) + (1 if grow else 0)
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

    growth, r0 = None, levels[d0][0].copy()
    if grow:
        growth = dict(r0=n_in - 1, z0=at[0], z=[], r=[])
        constants.append(at[0])
        ints([0], [0])
        z = [ZERO.copy()]
        for l in range(depth - 1):
            growth["z"].append(at[0])
            c, out = _hash_ctx(O, [z[l], z[l]])
            ctx(c)
            z.append(out)
        top = r0
        for i in range(grow):
            assert np.array_equal(levels[d0 + i][0], top) and np.array_equal(levels[d0 + i][1], z[d0 + i]), "the tree was not grown"
            growth["r"].append(at[0])
            c, top = _hash_ctx(O, [top, z[d0 + i]])
            ctx(c)
        assert np.array_equal(top, levels[depth][0])
    old_leaves, bits_all, sibs_all, regions, pub, roots = [], [], [], [], [], []
    for j in range(m):
        idx = int(indices[j])
        reg = dict(block=at[0], levels=[], new_leaf=at[0])
        new_leaf = np.asarray(leaves[j], dtype=np.uint64).copy()
        carried.append(at[0])
        adv.append(new_leaf[None]); sel.append(np.zeros(1, dtype=np.uint8)); at[0] += 1
        old_leaf = levels[0][idx].copy()
        cur_old, cur_new = old_leaf, new_leaf
        bits, path = [], [new_leaf]
        for l in range(depth):
            reg["levels"].append(at[0])
            node = idx >> l
            bit, sib = node & 1, levels[l][node ^ 1].copy()
            bits.append(bit)
            sibs_all.append(sib)
            (si,), (co,), (cn,) = to_ints(sib), to_ints(cur_old), to_ints(cur_new)
            ints(*assert_bit(bit))
            cells, gates, lo = select(si, co, bit)
            ints(cells, gates)
            cells, gates, ro = select(co, si, bit)
            ints(cells, gates)
            c, cur_old = _hash_ctx(O, list(to_limbs([lo, ro])))
            ctx(c)
            cells, gates, ln = select(si, cn, bit)
            ints(cells, gates)
            cells, gates, rn = select(cn, si, bit)
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
    inputs = [np.stack(old_leaves), to_limbs(bits_all), np.stack(sibs_all)] + ([r0[None]] if grow else [])
    advice = np.concatenate(inputs + adv)
    selectors = np.concatenate([np.zeros(n_in, dtype=np.uint8)] + sel)
    assert advice.shape[0] == selectors.shape[0] == at[0]
    return dict(advice=advice, selectors=selectors, constants=constants, carried=carried, perms=perms, n_in=n_in,
                public=np.stack([r0 if grow else roots[0][0]] + pub + [roots[-1][1]]), roots=roots, regions=regions, growth=growth)


def _indicators(s, cst, c, K):
    """idx_to_indicator(c, K) as select_from_idx unrolls it, appended to the stream -> the indicator integers"""
    ind = []
    for j in range(K):
        cells, gates, z = TM.is_equal(c, j)
        if j == 0:
            cells, gates = cells[4:], gates[4:]              # the unrolled is_zero(c): [z, c, inv, 1, 0, c, z, 0]
            cst += [s.n + 3, s.n + 4, s.n + 7]
        else:
            cst += [s.n + 1, s.n + 2, s.n + 7, s.n + 8, s.n + 11]
        s.ints(cells, gates)
        ind.append(z)
    return ind


def _selects(s, cst, new_root, olds, ind):
    outs = []
    for j in range(len(ind)):
        cells, gates, out = TM.select(new_root, olds[j], ind[j])
        cst.append(s.n + 1)
        s.ints(cells, gates)
        outs.append(out)
    return outs


def move_model(O, roots, a, b, tree_a, tree_b, slots, plan_k=None, same_cluster=False):
    """The closure on `roots` (K + 1, 4) = [centroids' root | cluster roots], a's `tree_a` (lists per level; updated in place, kept at
    its old size) and b's GROWN `tree_b` (updated in place).  same_cluster: a == b is admitted and tree_b is ignored: E_b runs on the
    tree E' and S leave, cut and grown, as a prover composing the two blocks sequentially would have it.
    -> dict(advice, selectors, flags, break_points, n_in, public (6 m + 4, 4), regions, delete / append: the two update blocks' dicts,
    indicators, indicators_b, picked, picked_b, mids, outs, s, g, s0, shrink_top, index_root_old, index_root_new, new_root_a, new_root_b,
    cut_tree: a's tree cut to lp >> s, tree_b)"""
    from test_merkle_ops_cpu import kernel_like_flags
    K, m = roots.shape[0] - 1, len(slots)
    assert 0 <= a < K and 0 <= b < K and (a != b or same_cluster)
    depth = len(tree_a) - 1
    s = TM._Stream()
    r_int = TM.to_ints(roots)
    s.ints([a, b] + r_int, [0] * (K + 3))
    reg, cst = {"indicator": s.n}, []
    ind = _indicators(s, cst, a, K)
    reg["select"] = s.n
    cells, gates, picked = TM.select_by_indicator(r_int[1:], ind)
    s.ints(cells, gates)
    reg["sponge_old"] = s.n
    ctx = O.Ctx(store=True, keygen=True)
    root_old = ctx.merkle_commitment(roots[None])
    assert ctx.err == 0
    s.ctx(ctx)
    reg["update"] = s.n
    assert picked == TM.to_ints(tree_a[depth][0][None])[0], "the tree is not cluster a's"
    n_a = AD.fill_of(tree_a)
    sh = AD.shrink_of(n_a, m)
    u = AD.path_ops_model(O, tree_a, slots)
    s.adv.append(u["advice"]); s.sel.append(u["selectors"]); s.n += u["advice"].shape[0]
    removed = [u["public"][2 + 6 * j].copy() for j in range(m)]      # the old leaf of update 2 j: what move j takes out of a
    new_root_a = u["public"][-1]
    reg["shrink"] = s.n
    s0 = top = None
    if sh:
        s0 = top = tree_a[depth - sh][0].copy()
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
        new_root_a = s0
    cut = [[x.copy() for x in tree_a[l][:len(tree_a[l]) >> sh]] for l in range(depth - sh + 1)]
    reg["mid"] = s.n
    mids = _selects(s, cst, TM.to_ints(new_root_a[None])[0], r_int[1:], ind)
    reg["indicator_b"] = s.n
    ind_b = _indicators(s, cst, b, K)
    reg["select_b"] = s.n
    cells, gates, picked_b = TM.select_by_indicator(mids, ind_b)
    s.ints(cells, gates)
    reg["update_b"] = s.n
    if same_cluster:
        g = MU.padded(n_a)[1] - MU.padded(n_a - m)[1]            # the cut tree grown back to hold its m members again
        tree_b = MO.grow_tree(O, cut, g)
        n_b = n_a - m
    else:
        n_b = AD.fill_of(tree_b) if len(tree_b) > 1 else 1
        g = MU.padded(n_b + m)[1] - MU.padded(n_b)[1]
    depth_b = len(tree_b) - 1
    assert picked_b == TM.to_ints(tree_b[depth_b - g][0][None])[0], "the tree is not cluster b's"
    ub = append_model(O, tree_b, [n_b + j for j in range(m)], removed, g)
    s.adv.append(ub["advice"]); s.sel.append(ub["selectors"]); s.n += ub["advice"].shape[0]
    new_root_b = ub["public"][-1]
    reg["new_roots"] = s.n
    outs = _selects(s, cst, TM.to_ints(new_root_b[None])[0], mids, ind_b)
    reg["sponge_new"] = s.n
    words = np.concatenate([roots[:1], TM.to_limbs(outs)])
    ctx = O.Ctx(store=True, keygen=True)
    root_new = ctx.merkle_commitment(words[None])
    assert ctx.err == 0
    s.ctx(ctx)
    advice, sel = np.concatenate(s.adv), np.concatenate(s.sel) & 1
    assert advice.shape[0] == sel.shape[0] == s.n
    flags = sel.copy()
    vals = TM.to_ints(advice)
    flags[cst] |= 2
    assert AN._mark_constants(flags, vals, reg["sponge_old"], K + 1) == reg["update"]
    assert AN._mark_constants(flags, vals, reg["sponge_new"], K + 1) == s.n
    flags[reg["update"]:reg["shrink"]] = kernel_like_flags(u)
    if sh:
        hashes = dict(advice=advice[reg["shrink"]:reg["mid"]], selectors=sel[reg["shrink"]:reg["mid"]], constants=[1],
                      perms=[(2 + h * 4506 + k * (18 + 2238), 2 - 2 * k) for h in range(depth - 1 + sh) for k in range(2)])
        flags[reg["shrink"]:reg["mid"]] = kernel_like_flags(hashes)
    flags[reg["update_b"]:reg["new_roots"]] = kernel_like_flags(ub)
    up, upb = u["public"], ub["public"]
    per = [np.stack([up[1 + 6 * j], up[2 + 6 * j], up[4 + 6 * j], up[3 + 6 * j], upb[1 + 3 * j], upb[2 + 3 * j]]) for j in range(m)]
    public = np.concatenate([root_old[None], TM.to_limbs([a, b])] + per + [root_new[None]])
    return dict(advice=advice, selectors=sel, flags=flags, break_points=TM.row_walk(sel, plan_k) if plan_k is not None else None, n_in=K + 3,
                public=public, regions=reg, delete=u, append=ub, indicators=ind, indicators_b=ind_b, picked=picked, picked_b=picked_b, mids=mids,
                outs=outs, s=sh, g=g, s0=s0, shrink_top=top, index_root_old=root_old, index_root_new=root_new, new_root_a=new_root_a,
                new_root_b=new_root_b, cut_tree=cut, tree_b=tree_b, removed=removed)
