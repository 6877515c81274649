"""The index update circuit as a checker (pipeline.AnnUpdateHotPath; include/vdb.h vdb_wit_ann_update), cell for cell, composed from bricks
the other models already have: header integers; topk_model's integer templates is_equal, select and select_by_indicator (indicator 0 is
the 8-cell is_zero form, the tail of is_equal's cells); merkle_ops_model.ops_model for the update block; Ctx.merkle_commitment of one
vector of K + 1 words for the two sponges, with ann_model._mark_constants for their constant bits; topk_model.row_walk for the break
points.  Nothing here knows how the GPU lays out its offset tables or work buffers.

    A  [c | centroids_root | cluster roots]         assigned
    B  ind_0 = is_zero(c); ind_j = is_equal(c, Constant(j))
    C  picked = select_by_indicator(cluster roots, ind)
    D  index_root_old = sponge([centroids_root | cluster roots])
    E  the update block on the cluster's tree (writes only)
    F  out_j = select(new cluster root, cluster_root_j, ind_j)
    G  index_root_new = sponge([centroids_root | out_j])
"""
import numpy as np

import ann_model as AN
import merkle_ops_model as MO
import merkle_update_model as MU
import topk_model as TM


def track_fill(indices, n_c):
    """the appends of a batch whose writes keep the members dense (a slot below the fill, or the fill itself) -> their count"""
    fill = n_c
    for s in indices:
        assert 0 <= s <= fill, "a write above the fill"
        fill += s == fill
    return fill - n_c


def smallest_grow(n_c, appends):
    (lp, _), g = MU.padded(n_c), 0
    while (lp << g) < n_c + appends:
        g += 1
    return g


def updated_database(db, ids, c, indices, new_vectors):
    """the database and ids after the batch: a replacement overwrites the row of the cluster's member at that slot, an append adds a
    row at the end of the database with cluster id c -> (db, ids)"""
    db, ids = db.copy(), np.asarray(ids).copy()
    members = list(np.flatnonzero(ids == c))
    for s, v in zip(indices, new_vectors):
        if s == len(members):
            members.append(db.shape[0])
            db, ids = np.concatenate([db, v[None]]), np.concatenate([ids, [c]])
        else:
            db[members[s]] = v
    return db, ids


class window_ints:
    """vals[i] for the cells of a few stretches [lo, hi) of a stream as canonical Python integers, the cells outside them left alone:
    what _mark_constants reads of a sponge without the whole stream being converted"""

    def __init__(self, advice, stretches):
        self.parts = [(lo, TM.to_ints(advice[lo:hi])) for lo, hi in stretches]

    def __getitem__(self, i):
        for lo, v in self.parts:
            if lo <= i < lo + len(v):
                return v[i - lo]
        raise IndexError(i)


def update_model(O, roots, c, tree, indices, new_vectors, grow=0, plan_k=None, block_flags=True):
    """The closure on `roots` (K + 1, 4) = [centroids' root | cluster roots] and the cluster's `tree` (lists per level, already grown;
    updated in place).  block_flags=False leaves the update block's flag bytes at their gate bits (the pass that reads the constant
    bits off every cell's integer takes most of the time of a long batch; the caller then holds that block's flags to something else)
    and reads the integers of the two sponges alone.  -> dict(advice, selectors, flags (the kernels' flag bytes: gate bit, constant bit), break_points, n_in, public
    (3 m + 3, 4), regions: first cell of each block, update: ops_model's dict, indicators, picked, outs, index_root_old, index_root_new)"""
    K, m = roots.shape[0] - 1, len(indices)
    assert 0 <= c < K
    track_fill(indices, _fill_of(tree))
    s = TM._Stream()
    r_int = TM.to_ints(roots)
    s.ints([c] + r_int, [0] * (K + 2))
    reg, cst = {"indicator": s.n}, []
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
    reg["select"] = s.n
    cells, gates, picked = TM.select_by_indicator(r_int[1:], ind)      # (its leading 0 is a constant of the map; the kernel does not flag it)
    s.ints(cells, gates)
    reg["sponge_old"] = s.n
    ctx = O.Ctx(store=True, keygen=True)
    root_old = ctx.merkle_commitment(roots[None])
    assert ctx.err == 0
    s.ctx(ctx)
    reg["update"] = s.n
    assert picked == TM.to_ints(tree[len(tree) - 1 - grow][0][None])[0], "the tree is not the cluster's"
    u = MO.ops_model(O, tree, indices, None, new_vectors, grow)
    s.adv.append(u["advice"]); s.sel.append(u["selectors"]); s.n += u["advice"].shape[0]
    (new_root,) = TM.to_ints(u["public"][-1][None])
    reg["new_roots"] = s.n
    outs = []
    for j in range(K):
        cells, gates, out = TM.select(new_root, r_int[1 + j], ind[j])
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
        flags[reg["update"]:reg["new_roots"]] = kernel_like_flags(u)
    public = np.concatenate([root_old[None], TM.to_limbs([c]), u["public"][1:-1], root_new[None]])
    return dict(advice=advice, selectors=sel, flags=flags, break_points=TM.row_walk(sel, plan_k) if plan_k is not None else None, n_in=K + 2,
                public=public, regions=reg, update=u, indicators=ind, picked=picked, outs=outs, index_root_old=root_old, index_root_new=root_new,
                new_cluster_root=u["public"][-1])


def _fill_of(tree):
    """the members of the cluster: the leaves before the first empty one (a leaf digest is never 0 for a vector)"""
    n = 0
    while n < len(tree[0]) and tree[0][n].any():
        n += 1
    assert not any(x.any() for x in tree[0][n:]), "the members are not dense"
    return n
