"""The linked write circuit as a checker (pipeline.AnnWriteHotPath; include/vdb.h vdb_wit_ann_write), cell for cell, composed from the
bricks the other models already have: ann_update_model's blocks A - D, E, F, G (header integers, topk_model's templates,
merkle_ops_model.ops_model for E, Ctx.merkle_commitment for the two sponges) and, between E and F, ann_move_model.append_model on the
database tree: m updates whose new leaf is ONE carried witness cell (an occupied slot is a replacement, an empty one an append), every
hash block an oracle Ctx.

    A - D  as ann_update_model
    E      the update block on the cluster's tree, dim words a row
    E_db   the update block on the database tree: update j writes the digest E's update j hashed to slot db_idx_j
    F, G   as ann_update_model, over E's final root

The writes are applied one after the other on two trees of Python lists and a list of the members' database slots: nothing here knows
how the GPU lays out its tables."""
import numpy as np

import ann_model as AN
import ann_move_model as AMV
import ann_update_model as AU
import merkle_ops_model as MO
import merkle_update_model as MU
import topk_model as TM

# name: (cluster sizes, c, slots in the cluster).  Between them: g_c = 0 and >= 1, g_db = 0 and >= 1 independently, an append that is
# then replaced (its database slot comes from the batch), a slot written twice, K = 1, c = K - 1, a replacement whose database slot is
# not its cluster slot (every cluster but the first of interleaved ids)
SHAPES = {
    "flat": ((3, 2), 0, [1]),                    # g_c = 0, g_db = 0: one replacement
    "both_grow": ((2, 2), 0, [2]),               # g_c = 1, g_db = 1: one append
    "cluster_grows": ((2, 3), 0, [2, 0]),        # g_c = 1, g_db = 0 (5 -> 6 rows under 8 leaves)
    "db_grows": ((3, 1), 0, [3]),                # g_c = 0 (3 -> 4 under 4 leaves), g_db = 1 (4 -> 5)
    "append_then_replace": ((2, 3), 1, [3, 3, 1, 1]),   # c = K - 1; the appended member replaced; slot 1 written twice
    "one_cluster": ((3,), 0, [0, 3]),            # K = 1
}


def interleaved_ids(sizes):
    """cluster ids over sum(sizes) database rows dealt round-robin, so that a member's database slot is not its cluster slot"""
    left, ids = list(sizes), []
    while any(left):
        for k in range(len(sizes)):
            if left[k]:
                left[k] -= 1
                ids.append(k)
    return np.asarray(ids, dtype=np.int64)


def db_indices(cluster_slots, indices, n_db):
    """the database slot of every write, by brute force on the list of the members' slots -> (db_idx, appends)"""
    place, out = [int(x) for x in cluster_slots], []
    n_c = len(place)
    for s in indices:
        assert 0 <= s <= len(place), "a write above the fill"
        if s == len(place):
            place.append(n_db + len(place) - n_c)
        out.append(place[s])
    return out, len(place) - n_c


def shape_of(n_c, n_db, appends):
    """(depth of the cluster's grown tree, g_c, depth of the grown database tree, g_db)"""
    d_c, d_db = MU.padded(n_c)[1], MU.padded(n_db)[1]
    return MU.padded(n_c + appends)[1], MU.padded(n_c + appends)[1] - d_c, MU.padded(n_db + appends)[1], MU.padded(n_db + appends)[1] - d_db


def write_model(O, roots, c, tree, tree_db, indices, db_idx, new_vectors, grow=0, grow_db=0, plan_k=None, carried=None, block_flags=True):
    """The closure on `roots` (K + 1, 4) = [centroids' root | cluster roots], the cluster's GROWN `tree` and the GROWN database tree
    `tree_db` (lists per level; both updated in place).  carried: digests E_db carries in place of E's new leaves (a prover who breaks
    the tie).  block_flags=False leaves the flag bytes of E and E_db at their gate bits (the pass that reads the constant bits off every
    cell takes most of the time of a long batch).  -> dict(advice, selectors, flags, break_points, n_in, public (4 m + 5, 4), regions,
    update / update_db: the two blocks' dicts, indicators, picked, outs, index_root_old, index_root_new, database_root_old,
    database_root_new)"""
    from test_merkle_ops_cpu import kernel_like_flags
    K, m = roots.shape[0] - 1, len(indices)
    assert 0 <= c < K and len(db_idx) == m
    AU.track_fill(indices, AU._fill_of(tree))
    s = TM._Stream()
    r_int = TM.to_ints(roots)
    s.ints([c] + r_int, [0] * (K + 2))
    reg, cst = {"indicator": s.n}, []
    ind = AMV._indicators(s, cst, c, K)
    reg["select"] = s.n
    cells, gates, picked = TM.select_by_indicator(r_int[1:], ind)
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
    reg["update_db"] = s.n
    leaves = [u["public"][3 + 3 * j].copy() for j in range(m)] if carried is None else carried
    udb = AMV.append_model(O, tree_db, db_idx, leaves, grow_db)
    s.adv.append(udb["advice"]); s.sel.append(udb["selectors"]); s.n += udb["advice"].shape[0]
    reg["new_roots"] = s.n
    outs = AMV._selects(s, cst, new_root, r_int[1:], ind)
    reg["sponge_new"] = s.n
    words = np.concatenate([roots[:1], TM.to_limbs(outs)])
    ctx = O.Ctx(store=True, keygen=True)
    root_new = ctx.merkle_commitment(words[None])
    assert ctx.err == 0
    s.ctx(ctx)
    advice, sel = np.concatenate(s.adv), np.concatenate(s.sel) & 1
    assert advice.shape[0] == sel.shape[0] == s.n
    flags = sel.copy()
    vals = AU.window_ints(advice, [(reg["sponge_old"], reg["update"]), (reg["sponge_new"], s.n)])
    flags[cst] |= 2
    assert AN._mark_constants(flags, vals, reg["sponge_old"], K + 1) == reg["update"]
    assert AN._mark_constants(flags, vals, reg["sponge_new"], K + 1) == s.n
    if block_flags:
        flags[reg["update"]:reg["update_db"]] = kernel_like_flags(u)
        flags[reg["update_db"]:reg["new_roots"]] = kernel_like_flags(udb)
    up, upd = u["public"], udb["public"]
    per = [np.stack([up[1 + 3 * j], upd[1 + 3 * j], up[2 + 3 * j], up[3 + 3 * j]]) for j in range(m)]
    public = np.concatenate([upd[:1], root_old[None], TM.to_limbs([c])] + per + [upd[-1:], root_new[None]])
    return dict(advice=advice, selectors=sel, flags=flags, break_points=TM.row_walk(sel, plan_k) if plan_k is not None else None, n_in=K + 2,
                public=public, regions=reg, update=u, update_db=udb, indicators=ind, picked=picked, outs=outs, index_root_old=root_old,
                index_root_new=root_new, database_root_old=upd[0], database_root_new=upd[-1], new_cluster_root=up[-1])
