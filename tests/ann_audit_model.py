"""The audit of one cluster's routing as a checker (pipeline.AnnAuditHotPath; include/vdb.h vdb_wit_ann_audit), cell for cell, in the manner
of ann_model.query_model: the head [header | indicators | selection | sponge] as ann_update_model.update_model states it (topk_model's
integer templates, Ctx.merkle_commitment of one vector of K + 1 words), oracle contexts for every distance and every qmin,
topk_model.select_by_indicator over Python integers for the pick, ann_model._merkle / _mark_constants for the two trees.

    A  [c | centroids_root | cluster roots]         assigned
    B  ind_0 = is_zero(c); ind_j = is_equal(c, Constant(j))
    C  picked = select_by_indicator(cluster roots, ind)
    D  index_root = sponge([centroids_root | cluster roots])
    I  [centroids | members]                        assigned
    R  per member i: d_ij = distance(centroid_j, member_i); m_i = the qmin chain; own_i = select_by_indicator(d_i, ind)   own_i <-> m_i
    MC croot = merkle_commitment(centroids)         croot <-> centroids_root
    MM mroot = merkle_commitment(members)           mroot <-> picked
"""
import numpy as np

import ann_model as AN
import topk_model as TM


def data(seed, K, n_c, c, dim=4):
    """the issue's recipe: centroids on the SIFT-like grid, the members of cluster c within 3 of their centroid -> (cent, members) f64"""
    rng = np.random.default_rng(seed)
    cent = rng.integers(0, 219, (K, dim))
    members = np.clip(cent[c] + rng.integers(-3, 4, (n_c, dim)), 0, 218)
    return cent.astype(np.float64), members.astype(np.float64)


def distances(O, metric, cent, members, P, L):
    """n_c lists of K canonical integers: distance(centroid_j, member_i) as values alone (none is negative: integers compare as they do)"""
    c = O.Ctx(store=False, keygen=False)
    return [TM.to_ints(np.stack([c.distance(metric, cj, mi, P=P, L=L) for cj in cent])) for mi in members]


def audit_model(O, metric, cent, members, roots, c, P, L, plan_k=None):
    """the circuit on quantized cent (K, dim, 4), members (n_c, dim, 4), roots (K + 1, 4) = [centroids' root | cluster roots] and the header's
    c -> dict(advice, lookup, flags, selectors, generator: the cells of the distance and qmin blocks (the oracle keeps no constant bit
    there), break_points, n_in, regions, per_member, per_member_l, chain_off, pick_off, routed (n_c,) uint8, public (2, 4), ties: the
    (cell, earlier cell) pairs the circuit constrains equal beyond the gadgets' own, own, m: the cells of own_i and m_i, index_root)"""
    K, dim, n_c = cent.shape[0], cent.shape[1], members.shape[0]
    assert 0 <= c < K and roots.shape == (K + 1, 4)
    s = TM._Stream()
    r_int = TM.to_ints(roots)
    s.ints([c] + r_int, [0] * (K + 2))
    reg, cst, ind = {"indicator": s.n}, [], []
    for j in range(K):                                       # as ann_update_model.update_model
        cells, gates, z = TM.is_equal(c, j)
        if j == 0:
            cells, gates = cells[4:], gates[4:]              # the unrolled is_zero(c): [z, c, inv, 1, 0, c, z, 0]
            cst += [s.n + 3, s.n + 4, s.n + 7]
        else:
            cst += [s.n + 1, s.n + 2, s.n + 7, s.n + 8, s.n + 11]
        s.ints(cells, gates)
        ind.append(z)
    reg["select"] = s.n
    cells, gates, picked = TM.select_by_indicator(r_int[1:], ind)
    s.ints(cells, gates)
    picked_cell = s.n - 1
    reg["sponge_old"] = s.n
    ctx = O.Ctx(store=True, keygen=True)
    index_root = ctx.merkle_commitment(roots[None])
    s.ctx(ctx)
    s.lk.pop()
    reg["centroids"] = s.n
    s.adv += [cent.reshape(-1, 4), members.reshape(-1, 4)]
    s.sel.append(np.zeros((K + n_c) * dim, dtype=np.uint8))
    s.n += (K + n_c) * dim
    reg["members"], reg["routed"] = reg["centroids"] + K * dim, s.n
    generator, own_cells, m_cells, routed, ties = [], [], [], [], []
    per_member = per_member_l = chain_off = pick_off = None
    from halo2_vectordb_amd import circuit_sym as CS
    d_out = int(CS._distance_block(metric, dim, P, L).outs[0])   # where a distance block holds its output (Sym's trace of distance)
    for i in range(n_c):
        at, lk_at = s.n, sum(x.shape[0] for x in s.lk)
        ctx = O.Ctx(store=True, keygen=True)
        d = [ctx.distance(metric, cent[j], members[i], P=P, L=L) for j in range(K)]
        s.ctx(ctx)
        dist_cells = (s.n - at) // K
        d_int = TM.to_ints(np.stack(d))
        chain = s.n
        ctx = O.Ctx(store=True, keygen=True)
        m = d[0]
        for j in range(1, K):
            m = ctx.op("qmin", m, d[j], P=P, L=L)
        s.ctx(ctx)
        (m_int,) = TM.to_ints(m[None])
        generator.append((at, s.n))
        m_cells.append(s.n - 1 if K > 1 else at + d_out)     # qmin ends in its select: the output is the block's last cell
        pick = s.n
        cells, gates, own = TM.select_by_indicator(d_int, ind)
        s.ints(cells, gates)
        own_cells.append(s.n - 1)
        ties.append((s.n - 1, m_cells[-1]))
        routed.append(1 if own == m_int else 0)
        assert own == d_int[c]
        if i == 0:
            per_member, per_member_l = s.n - at, sum(x.shape[0] for x in s.lk) - lk_at
            chain_off, pick_off = chain - at, pick - at
            assert dist_cells * K == chain_off
        assert (s.n - at, sum(x.shape[0] for x in s.lk) - lk_at) == (per_member, per_member_l)
    reg["merkle_c"] = s.n
    croot, zero = AN._merkle(O, s, cent, False)
    reg["merkle_m"] = s.n
    mroot, _ = AN._merkle(O, s, members, zero)
    advice, sel = np.concatenate(s.adv), np.concatenate(s.sel) & 1
    lookup = np.concatenate([x for x in s.lk if x.shape[0]] or [np.zeros((0, 4), dtype=np.uint64)])
    assert advice.shape[0] == sel.shape[0] == s.n
    flags, vals = sel.copy(), TM.to_ints(advice)
    flags[cst] |= 2
    # a root's cell: the last cell of its tree's trace that holds the digest (the squeeze of the last permutation)
    last = lambda lo, hi, v: max(x for x in range(lo, hi) if vals[x] == v)
    croot_cell = last(reg["merkle_c"], reg["merkle_m"], TM.to_ints(croot[None])[0])
    mroot_cell = last(reg["merkle_m"], s.n, TM.to_ints(mroot[None])[0])
    ties += [(croot_cell, 1), (mroot_cell, picked_cell)]
    pad_c, pad_m = (1 << (K - 1).bit_length()) > K, (1 << (n_c - 1).bit_length()) > n_c
    assert AN._mark_constants(flags, vals, reg["sponge_old"], K + 1) == reg["centroids"]
    assert AN._mark_constants(flags, vals, reg["merkle_c"], dim, K, pad_c) == reg["merkle_m"]
    assert AN._mark_constants(flags, vals, reg["merkle_m"], dim, n_c, pad_m and not pad_c) == s.n
    gen = np.zeros(s.n, dtype=bool)
    for lo, hi in generator:
        gen[lo:hi] = True
    return dict(advice=advice, lookup=lookup, flags=flags, selectors=sel, generator=gen, break_points=TM.row_walk(sel, plan_k) if plan_k is not None else None,
                n_in=K + 2, regions=reg, per_member=per_member, per_member_l=per_member_l, chain_off=chain_off, pick_off=pick_off,
                routed=np.asarray(routed, dtype=np.uint8), public=np.stack([index_root, TM.to_limbs([c])[0]]), ties=ties, own=own_cells, m=m_cells,
                indicators=ind, picked=picked, picked_cell=picked_cell, croot_cell=croot_cell, mroot_cell=mroot_cell, index_root=index_root,
                centroids_root=croot, members_root=mroot)
