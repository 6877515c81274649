"""The recentre of one cluster as a checker (pipeline.AnnRecentreHotPath; include/vdb.h vdb_wit_ann_recentre), cell for cell, in the manner
of ann_mean_model.mean_model and from the same bricks: the head [header | indicators | selection | sponge] as ann_update_model.update_model
states it, oracle contexts for every qadd and every qdiv, ann_model._merkle for the members' tree, merkle_ops_model.ops_model (a plain
batch of it is merkle_update_model's stream) for the one write into the centroids' tree, Ctx.merkle_commitment of one vector of K + 1
words for the two sponges.  Nothing here knows how the GPU lays out its work buffers.

    A  [c | centroids_root | cluster roots]         assigned
    B  ind_0 = is_zero(c); ind_j = is_equal(c, Constant(j))
    C  picked = select_by_indicator(cluster roots, ind)
    D  index_root_old = sponge([centroids_root | cluster roots])
    I  members                                      assigned
    M  len = Constant(quantization(n_c)); s_ij = qadd(member_i[j], s_i-1,j), member-major; mean_j = qdiv(s_j, len)
    MM mroot = merkle_commitment(members)           mroot <-> picked
    U  the update block of the centroids' tree, one write at slot c: old root <-> centroids_root, idx <-> c, new vector word j <-> mean_j
    G  index_root_new = sponge([U's new root | cluster roots])

The old centroid c never appears: `tree`, the centroids' tree, carries it as the old leaf of the path.
"""
import numpy as np

import ann_mean_model as MM
import ann_model as AN
import merkle_ops_model as MO
import topk_model as TM

NODE = 2 * 2238 + 18 + 12                                    # a tree node's hash: the permutation absorbing two words, then the padding-only one


def recentre_model(O, tree, members, roots, c, P, L, plan_k=None, new_vector=None):
    """the circuit on the centroids' `tree` (merkle_update_model.build_tree's lists per level; updated in place), quantized members
    (n_c, dim, 4), roots (K + 1, 4) = [centroids' root | cluster roots] and the header's c.  `new_vector` (dim, 4): what the update block
    absorbs in place of the quotients (a test of the binding) -> dict(advice, lookup, flags, selectors, generator: the cells of the qdiv
    blocks, break_points, n_in, regions, public (3, 4), new_centroid (dim, 4), ties: the (cell, earlier cell) pairs the circuit constrains
    equal beyond the gadgets' own and the sponge G's absorbed words, mean, new_vector: cells, picked_cell, mroot_cell, old_root_cell,
    new_root_cell, idx_cell, update: ops_model's dict, qdiv_cells, qdiv_lk)"""
    K, n_c, dim = roots.shape[0] - 1, members.shape[0], members.shape[1]
    assert 0 <= c < K and K >= 2 and len(tree[0]) == 1 << (K - 1).bit_length()
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
    root_old = ctx.merkle_commitment(roots[None])
    assert ctx.err == 0
    s.ctx(ctx)
    s.lk.pop()
    reg["update"] = reg["members"] = s.n
    s.adv.append(members.reshape(-1, 4))
    s.sel.append(np.zeros(n_c * dim, dtype=np.uint8))
    s.n += n_c * dim
    reg["len"] = s.n
    ln = MM.quantization(n_c, P)
    s.ints([ln], [0])
    cst.append(reg["len"])
    reg["chain"] = s.n
    ctx = O.Ctx(store=True, keygen=True)
    sums = [members[0, j] for j in range(dim)]
    for i in range(1, n_c):
        for j in range(dim):
            sums[j] = ctx.op("qadd", members[i, j], sums[j], P=P, L=L)
    s.ctx(ctx)
    assert s.n - reg["chain"] == 4 * (n_c - 1) * dim and ctx.n_lookup == 0
    cst += [reg["chain"] + 4 * t + 2 for t in range((n_c - 1) * dim)]          # qadd's [a, b, Constant(1), out]
    reg["div"] = s.n
    ctx = O.Ctx(store=True, keygen=True)
    ln_fr = TM.to_limbs([ln])[0]
    mean = np.stack([ctx.op("qdiv", sums[j], ln_fr, P=P, L=L) for j in range(dim)])
    assert ctx.err == 0
    s.ctx(ctx)
    qdiv_cells, qdiv_lk = (s.n - reg["div"]) // dim, ctx.n_lookup // dim
    assert qdiv_cells * dim == s.n - reg["div"] and qdiv_lk * dim == ctx.n_lookup
    mean_cells = [reg["div"] + (j + 1) * qdiv_cells - 1 for j in range(dim)]   # qdiv ends in cond_neg's select: the block's last cell
    reg["merkle_m"] = s.n
    mroot, has_zero = AN._merkle(O, s, members, False)
    reg["centroid_update"] = ub = s.n
    absorbed = mean if new_vector is None else np.ascontiguousarray(new_vector, dtype=np.uint64)
    u = MO.ops_model(O, tree, [c], None, absorbed[None], 0)
    s.adv.append(u["advice"]); s.sel.append(u["selectors"]); s.n += u["advice"].shape[0]
    reg["sponge_new"] = s.n
    words = np.concatenate([u["public"][-1][None], roots[1:]])
    ctx = O.Ctx(store=True, keygen=True)
    root_new = ctx.merkle_commitment(words[None])
    assert ctx.err == 0
    s.ctx(ctx)
    advice, sel = np.concatenate(s.adv), np.concatenate(s.sel) & 1
    lookup = np.concatenate([x for x in s.lk if x.shape[0]] or [np.zeros((0, 4), dtype=np.uint64)])
    assert advice.shape[0] == sel.shape[0] == s.n
    flags, vals = sel.copy(), TM.to_ints(advice)
    flags[cst] |= 2
    assert [vals[x] for x in mean_cells] == TM.to_ints(mean)
    last = lambda lo, hi, v: max(x for x in range(lo, hi) if vals[x] == v)
    (v_mroot,), (v_old,), (v_new,) = TM.to_ints(mroot[None]), TM.to_ints(u["public"][0][None]), TM.to_ints(u["public"][-1][None])
    mroot_cell = last(reg["merkle_m"], ub, v_mroot)
    top = ub + u["regions"][0]["levels"][-1]                 # the top level: [assert_bit 4 | select 8 | select 8 | H old | select 8 | select 8 | H new]
    old_root_cell = last(top + 20, top + 20 + NODE, v_old)
    new_root_cell = last(top + 36 + NODE, top + 36 + 2 * NODE, v_new)
    idx_cell = reg["sponge_new"] - 1                         # the index inner product ends the block
    assert vals[idx_cell] == c
    new_vector_cells = [ub + j for j in range(dim)]
    ties = list(zip(new_vector_cells, mean_cells)) + [(old_root_cell, 1), (idx_cell, 0), (mroot_cell, picked_cell)]
    assert AN._mark_constants(flags, vals, reg["sponge_old"], K + 1) == reg["members"]
    assert AN._mark_constants(flags, vals, reg["merkle_m"], dim, n_c, has_zero) == ub
    assert AN._mark_constants(flags, vals, reg["sponge_new"], K + 1) == s.n
    from test_merkle_ops_cpu import kernel_like_flags
    flags[ub:reg["sponge_new"]] = kernel_like_flags(u)
    gen = np.zeros(s.n, dtype=bool)
    gen[reg["div"]:reg["merkle_m"]] = True
    public = np.stack([root_old, TM.to_limbs([c])[0], root_new])
    return dict(advice=advice, lookup=lookup, flags=flags, selectors=sel, generator=gen, break_points=TM.row_walk(sel, plan_k) if plan_k is not None else None,
                n_in=K + 2, regions=reg, public=public, new_centroid=mean, ties=ties, mean=mean_cells, new_vector=new_vector_cells, picked_cell=picked_cell,
                mroot_cell=mroot_cell, old_root_cell=old_root_cell, new_root_cell=new_root_cell, idx_cell=idx_cell, update=u, qdiv_cells=qdiv_cells,
                qdiv_lk=qdiv_lk, indicators=ind, picked=picked, index_root_old=root_old, index_root_new=root_new, members_root=mroot,
                new_centroids_root=u["public"][-1])
