"""The mean audit of one cluster as a checker (pipeline.AnnMeanHotPath; include/vdb.h vdb_wit_ann_mean), cell for cell, in the manner of
ann_audit_model.audit_model: the head [header | indicators | selection | sponge] as ann_update_model.update_model states it (topk_model's
integer templates, Ctx.merkle_commitment of one vector of K + 1 words), topk_model.select_by_indicator over Python integers for the
centroid's words, oracle contexts for every qadd and every qdiv, ann_model._merkle / _mark_constants for the two trees.

    A  [c | centroids_root | cluster roots]         assigned
    B  ind_0 = is_zero(c); ind_j = is_equal(c, Constant(j))
    C  picked = select_by_indicator(cluster roots, ind)
    D  index_root = sponge([centroids_root | cluster roots])
    I  [centroids | members]                        assigned
    S  own_j = select_by_indicator(centroids[:, j], ind), j = 0 .. dim - 1
    M  len = Constant(quantization(n_c)); s_ij = qadd(member_i[j], s_i-1,j), member-major; mean_j = qdiv(s_j, len)   mean_j <-> own_j
    MC croot = merkle_commitment(centroids)         croot <-> centroids_root
    MM mroot = merkle_commitment(members)           mroot <-> picked

means() is the values-only statement: the same qadd and qdiv through an oracle context that stores nothing; means_int() states it once
more over Python integers alone, the signed fixed-point quotient |sum| 2^P // (n 2^P) with the sign put back.
"""
import numpy as np

import ann_model as AN
import topk_model as TM

R = TM.R


def quantization(n, P):
    """quantization(n) of an integer count: n 2^P"""
    return n << P


def means(O, members, P, L):
    """(dim, 4): qdiv(sum_i members[i][j], quantization(n)) per word, from the oracle's qadd and qdiv"""
    n, dim = members.shape[0], members.shape[1]
    c = O.Ctx(store=False, keygen=False)
    ln = TM.to_limbs([quantization(n, P)])[0]
    out = []
    for j in range(dim):
        s = members[0, j]
        for i in range(1, n):
            s = c.op("qadd", members[i, j], s, P=P, L=L)
        out.append(c.op("qdiv", s, ln, P=P, L=L))
    assert c.err == 0
    return np.stack(out)


def means_int(members, P):
    """dim canonical integers: the same means over Python integers (a value above R / 2 is negative)"""
    n, dim = members.shape[0], members.shape[1]
    vals = np.asarray(TM.to_ints(members), dtype=object).reshape(n, dim)
    out = []
    for j in range(dim):
        s = sum(int(v) for v in vals[:, j]) % R
        neg = s > R // 2
        q = ((R - s if neg else s) << P) // quantization(n, P)
        out.append((R - q) % R if neg else q)
    return out


def index_means(O, grouped, offsets, P, L):
    """(K, dim, 4): means() of every cluster of grouped rows (n, dim, 4), cluster k the rows [offsets[k], offsets[k + 1])"""
    return np.stack([means(O, grouped[int(offsets[k]):int(offsets[k + 1])], P, L) for k in range(len(offsets) - 1)])


def mean_model(O, cent, members, roots, c, P, L, plan_k=None):
    """the circuit on quantized cent (K, dim, 4), members (n_c, dim, 4), roots (K + 1, 4) = [centroids' root | cluster roots] and the header's
    c -> dict(advice, lookup, flags, selectors, generator: the cells of the qdiv blocks (the oracle keeps no constant bit there),
    break_points, n_in, regions, mean_ok (dim,) uint8, public (2, 4), ties: the (cell, earlier cell) pairs the circuit constrains equal
    beyond the gadgets' own, own, mean: the cells of own_j and mean_j, qdiv_cells, qdiv_lk, index_root)"""
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
    reg["members"], reg["own"] = reg["centroids"] + K * dim, s.n
    cent_int = np.asarray(TM.to_ints(cent), dtype=object).reshape(K, dim)
    own_cells, own_vals = [], []
    for j in range(dim):
        cells, gates, own = TM.select_by_indicator([int(v) for v in cent_int[:, j]], ind)
        s.ints(cells, gates)
        own_cells.append(s.n - 1)
        own_vals.append(own)
        assert own == cent_int[c, j]
    reg["len"] = s.n
    ln = quantization(n_c, P)
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
    mean = [ctx.op("qdiv", sums[j], ln_fr, P=P, L=L) for j in range(dim)]
    s.ctx(ctx)
    qdiv_cells, qdiv_lk = (s.n - reg["div"]) // dim, ctx.n_lookup // dim
    assert qdiv_cells * dim == s.n - reg["div"] and qdiv_lk * dim == ctx.n_lookup
    mean_int = TM.to_ints(np.stack(mean))
    mean_cells = [reg["div"] + (j + 1) * qdiv_cells - 1 for j in range(dim)]   # qdiv ends in cond_neg's select: the block's last cell
    ties = list(zip(mean_cells, own_cells))
    mean_ok = [1 if a == b else 0 for a, b in zip(mean_int, own_vals)]
    reg["merkle_c"] = s.n
    croot, zero = AN._merkle(O, s, cent, False)
    reg["merkle_m"] = s.n
    mroot, _ = AN._merkle(O, s, members, zero)
    advice, sel = np.concatenate(s.adv), np.concatenate(s.sel) & 1
    lookup = np.concatenate([x for x in s.lk if x.shape[0]] or [np.zeros((0, 4), dtype=np.uint64)])
    assert advice.shape[0] == sel.shape[0] == s.n
    flags, vals = sel.copy(), TM.to_ints(advice)
    flags[cst] |= 2
    assert [vals[x] for x in mean_cells] == mean_int
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
    gen[reg["div"]:reg["merkle_c"]] = True
    return dict(advice=advice, lookup=lookup, flags=flags, selectors=sel, generator=gen, break_points=TM.row_walk(sel, plan_k) if plan_k is not None else None,
                n_in=K + 2, regions=reg, mean_ok=np.asarray(mean_ok, dtype=np.uint8), public=np.stack([index_root, TM.to_limbs([c])[0]]), ties=ties,
                own=own_cells, mean=mean_cells, mean_values=np.stack(mean), qdiv_cells=qdiv_cells, qdiv_lk=qdiv_lk, indicators=ind, picked=picked,
                picked_cell=picked_cell, croot_cell=croot_cell, mroot_cell=mroot_cell, index_root=index_root, centroids_root=croot, members_root=mroot)
