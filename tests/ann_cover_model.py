"""The cover of the database by the index as a checker (pipeline.AnnCoverHotPath; include/vdb.h vdb_wit_ann_cover), cell for cell, built
the way merkle_update_model builds its stream: every node hash and the sponge G are Ctx.merkle_commitment of ONE vector of two words, the
sponge D is Ctx.merkle_commitment of one vector of K + 1 words, and the two gate templates between them come from Python integers:

    sub(a, b)   [a - b, b, 1, a]      gate at cell 0, Constant(1) at cell 2
    mul(a, b)   [0, a, b, a b]        gate at cell 0, Constant(0) at cell 0

    A   [centroids_root | cluster_root_0 .. K-1]                    assigned
    I   a_0 .. a_{n-1} (slot order), b_0 .. b_{n-1} (grouped order)  assigned
    Z   load_zero, once, where any of the K + 1 trees is padded
    TD  the database tree's nodes over a, level-major -> droot
    TC  the K cluster trees' nodes over their stretch of b -> root_c     root_c <-> header's cluster_root_c
    D   index_root = sponge(header)
    G   gamma = sponge([droot, index_root])
    SA  t_i = sub(gamma, a_i);  MA  acc_i = mul(acc_{i-1}, t_i), acc_0 = t_0
    SB, MB  the same over b                                             last acc of MB <-> last acc of MA

Nothing here knows how the GPU lays out its work buffers.  The trees are hashed over the digests that are given: a cluster leaf that
is not a database leaf gives a witness whose products differ."""
import numpy as np

import ann_model as AN
import merkle_update_model as MU
import topk_model as TM

R = TM.R
NODE = 2 * 2238 + 18 + 12                                    # the permutation absorbing two words, then the padding-only one


def sub(a, b):
    return [(a - b) % R, b, 1, a], [1, 0, 0, 0], (a - b) % R


def mul(a, b):
    return [0, a, b, a * b % R], [1, 0, 0, 0], a * b % R


def _root(O, digests, lp):
    """the root of the tree over `digests` (k, 4) padded with zero to lp leaves, values only"""
    level = [digests[i] if i < digests.shape[0] else MU.ZERO for i in range(lp)]
    while len(level) > 1:
        level = list(O.poseidon_hash_many(np.stack([np.stack([level[2 * i], level[2 * i + 1]]) for i in range(len(level) // 2)])))
    return np.ascontiguousarray(level[0], dtype=np.uint64)


def _tree(O, s, digests, lp):
    """the nodes of the tree over `digests` (k, 4) padded with zero to lp leaves, appended level-major -> (root, cell of the root or None
    where the tree has no node)"""
    level = [digests[i] if i < digests.shape[0] else MU.ZERO for i in range(lp)]
    at = None
    while len(level) > 1:
        nxt = []
        for i in range(len(level) // 2):
            c, h = MU._hash_ctx(O, [level[2 * i], level[2 * i + 1]])
            at = s.n
            s.ctx(c)
            assert s.n - at == NODE
            nxt.append(h)
        level = nxt
    return level[0], at


def cover_model(O, a, b, sizes, croot, header_roots=None, plan_k=None):
    """the circuit on the database's leaf digests `a` (n, 4) in slot order, the clusters' `b` (n, 4) in grouped order, the K cluster
    `sizes` and the centroids' root (4,).  `header_roots` (K, 4): what the header states in place of the K roots of the trees over b (a
    test of the binding).  -> dict(advice, lookup (none), flags, selectors, break_points, n_in, regions, public (2, 4): [database_root |
    index_root], ties: the (cell, earlier cell) pairs the circuit constrains equal beyond the gadgets' own inputs: root_c <-> the
    header's word 1 + c, the last accumulator of b <-> that of a; root_cells, droot_cell, iroot_cell, gamma_cell, last_a, last_b, gamma)"""
    sizes = [int(x) for x in sizes]
    K, n = len(sizes), a.shape[0]
    assert sum(sizes) == n == b.shape[0] and min(sizes) >= 1
    lp, lps = MU.padded(n)[0], [MU.padded(x)[0] for x in sizes]
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(int)
    s = TM._Stream()
    cst = []
    # the trees' values first: the header states the roots before any node is traced
    roots_b = [_root(O, b[offs[c]:offs[c + 1]], lps[c]) for c in range(K)]
    hdr_roots = np.stack(roots_b) if header_roots is None else np.ascontiguousarray(header_roots, dtype=np.uint64)
    words = np.concatenate([np.ascontiguousarray(croot, dtype=np.uint64).reshape(1, 4), hdr_roots])
    reg = dict(header=0, a=K + 1, b=K + 1 + n)
    s.adv += [words, np.ascontiguousarray(a, dtype=np.uint64), np.ascontiguousarray(b, dtype=np.uint64)]
    s.sel.append(np.zeros(K + 1 + 2 * n, dtype=np.uint8))
    s.n = K + 1 + 2 * n
    padded = lp > n or any(l > x for l, x in zip(lps, sizes))
    reg["zero"] = s.n if padded else None
    if padded:
        s.ints([0], [0])
        cst.append(reg["zero"])
    reg["tree_d"] = s.n
    droot, droot_at = _tree(O, s, a, lp)
    reg["tree_c"], reg["tree_c_at"] = s.n, []
    root_at = []
    for c in range(K):
        reg["tree_c_at"].append(s.n)
        r, at = _tree(O, s, b[offs[c]:offs[c + 1]], lps[c])
        assert np.array_equal(r, roots_b[c])
        root_at.append(at)
    n_nodes = (s.n - reg["tree_d"]) // NODE
    reg["sponge"] = s.n
    ctx = O.Ctx(store=True, keygen=True)
    iroot = ctx.merkle_commitment(words[None])
    s.ctx(ctx)
    reg["gamma"] = s.n
    ctx, gamma = MU._hash_ctx(O, [droot, iroot])
    s.ctx(ctx)
    assert s.n - reg["gamma"] == NODE
    (g,) = TM.to_ints(gamma[None])
    last = []
    for key, x in (("a", TM.to_ints(a)), ("b", TM.to_ints(b))):
        reg["sub_" + key] = s.n
        t = []
        for i in range(n):
            cells, gates, out = sub(g, x[i])
            cst.append(s.n + 2)
            s.ints(cells, gates)
            t.append(out)
        reg["mul_" + key] = s.n
        acc = t[0]
        for i in range(1, n):
            cells, gates, acc = mul(acc, t[i])
            cst.append(s.n)
            s.ints(cells, gates)
        last.append(s.n - 1 if n > 1 else reg["sub_" + key])
    advice, sel = np.concatenate(s.adv), np.concatenate(s.sel) & 1
    assert advice.shape[0] == sel.shape[0] == s.n
    flags = sel.copy()
    flags[cst] |= 2
    ints = lambda lo, hi: TM.to_ints(advice[lo:hi])          # (the whole stream as Python integers would cost seconds at n = 300)

    def mark(lo, hi, words):
        """the constant bit of the permutations of one sponge over `words` words in cells [lo, hi)"""
        fl = flags[lo:hi].copy()
        assert AN._mark_constants(fl, ints(lo, hi), 0, words) == hi - lo
        return fl

    # one node's pattern serves every node (the template does not depend on the data)
    if n_nodes:
        first = mark(reg["tree_d"], reg["tree_d"] + NODE, 2)
        tree = flags[reg["tree_d"]:reg["sponge"]].reshape(n_nodes, NODE)
        assert (tree == (first & 1)[None, :]).all()
        tree |= first[None, :] & 2
    flags[reg["sponge"]:reg["gamma"]] = mark(reg["sponge"], reg["gamma"], K + 1)
    flags[reg["gamma"]:reg["sub_a"]] = mark(reg["gamma"], reg["sub_a"], 2)

    def lastv(lo, hi, v):
        return lo + max(x for x, y in enumerate(ints(lo, hi)) if y == v)

    root_cells = []
    for c in range(K):
        (v,) = TM.to_ints(roots_b[c][None])
        root_cells.append(reg["b"] + int(offs[c]) if root_at[c] is None else lastv(root_at[c], root_at[c] + NODE, v))
    (vd,), (vi,) = TM.to_ints(droot[None]), TM.to_ints(iroot[None])
    droot_cell = reg["a"] if droot_at is None else lastv(droot_at, droot_at + NODE, vd)
    iroot_cell = lastv(reg["sponge"], reg["gamma"], vi)
    gamma_cell = lastv(reg["gamma"], reg["sub_a"], g)
    ties = [(root_cells[c], 1 + c) for c in range(K)] + [(last[1], last[0])]
    reg["total"] = s.n
    return dict(advice=advice, lookup=np.zeros((0, 4), dtype=np.uint64), flags=flags, selectors=sel,
                break_points=TM.row_walk(sel, plan_k) if plan_k is not None else None, n_in=K + 1 + 2 * n, regions=reg,
                public=np.stack([droot, iroot]), ties=ties, root_cells=root_cells, droot_cell=droot_cell, iroot_cell=iroot_cell,
                gamma_cell=gamma_cell, last_a=last[0], last_b=last[1], gamma=gamma, roots=np.stack(roots_b))
