"""The Merkle circuit's constraint map without a GPU.  circuit_sym.build_merkle places one Poseidon permutation block along the leaves,
the padding's zero cell and the tree; here its host-built map is held against the oracle's own stream of the closure — assign the
vectors, merkle_commitment over them — and against what the closure says about its cells: every assigned word is absorbed once, by
its leaf, every node absorbs its two children's digests (the zero cell where the tree is padded), the sponge starts from 2^64, 0, 0.
The query circuits' map (the queries' blocks, then place_merkle over the same assigned vectors) is held against the oracle's stream
of that closure, and its Merkle part is the stand-alone circuit's, moved."""
import numpy as np
import pytest

import merkle_update_model as MU
import topk_model as TM
from halo2_vectordb_amd import circuit_sym as CS
from halo2_vectordb_amd import copymap as CM
from test_batch_query_cpu import same_map

P, L = 48, 11
SHAPES = [(6, 5), (5, 4), (8, 3), (1, 2), (2, 1), (3, 7)]        # odd and even word counts, padded and full trees, no tree, dim = 1
# cells of one permutation, from the templates it starts with: sum(state_0, c) is 4 cells, every sum(state_i, word, c) 7 with the word
# as its second cell, the unfed words' sum(state_i, c) 4 again
STATE_AT = {2: (0, 4, 11), 1: (0, 4, 11), 0: (0, 4, 8)}
WORD_AT = (5, 12)


def mark_constants(vals, flags, spans):
    """test_merkle_update_cpu.kernel_like_flags for the permutations at `spans` = [(first cell, words absorbed)]: the oracle keeps gate
    bits only, the kernels flag constant cells too (bit 1).  Whether an inner_product starts with a constant zero is read off the
    values (the cell holds 0 and the first gate is 0 + a_0 c_0); the tracer's gate bits must then be the oracle's."""
    for at, n_in in spans:
        size = CM.perm_cells(n_in)
        t = CM._Tracer(None)
        t.next_is_const = lambda: vals[at + len(t.src)] == 0 and vals[at + len(t.src) + 3] == vals[at + len(t.src) + 1] * vals[at + len(t.src) + 2] % CS.R
        CM._trace_permutation(t, n_in)
        assert len(t.src) == size and np.array_equal(np.asarray(t.gate, dtype=np.uint8), flags[at:at + size] & 1)
        flags[at:at + size] |= np.asarray(t.cst, dtype=np.uint8) << 1


def merkle_spans(n, dim, base):
    """where the closure's permutations lie, written out leaf by leaf and node by node: -> (spans for mark_constants, first cell of
    every leaf, the zero cell or None, per tree level the first cell of every node, the cell after the last)"""
    node = CM.perm_cells(2) + CM.perm_cells(0)
    words = [min(2, dim - 2 * p) for p in range(dim // 2 + 1)]        # a sponge of rate 2 pads in a permutation of its own when full
    spans, leaves, at = [], [], base
    for _ in range(n):
        leaves.append(at)
        for w in words:
            spans.append((at, w))
            at += CM.perm_cells(w)
    lp, _depth = MU.padded(n)
    zero = at if lp > n else None
    at += lp > n
    levels, width = [], lp
    while width > 1:
        width //= 2
        levels.append([])
        for _ in range(width):
            levels[-1].append(at)
            spans += [(at, 2), (at + CM.perm_cells(2), 0)]
            at += node
    return spans, leaves, zero, levels, at


def database(O, n, dim, seed):
    return O.quantize(np.random.default_rng(seed).integers(0, 219, size=(n, dim)).astype(np.float64), P)


def oracle_merkle(O, n, dim):
    """-> (database, the closure's values, kernel-like flags, the oracle's selectors, the root merkle_commitment returned)"""
    db = database(O, n, dim, 10 * n + dim)
    c = O.Ctx(store=True, keygen=True)
    c.assign_witnesses(db)
    root = c.merkle_commitment(db)
    assert c.err == 0 and c.n_lookup == 0
    vals, sel = TM.to_ints(c.advice()), c.selectors().astype(np.uint8) & 1
    flags = sel.copy()
    spans, _leaves, zero, _levels, _end = merkle_spans(n, dim, n * dim)
    mark_constants(vals, flags, spans)
    if zero is not None:
        flags[zero] |= 2                                     # ctx.load_zero(): a constant cell of the kernels' too
    return db, vals, flags, sel, root


@pytest.mark.parametrize("n,dim", SHAPES)
def test_host_built_map_is_the_oracles_closure(O, n, dim):
    db, vals, flags, sel, root = oracle_merkle(O, n, dim)
    cm, root_cell = CS.build_merkle(n, dim, lambda lo, hi: flags[lo:hi], lambda lo, hi: vals[lo:hi])
    _spans, leaves, zero, levels, end = merkle_spans(n, dim, n * dim)
    assert cm.n_cells == len(vals) == end and len(cm.lookup_src) == 0 and not cm.asserted.any()
    (root_int,) = TM.to_ints(root)
    assert vals[root_cell] == root_int == TM.to_ints(O.poseidon_merkle_root(db))[0]
    w = np.asarray(vals, dtype=object)
    rep = cm.check_witness(w, [], flags)
    assert not any(rep.values()), rep
    assert np.array_equal(cm.gate, sel.astype(bool))
    # every assigned word is copied exactly once: word i of vector j by the permutation of leaf j that absorbs it
    for j in range(n):
        for i in range(dim):
            users = np.flatnonzero(cm.copy_of == j * dim + i)
            users = users[users != j * dim + i]
            assert users.tolist() == [leaves[j] + i // 2 * CM.perm_cells(2) + WORD_AT[i % 2]], (j, i)
    # every node absorbs the digests of its two children: cells inside the child's own trace that hold its hash, or the zero cell
    tree = MU.build_tree(O, db)
    digests = [TM.to_ints(np.stack(lv)) for lv in tree]
    first_after_leaves = zero if zero is not None else levels[0][0] if levels else end
    spans_of = [list(zip(leaves, leaves[1:] + [first_after_leaves]))] + [[(a, a + CM.perm_cells(2) + CM.perm_cells(0)) for a in lv] for lv in levels]
    zero_users = 0
    for l, lv in enumerate(levels):
        for i, at in enumerate(lv):
            for side in range(2):
                child, cell = 2 * i + side, at + WORD_AT[side]
                src = int(cm.copy_of[cell])
                assert vals[cell] == digests[l][child]
                if l == 0 and child >= n:
                    assert src == zero and vals[src] == 0
                    zero_users += 1
                else:
                    lo, hi = spans_of[l][child]
                    assert lo <= src < hi and int(cm.copy_of[src]) == src and vals[src] == digests[l][child], (l, i, side)
    lo, hi = spans_of[-1][0]
    assert digests[-1] == [root_int] and lo <= root_cell < hi
    lp = len(tree[0])
    if zero is not None:
        assert zero_users == lp - n == int((cm.copy_of == zero).sum()) - 1 and cm.consts[cm.const_idx[zero]] == 0
    else:
        assert zero_users == 0 and lp == n
    # the sponge's initial state at the head of every leaf and every node, which the kernels do not flag, and the flagged constants
    held = {int(cm.consts[i]) for i in set(cm.const_idx[cm.const_idx >= 0].tolist())}
    assert {1 << 64, 0} <= held
    heads = [(a, min(2, dim)) for a in leaves] + [(a, 2) for lv in levels for a in lv]
    for at, n_in in heads:
        assert [int(cm.consts[cm.const_idx[at + o]]) for o in STATE_AT[n_in]] == [1 << 64, 0, 0], at
    unflagged = (cm.const_idx >= 0) & ((flags & 2) == 0)
    assert int(unflagged.sum()) == 3 * len(heads)
    # an altered child digest and an altered assigned word are noticed
    for cell in ([int(cm.copy_of[levels[0][0] + WORD_AT[0]])] if levels else []) + [0, n * dim - 1]:
        alt = w.copy()
        alt[cell] = (alt[cell] + 1) % CS.R
        assert cm.check_witness(alt, [])["copies_unequal"] >= 1, cell
    # no assigned word may look like a gate or a constant, and the flags must be this circuit's
    bad = flags.copy()
    bad[0] |= 1
    with pytest.raises(ValueError):
        CS.build_merkle(n, dim, lambda lo, hi: bad[lo:hi], lambda lo, hi: vals[lo:hi])
    with pytest.raises(ValueError):
        CS.build_merkle(n, dim + 1, lambda lo, hi: flags[lo:hi], lambda lo, hi: vals[lo:hi])


def test_query_map_on_the_host_builder_accepts_the_oracles_closure(O):
    """build_nearest_topk(finish=False), then place_merkle, on the numpy builder: what TopKQueryHotPath.constraint_map(on_device=False)
    assembles for a query circuit that commits to its database"""
    metric, q, n, dim, topk = "euclidean", 2, 3, 2, 2
    rng = np.random.default_rng(41)
    queries, db = O.quantize(rng.random((q, dim)) + 0.1, P), O.quantize(rng.random((n, dim)) + 0.1, P)
    m = TM.topk_model(O, metric, queries, db, topk, P, L, merkle=True)
    vals, sel = TM.to_ints(m["advice"]), m["selectors"].astype(np.uint8) & 1
    base = m["regions"]["merkle"]
    spans, _leaves, _zero, _levels, end = merkle_spans(n, dim, base)
    assert end == len(vals)
    flags = sel.copy()
    mark_constants(vals, flags, spans)
    B, (ind, res), used = CS.build_nearest_topk(metric, q, n, dim, topk, P, L, extra_cells=end - base, finish=False)
    assert used == base and isinstance(B, CS._Builder)
    root_cell, stop = CS.place_merkle(B, n, dim, used, q * dim, lambda lo, hi: flags[lo:hi], lambda lo, hi: vals[lo:hi])
    cm = B.finish()
    assert stop == end == cm.n_cells and vals[root_cell] == TM.to_ints(m["root"])[0] == TM.to_ints(O.poseidon_merkle_root(db))[0]
    rep = cm.check_witness(np.asarray(vals, dtype=object), TM.to_ints(m["lookup"]), flags)
    assert not any(rep.values()), rep
    assert [vals[c] for c in res.reshape(-1)] == TM.to_ints(m["results"])
    # the distances and the leaves read the same assigned cells
    for cell in range(q * dim, (q + n) * dim):
        users = np.flatnonzero(cm.copy_of == cell)
        assert int((users >= base).sum()) == 1 and int((users < base).sum()) >= 1 + q
    # the Merkle part is the stand-alone circuit's map, moved by `base` with its words moved to where the query circuit assigns them
    mflags = np.concatenate([np.zeros(n * dim, dtype=np.uint8), flags[base:]])
    mvals = vals[q * dim:(q + n) * dim] + vals[base:]
    alone, alone_root = CS.build_merkle(n, dim, lambda lo, hi: mflags[lo:hi], lambda lo, hi: mvals[lo:hi])
    assert alone_root - n * dim == root_cell - base
    moved = np.where(alone.copy_of < n * dim, alone.copy_of + q * dim, alone.copy_of - n * dim + base)[n * dim:]
    part = CS.CopyMap(moved, alone.const_idx[n * dim:], alone.consts, alone.asserted[n * dim:], alone.gate[n * dim:], alone.lookup_src)
    none = np.zeros(0, dtype=np.int64)
    same_map(part, CS.CopyMap(cm.copy_of[base:], cm.const_idx[base:], cm.consts, cm.asserted[base:], cm.gate[base:], none))
