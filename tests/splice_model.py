"""Which PARTS of a witness can be swapped alone?  The splice sweep of tests/test_splice_cpu.py and tests/test_gpu_splice.py, over
Python integers and numpy; it imports nothing from the product and counts with tests/alteration_model.py.

The single-cell sweep of alteration_model asks of every cell whether it can be replaced alone.  A consumer that is cut from its
producer escapes it: everything downstream of the cut can be replaced TOGETHER and consistently, and no single cell is free.  So:
take two honest witnesses W, W' of one circuit whose inputs differ in one coordinate.  The set D of cells where they differ is what
that input reaches.  Link the cells of D as the constraint map links them — a copy and its source, a lookup cell and its source,
the changed cells of one gate — and D falls into pieces.  A hybrid witness (W with W' written into part of D) that satisfies every
constraint cannot take one end of a link without the other, so it is a union of pieces.  In a sound circuit the piece that holds the
altered input is the only one that can be written alone; any other piece S whose splice violates nothing is a cut — a forgery recipe
— and has to have a reason in the reference's own circuit (`explain_cut`) or it is a missing tie of the map.

Gates are linked finely.  With C the changed cells of a gate a + b c = d, every proper non-empty subset T of C is tried (T from W',
the rest from W: at most 14 per gate); x and y of C are linked unless some T that satisfies the gate separates them.  A satisfying
hybrid meets the gate in nothing, in all of C or in a satisfying T, so it still is a union of pieces: the refinement loses no cut,
and it finds the ones a coarse link of all of C hides (the inverse witness beside an operand that becomes zero).

Witnesses are object arrays of canonical integers indexed by cell.  Large ones may be sparse: `needed` names the cells the sweep
reads, every other entry may stay None (arithmetic on a None raises: nothing is read silently)."""
import numpy as np

import alteration_model as AM

R = AM.R
HAMMING_LOADED_SUM = ("the tail of a Hamming distance after ab_sum_q, which hamming_distance loads with load_witness "
                      "(reference src/gadget/distance.rs:165-169): the reference ties the qdiv / qsub tail to nothing upstream")


def changed(W, W2, LK, LK2):
    """-> (D, DL): the advice cells and the lookup cells where two witnesses differ.  Limbs ((n, 4) unsigned words) are compared
    by numpy as they are; arrays of integers element by element."""
    def diff(a, b):
        a, b = np.asarray(a), np.asarray(b)
        assert a.shape == b.shape, (a.shape, b.shape)
        if a.ndim == 2:
            return np.flatnonzero((a != b).any(axis=1))
        return np.flatnonzero(np.asarray(a != b, dtype=bool)) if len(a) else np.zeros(0, dtype=np.int64)
    return diff(W, W2), diff(LK, LK2)


def needed(cm, D, DL, public=()):
    """the cells whose integers a sweep over (D, DL) reads: D, the four cells of every gate that touches D, the sources D copies,
    the cells that copy D, the sources of the changed lookup cells, the public cells"""
    n = cm.n_cells
    D = np.asarray(D, dtype=np.int64)
    copy_of, lsrc = np.asarray(cm.copy_of), np.asarray(cm.lookup_src)
    near = (D[:, None] + np.arange(-3, 4)[None, :]).reshape(-1)
    users = np.flatnonzero(np.isin(copy_of, D))
    src = lsrc[np.asarray(DL, dtype=np.int64)] if len(DL) else np.zeros(0, dtype=np.int64)
    out = np.unique(np.concatenate([near, copy_of[D], users, src, np.asarray(list(public), dtype=np.int64)]))
    return out[(out >= 0) & (out < n)]


def sparse(n, cells, integers):
    """an object array of n cells that holds `integers` at `cells` and None elsewhere"""
    a = np.empty(n, dtype=object)
    a[np.asarray(cells, dtype=np.int64)] = list(integers)
    return a


class _Sets:
    def __init__(self, n):
        self.p = list(range(n))

    def find(self, x):
        p = self.p
        while p[x] != x:
            p[x] = p[p[x]]
            x = p[x]
        return x

    def union(self, a, b):
        a, b = self.find(a), self.find(b)
        if a != b:
            self.p[max(a, b)] = min(a, b)


def _gate_links(cm, W, W2, D, in_d, refine=True):
    """pairs of changed cells that a gate holds together: (x, y) of one gate's changed cells C, unless a proper non-empty subset T
    of C, taken from W2 with the rest from W, satisfies a + b c = d and has exactly one of x, y (refine False: every pair)"""
    n, gate = cm.n_cells, np.asarray(cm.gate)
    near = np.unique((D[:, None] - np.arange(4)[None, :]).reshape(-1))
    near = near[(near >= 0) & (near + 3 < n)]
    starts = near[gate[near]]
    pattern = sum(in_d[starts + i].astype(np.int64) << i for i in range(4)) if len(starts) else np.zeros(0, dtype=np.int64)
    a, b = [], []
    for p in range(3, 16):
        bits = [i for i in range(4) if p >> i & 1]
        s = starts[pattern == p]
        if len(bits) < 2 or not len(s):
            continue
        pairs = [(x, y) for x in bits for y in bits if x < y]
        apart = {xy: np.zeros(len(s), dtype=bool) for xy in pairs}
        for t in range(1, 16 if refine else 0):
            if t & p != t or t == p:
                continue
            v = [(W2 if t >> i & 1 else W)[s + i] for i in range(4)]
            holds = np.asarray((v[0] + v[1] * v[2] - v[3]) % R == 0, dtype=bool)
            for x, y in pairs:
                if (t >> x ^ t >> y) & 1:
                    apart[(x, y)] |= holds
        for x, y in pairs:
            keep = ~apart[(x, y)]
            a.append(s[keep] + x)
            b.append(s[keep] + y)
    none = np.zeros(0, dtype=np.int64)
    return (np.concatenate(a) if a else none), (np.concatenate(b) if b else none)


def links(cm, W, W2, D, DL, refine=True):
    """the links among the changed cells as arrays over nodes (node i < len(D): cell D[i]; node len(D) + j: lookup cell DL[j])
    -> (a, b, tie): link k joins nodes a[k] and b[k]; tie[k] is the copying cell where the link is a copy constraint, else -1.
    A changed cell whose copy source is unchanged, a changed lookup cell whose source is unchanged, or an unchanged one whose source
    changed: one of the witnesses does not satisfy the map, which is an error and not a link."""
    n = cm.n_cells
    copy_of, lsrc = np.asarray(cm.copy_of), np.asarray(cm.lookup_src)
    in_d, in_dl = np.zeros(n, dtype=bool), np.zeros(len(lsrc), dtype=bool)
    in_d[D] = True
    in_dl[DL] = True
    assert (in_d[copy_of] == in_d).all(), f"cells {np.flatnonzero(in_d[copy_of] != in_d)[:8].tolist()} changed without their copy source, or it without them"
    assert not len(lsrc) or (in_d[lsrc] == in_dl).all(), f"lookup cells {np.flatnonzero(in_d[lsrc] != in_dl)[:8].tolist()} changed without their source, or it without them"
    node = np.full(n, -1, dtype=np.int64)
    node[D] = np.arange(len(D))
    ga, gb = _gate_links(cm, W, W2, D, in_d, refine)
    copies = D[copy_of[D] != D]
    a = np.concatenate([node[copies], len(D) + np.arange(len(DL)), node[ga]])
    b = np.concatenate([node[copy_of[copies]], node[lsrc[DL]] if len(DL) else DL, node[gb]])
    tie = np.concatenate([copies, np.full(len(DL) + len(ga), -1, dtype=np.int64)])
    return a, b, tie


def pieces(cm, W, W2, LK, LK2, D=None, DL=None, refine=True):
    """the pieces of D under the map's links -> [(cells, lookup cells)], sorted arrays, ordered by their first cell.  (The links do
    not depend on which witness is written into which: a subset T of a gate's changed cells taken from W2 is its complement taken
    from W, and both are tried.)  refine False: the coarse pieces, every gate holding all its changed cells together."""
    if D is None:
        D, DL = changed(W, W2, LK, LK2)
    D, DL = np.asarray(D, dtype=np.int64), np.asarray(DL, dtype=np.int64)
    a, b, _tie = links(cm, W, W2, D, DL, refine)
    sets = _Sets(len(D) + len(DL))
    for x, y in zip(a.tolist(), b.tolist()):
        sets.union(x, y)
    root = np.fromiter((sets.find(x) for x in range(len(D) + len(DL))), dtype=np.int64, count=len(D) + len(DL))
    order = np.argsort(root, kind="stable")
    out = []
    for grp in np.split(order, np.flatnonzero(np.diff(root[order])) + 1) if len(order) else []:
        out.append((D[grp[grp < len(D)]], DL[grp[grp >= len(D)] - len(D)]))
    return sorted(out, key=lambda p: int(p[0][0]) if len(p[0]) else -1)


def bridge_ties(cm, W, W2, LK, LK2, D, DL, start):
    """the copy constraints that alone hold a part of D to the cell `start` (the altered input): [(cells and lookup cells behind the
    tie, the copying cell)], the largest part first; behind the tie lies the copying cell or its source, whichever the walk met last.
    Removing such a tie from the map must open a cut; the tests do that to a copy of the map to see that the sweep and the device
    notice.  (A walk over the links from `start`; a link is such a bridge when nothing behind it
    reaches back above it.  The links are the coarse ones, every gate holding all its changed cells together: what lies behind such
    a tie meets no constraint in part, so that written alone it violates nothing but the tie.)"""
    D, DL = np.asarray(D, dtype=np.int64), np.asarray(DL, dtype=np.int64)
    a, b, tie = links(cm, W, W2, D, DL, refine=False)
    n_nodes, m = len(D) + len(DL), len(a)
    ends = np.concatenate([a, b])
    other, link = np.concatenate([b, a]), np.concatenate([np.arange(m), np.arange(m)])
    order = np.argsort(ends, kind="stable")
    first = np.searchsorted(ends[order], np.arange(n_nodes + 1)).tolist()
    other, link, tie = other[order].tolist(), link[order].tolist(), tie.tolist()
    root = int(np.searchsorted(D, start))
    assert D[root] == start
    seen, low, size, at = [-1] * n_nodes, [0] * n_nodes, [1] * n_nodes, list(first[:-1])
    seen[root], clock, stack, found = 0, 1, [(root, -1)], []
    while stack:
        x, via = stack[-1]
        if at[x] < first[x + 1]:
            y, k = other[at[x]], link[at[x]]
            at[x] += 1
            if k == via:
                continue
            if seen[y] < 0:
                seen[y] = low[y] = clock
                clock += 1
                stack.append((y, k))
            else:
                low[x] = min(low[x], seen[y])
        else:
            stack.pop()
            if stack:
                up = stack[-1][0]
                low[up] = min(low[up], low[x])
                size[up] += size[x]
                if low[x] > seen[up] and tie[via] >= 0:
                    found.append((size[x], tie[via]))
    return sorted(found, reverse=True)


def one_piece(cm, W, W2, LK, LK2, D=None, DL=None):
    """what the sweep would be without its method: all of D as one piece (the self-checks of the tests must fail with this)"""
    if D is None:
        D, DL = changed(W, W2, LK, LK2)
    return [(np.asarray(D, dtype=np.int64), np.asarray(DL, dtype=np.int64))]


def spliced(W, W2, LK, LK2, piece):
    """W with W2 written into `piece` -> (values, lookup values), copies"""
    vals, lks = np.array(W, dtype=object), np.array(LK, dtype=object)
    vals[piece[0]] = W2[piece[0]]
    if len(piece[1]):
        lks[piece[1]] = LK2[piece[1]]
    return vals, lks


def splice_report(cm, W, W2, LK, LK2, piece, public, L):
    """the recount of W with W2 written into `piece`, the instance column being the hybrid's own public cells (a forger states what
    the witness holds); only the constraints that read the piece are counted.  W and LK are written and restored in place."""
    cells, lcells = piece
    keep, lkeep = W[cells].copy(), LK[lcells].copy() if len(lcells) else None
    try:
        W[cells] = W2[cells]
        if len(lcells):
            LK[lcells] = LK2[lcells]
        return AM.recount(cm, W, LK, L, public, [W[c] for c in public], touched=(cells, lcells))
    finally:
        W[cells] = keep
        if len(lcells):
            LK[lcells] = lkeep


def cuts(cm, W, W2, LK, LK2, inputs, public, L, D=None, DL=None, split=None):
    """both directions, W2 into W (direction 0) and W into W2 (direction 1): every piece that holds no cell of `inputs` (the free
    input cells at the head of the stream) is spliced alone; one whose splice violates nothing is a cut.  The fine pieces first,
    then the coarse ones that are not fine pieces themselves: the fine links may part two cells of a gate that only go together
    (x from one satisfying subset, y from another), and then no fine piece alone is the cut, while their union — a coarse piece — is.
    -> (the fine pieces, [dict(direction, cells, lookups)])"""
    W, W2, LK, LK2 = (AM._obj(x) for x in (W, W2, LK, LK2))
    public, inputs = [int(c) for c in public], np.asarray(list(inputs), dtype=np.int64)
    found, parts = [], (split or pieces)(cm, W, W2, LK, LK2, D, DL)
    every = list(parts)
    if split is None:
        fine = set((len(p[0]), int(p[0][0]) if len(p[0]) else -1, len(p[1])) for p in parts)
        every += [p for p in pieces(cm, W, W2, LK, LK2, D, DL, refine=False) if (len(p[0]), int(p[0][0]) if len(p[0]) else -1, len(p[1])) not in fine]
    for direction, (a, a2, l, l2) in enumerate(((W, W2, LK, LK2), (W2, W, LK2, LK))):
        for piece in every:
            if np.isin(piece[0], inputs).any():
                continue
            if AM.violations(splice_report(cm, a, a2, l, l2, piece, public, L)) == 0:
                found.append(dict(direction=direction, cells=piece[0], lookups=piece[1]))
    return parts, found


def fed_through(cm, cells):
    """the cells of a piece that nothing upstream states: they copy nothing, are tied to no constant and lie in no gate — cells a
    circuit loads with load_witness (the inputs are such cells; so are the two of a Hamming distance)"""
    cells = np.asarray(cells, dtype=np.int64)
    copy_of, const_idx = np.asarray(cm.copy_of), np.asarray(cm.const_idx)
    loose = cells[(copy_of[cells] == cells) & (const_idx[cells] < 0)]
    return [int(c) for c in loose if not AM.gates_of(cm, int(c))]


def loaded_witnesses(cm, n_in):
    """the cells after the inputs that copy nothing, are tied to no constant and lie in no gate: what a circuit loads with
    load_witness and uses only through copies.  The tests locate the two of every Hamming distance (`len`, `ab_sum_q`) with this."""
    return fed_through(cm, np.arange(n_in, cm.n_cells))


def explain_cut(cm, W, cut, hamming_loaded=()):
    """why the reference's own circuit has this cut too, or None: a cut without a reason is a missing tie of the map.  `W`: the
    witness the piece was written into (the direction's base).

    alteration_model's reasons hold for a piece of one cell (IS_ZERO_INVERSE: the inverse witness beside an operand that is zero in
    W).

    HAMMING_LOADED_SUM — hamming_distance sums its is_equal bits and then loads `len` and `ab_sum_q` with ctx.load_witness
    (reference src/gadget/distance.rs:165-169) instead of deriving them from that sum: the qdiv(ab_sum_q, len) and the closing qsub
    hang on two cells nothing upstream states.  Told by: the piece is fed through load_witness cells (`fed_through`), at least one,
    and every one of them is among `hamming_loaded`, the cells the caller located in the traced map.

    A further reason may be added only with the line of the reference that leaves the piece free, next to the rule."""
    cells, lookups = cut["cells"], cut["lookups"]
    if len(cells) == 1 and not len(lookups):
        return AM.explain(cm, W, int(cells[0]))
    feeds = fed_through(cm, cells)
    if feeds and set(feeds) <= set(int(c) for c in hamming_loaded):
        return HAMMING_LOADED_SUM
    return None


def describe(cm, cut):
    """for a failure message: the piece's first cells, its size and the cells it is fed through"""
    cells = cut["cells"]
    return (f"piece of {len(cells)} cells and {len(cut['lookups'])} lookup cells from cell {int(cells[0])} ({cells[:8].tolist()} ..), "
            f"written {'W2 into W' if cut['direction'] == 0 else 'W into W2'}, fed through {fed_through(cm, cells)[:8]}")


def summary(name, cm, D, DL, parts, found, reasons):
    """the line every sweep prints: cells, changed cells, pieces, cuts with their reasons and counts (pieces; cells)"""
    counts = {}
    for c, r in zip(found, reasons):
        k = (r or "UNEXPLAINED").split(",")[0].split(" (")[0]
        counts[k] = (counts.get(k, (0, 0))[0] + 1, counts.get(k, (0, 0))[1] + len(c["cells"]))
    what = "; ".join(f"{k}: {v[0]} ({v[1]} cells)" for k, v in sorted(counts.items())) or "none"
    return f"{name}: {cm.n_cells} cells, {len(D)} changed (+ {len(DL)} lookup cells), {len(parts)} pieces, {len(found)} cuts — {what}"
