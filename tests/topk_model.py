"""The top-k query circuit as a checker (pipeline.TopKQueryHotPath; include/vdb.h vdb_wit_nearest_topk), cell for cell.

The oracle has the bricks the reference has — `distance`, `op("qmin")`, `nearest_vector`, `merkle_commitment`, `assign_witnesses` — but
not the bare GateChip calls the closure adds between them.  The model therefore assembles the closure's advice stream, lookup stream,
gate-start bits and break points from oracle contexts for those bricks, and from three templates over Python integers for the rest:

    is_equal(a, b)                  [a - b, b, 1, a] then [z, x, inv, 1, 0, x, z, 0] with x = a - b      gates at cells 0, 4 and 8
    select(a, b, sel)               [a - b, 1, b, a, b, sel, a - b, out]                                 gates at cells 0 and 4
    select_by_indicator(a, ind)     [0, a_0, ind_0, s_0, a_1, ind_1, s_1, ...]                           gates at cell 0 and at every s_i but the last

plus the row walk of halo2-base's GateThreadBuilder::assign_all for the break points.  tests/test_topk_cpu.py holds each of the four
against the oracle's own cells before anything is compared with the model.

Per query, in query order: the n distances, then for round r = 0 .. t - 1 over the entries `cur` (the distances for r = 0): the qmin
chain, n is_equal(min, cur_i), dim select_by_indicator, and — unless r is the last round — n select(Constant(M), cur_i, ind_i) that
give the next round's entries, M = 2^(2P) - 1.
"""
import numpy as np

R = 0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001
MONT_R = (1 << 256) % R
MONT_RINV = pow(MONT_R, -1, R)


def mask_value(P):
    """the largest value inside the chip's stated range"""
    return (1 << (2 * P)) - 1


# ---------------------------------------------------------------------------------------------------------------- integers <-> limbs
def to_limbs(vals):
    """canonical Python integers -> Montgomery limbs (m, 4) uint64"""
    if len(vals) == 0:
        return np.zeros((0, 4), dtype=np.uint64)
    raw = b"".join(((int(v) % R) * MONT_R % R).to_bytes(32, "little") for v in vals)
    return np.frombuffer(raw, dtype="<u8").reshape(-1, 4).astype(np.uint64)


def to_ints(limbs):
    """Montgomery limbs (.., 4) -> list of canonical Python integers"""
    raw = np.ascontiguousarray(limbs, dtype="<u8").reshape(-1, 4).tobytes()
    return [int.from_bytes(raw[i:i + 32], "little") * MONT_RINV % R for i in range(0, len(raw), 32)]


# ---------------------------------------------------------------------------------------------------------------- the three templates
def is_equal(a, b):
    """gate.is_equal(a, b) -> (cells, gate bits, output): sub, then is_zero of the difference"""
    x = (a - b) % R
    z = 1 if x == 0 else 0
    inv = 1 if x == 0 else pow(x, -1, R)
    return [x, b, 1, a, z, x, inv, 1, 0, x, z, 0], [1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], z


def select(a, b, sel):
    """gate.select(a, b, sel) = sel ? a : b -> (cells, gate bits, output)"""
    d = (a - b) % R
    out = (sel * d + b) % R
    return [d, 1, b, a, b, sel, d, out], [1, 0, 0, 0, 1, 0, 0, 0], out


def select_by_indicator(a, ind):
    """gate.select_by_indicator(a, ind) -> (cells, gate bits, output): the running value takes a_i wherever ind_i is set"""
    n = len(a)
    cells, gates, s = [0], [1 if n else 0], 0
    for i in range(n):
        if ind[i] != 0:
            s = a[i]
        cells += [a[i], ind[i], s]
        gates += [0, 0, 1 if i + 1 < n else 0]
    return cells, gates, s


def row_walk(gate_bits, k, minimum_rows=9):
    """GateThreadBuilder::assign_all's rows: a column is left at a gate start that has no four rows below it any more (the cell is
    repeated at the top of the next column), at the latest on the last usable row; -> the break points"""
    max_rows = (1 << k) - minimum_rows
    bp, row = [], 0
    for q in np.asarray(gate_bits, dtype=np.uint8).tolist():
        if (q and row + 4 > max_rows) or row >= max_rows - 1:
            bp.append(row)
            row = 0
        row += 1
    return np.asarray(bp, dtype=np.uint64)


# ---------------------------------------------------------------------------------------------------------------- the closure
class _Stream:
    def __init__(self):
        self.adv, self.sel, self.lk, self.n = [], [], [], 0

    def ctx(self, c):
        """everything an oracle context emitted"""
        assert c.err == 0, "the reference would have panicked on these inputs"
        a = c.advice()
        self.adv.append(a)
        self.sel.append(c.selectors().astype(np.uint8) & 1)
        self.lk.append(c.lookup())
        self.n += a.shape[0]

    def ints(self, cells, gates):
        self.adv.append(to_limbs(cells))
        self.sel.append(np.asarray(gates, dtype=np.uint8))
        self.n += len(cells)


def topk_model(O, metric, queries, db, topk, P, L, plan_k=None, inputs=True, merkle=False):
    """The closure on quantized `queries` (q, dim, 4) and `db` (n, dim, 4).  `inputs`: the stream starts with the assigned queries and
    database (the whole circuit) instead of at the first query's block (the entry points' stream); `merkle`: merkle_commitment(db)
    follows; `plan_k`: also walk the rows for the break points.  -> dict(advice, lookup, selectors, break_points, indicators
    (q, topk, n, 4), results (q, topk, dim, 4), root, regions) with regions[(query, round)] = dict(qmin, is_equal, select, mask) giving
    the first cell of each stage (mask: None in the last round) and regions["block"] = first cell of every query's block."""
    q, n, dim = queries.shape[0], db.shape[0], db.shape[1]
    assert 1 <= topk <= n and queries.shape[1] == dim
    M = mask_value(P)
    s = _Stream()
    if inputs:
        s.adv += [np.ascontiguousarray(queries).reshape(-1, 4), np.ascontiguousarray(db).reshape(-1, 4)]
        s.sel.append(np.zeros((q + n) * dim, dtype=np.uint8))
        s.n += (q + n) * dim
    db_int = [to_ints(db[i]) for i in range(n)]
    regions = {"block": []}
    inds, ress = [], []
    for qi in range(q):
        regions["block"].append(s.n)
        c = O.Ctx(store=True, keygen=True)
        cur = [c.distance(metric, db[i], queries[qi], P=P, L=L) for i in range(n)]
        s.ctx(c)
        cur_int = to_ints(np.stack(cur))
        q_ind, q_res = [], []
        for r in range(topk):
            reg = {"qmin": s.n}
            c = O.Ctx(store=True, keygen=True)
            m = cur[0]
            for i in range(1, n):
                m = c.op("qmin", m, cur[i], P=P, L=L)
            s.ctx(c)
            (m_int,) = to_ints(m)
            reg["is_equal"] = s.n
            ind = []
            for i in range(n):
                cells, gates, z = is_equal(m_int, cur_int[i])
                s.ints(cells, gates)
                ind.append(z)
            reg["select"] = s.n
            res = []
            for j in range(dim):
                cells, gates, out = select_by_indicator([db_int[i][j] for i in range(n)], ind)
                s.ints(cells, gates)
                res.append(out)
            q_ind.append(ind)
            q_res.append(res)
            reg["mask"] = None
            if r + 1 < topk:
                reg["mask"] = s.n
                nxt = []
                for i in range(n):
                    cells, gates, out = select(M, cur_int[i], ind[i])
                    s.ints(cells, gates)
                    nxt.append(out)
                cur_int = nxt
                lim = to_limbs(cur_int)
                cur = [lim[i] for i in range(n)]
            regions[(qi, r)] = reg
        inds.append(q_ind)
        ress.append(q_res)
    root = None
    regions["merkle"] = s.n
    if merkle:
        c = O.Ctx(store=True, keygen=True)
        root = c.merkle_commitment(db)
        s.ctx(c)
    advice = np.concatenate(s.adv) if s.adv else np.zeros((0, 4), dtype=np.uint64)
    selectors = np.concatenate(s.sel) if s.sel else np.zeros(0, dtype=np.uint8)
    lookup = np.concatenate([x for x in s.lk if x.shape[0]] or [np.zeros((0, 4), dtype=np.uint64)])
    assert advice.shape[0] == selectors.shape[0] == s.n
    return dict(advice=advice, lookup=lookup, selectors=selectors, break_points=row_walk(selectors, plan_k) if plan_k is not None else None,
                indicators=to_limbs([z for a in inds for b in a for z in b]).reshape(q, topk, n, 4),
                results=to_limbs([v for a in ress for b in a for v in b]).reshape(q, topk, dim, 4), root=root, regions=regions,
                indicator_bits=np.asarray(inds, dtype=np.int64))
