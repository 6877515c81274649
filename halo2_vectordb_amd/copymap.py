"""The Poseidon permutation's cell template and the tests' host restatements of the permutation argument's inputs.

`permutation_template` is one PoseidonChip<F, 3, 2>::permutation as `merkle_commitment` emits it
(src/gadget/vectordb.rs:165-223): for every cell, the earlier cell of the permutation, the state word or the absorbed
word it copies.  It is traced symbolically from the cell templates of the halo2-base primitives the permutation is made of —
GateChip::sum, inner_product with constants, mul, mul_add — in exactly the order halo2_vectordb_amd/csrc/witness.hip
(trace_permutation) emits them.  The tracer consumes the gate / constant flag bytes of one real permutation (a keygen-style run) both
to resolve the one structural choice that depends on the spec's constants (inner_product starts with the first operand itself when
its constant is one) and as a check: every gate-start bit and every constant bit of the template must equal the kernel's.
The block builders turn the template into a unit block and place it along the leaves and the tree (place_merkle, build_merkle,
build_merkle_update).  `lookup_sources` and `mapping_from_copy_of` restate on the host what keygen does on the device.
[UPSTREAM-RECALL] for the primitives' cell templates, as for the kernels themselves."""
import numpy as np

T, RATE, R_F, R_P = 3, 2, 8, 57
HALF = R_F // 2
SELF, CONST = -1, -2          # template codes; >= 0: offset inside the block; state input i: -10 - i; message input i: -20 - i


class _Tracer:
    """symbolic WCtx: records per cell (source code, gate bit, constant bit)"""

    def __init__(self, flags):
        self.src, self.gate, self.cst, self.flags = [], [], [], flags

    def push(self, src, gate, cst=False):
        pos = len(self.src)
        self.src.append(CONST if cst else (SELF if src is None else src))
        self.gate.append(bool(gate))
        self.cst.append(bool(cst))
        return pos

    def next_is_const(self):
        return bool(self.flags[len(self.src)] & 2)

    # GateChip::sum: v0, then (v_i, 1, s_i); `cmask` bit i: v_i is a constant
    def sum(self, v, cmask):
        self.push(v[0], len(v) > 1, bool(cmask & 1))
        out = None
        for i in range(1, len(v)):
            self.push(v[i], False, bool((cmask >> i) & 1))
            self.push(None, False, True)
            out = self.push(None, i + 1 < len(v))
        return out

    # inner_product(a, constants): starts with a_0 itself when the first constant is one, with a constant zero otherwise
    def ip_const(self, a):
        n = len(a)
        if self.next_is_const():
            self.push(None, True, True)
            i0, ng = 0, n
        else:
            self.push(a[0], n - 1 > 0)
            i0, ng = 1, n - 1
        out, gi = None, 1
        for i in range(i0, n):
            self.push(a[i], False)
            self.push(None, False, True)
            out = self.push(None, gi < ng)
            gi += 1
        return out

    def mul(self, a, b):                       # [0, a, b, out]
        self.push(None, True, True)
        self.push(a, False)
        self.push(b, False)
        return self.push(None, False)

    def sbox(self, x):                         # x^5 + c: mul(x, x), mul(x2, x2), mul_add(x, x4, c) = [c, x, x4, out]
        x2 = self.mul(x, x)
        x4 = self.mul(x2, x2)
        self.push(None, True, True)
        self.push(x, False)
        self.push(x4, False)
        return self.push(None, False)

    def dense(self, st):
        return [self.ip_const(st) for _ in range(T)]


def _trace_permutation(t, n_in):
    """one PoseidonChip::permutation absorbing n_in message words on tracer `t`; -> the final state's cells"""
    st = [-10 - i for i in range(T)]
    st[0] = t.sum([st[0], None], 0b10)
    for i in range(n_in):
        st[1 + i] = t.sum([st[1 + i], -20 - i, None], 0b100)
    for i in range(n_in + 1, T):
        st[i] = t.sum([st[i], None], 0b10)
    for _ in range(1, HALF):
        st = t.dense([t.sbox(x) for x in st])
    st = t.dense([t.sbox(x) for x in st])                       # last of the first full rounds, then the pre-sparse matrix
    for _ in range(R_P):
        s0 = t.sbox(st[0])
        cur = [s0, st[1], st[2]]
        nxt = [t.ip_const(cur)]
        for i in range(1, T):                                   # mul_add(s0, e, s_i) = [s_i, s0, e, out]
            t.push(cur[i], True)
            t.push(s0, False)
            t.push(None, False, True)
            nxt.append(t.push(None, False))
        st = nxt
    for _ in range(HALF - 1):
        st = t.dense([t.sbox(x) for x in st])
    return t.dense([t.sbox(x) for x in st])


def permutation_template(flags, n_in):
    """(src codes, final state offsets) of one PoseidonChip::permutation absorbing n_in message words; `flags`: the kernel's
    flag bytes of one such permutation (bit 0 gate start, bit 1 constant)."""
    t = _Tracer(flags)
    st = _trace_permutation(t, n_in)
    n = len(t.src)
    if n != len(flags):
        raise ValueError(f"permutation template has {n} cells, the kernel emitted {len(flags)}")
    gate = np.array(t.gate, dtype=bool)
    cst = np.array(t.cst, dtype=bool)
    f = np.asarray(flags)
    if not (np.array_equal(gate, (f & 1).astype(bool)) and np.array_equal(cst, (f & 2).astype(bool))):
        raise ValueError("permutation template disagrees with the kernel's gate / constant flags")
    return np.array(t.src, dtype=np.int64), st


def perm_cells(n_in):
    return {2: 18, 1: 15, 0: 12}[n_in] + 2238


def lookup_sources(flags, n_lookup):
    """For every cell of the lookup stream (cells_to_lookup: copies of advice cells, laid out in the lookup columns) the
    stream offset of the advice cell it copies, from a keygen-style run's flag bytes: the kernels mark those cells with bit 2
    in the order they queue them (gadgets.hpp r_range_check).  Raises when the counts differ — a circuit that looks a cell
    up that was assigned somewhere else (a range check of at most lookup_bits bits) is not covered."""
    src = np.flatnonzero(np.asarray(flags, dtype=np.uint8) & 4).astype(np.int64)
    if src.size != n_lookup:
        raise ValueError(f"{src.size} advice cells are marked as lookup sources for {n_lookup} lookup cells")
    return src


def mapping_from_copy_of(copy_of, break_points, n_cols, rows, lookup_src=None, lookup_rows=None, const_idx=None, n_consts=0, instance_cells=None):
    """Permutation over a grid of columns x rows (words col << 32 | row, the identity where nothing is tied) from a copy map
    over the stream cells that fill the first len(break_points) + 1 columns: every set of cells that copy one another
    (directly or through other copies) becomes one cycle, and the overlap cell that ends column c is the cell that starts
    column c + 1.  `lookup_src` (with `lookup_rows` cells per lookup column): lookup cell j, at row j % lookup_rows of column
    n_adv + j // lookup_rows, joins the cycle of the advice cell lookup_src[j].
    `const_idx` (with `n_consts`): cell i with const_idx[i] = r >= 0 is tied to row r of ONE MORE column, number n_cols, the
    fixed column that holds the circuit's constants — how halo2-base pins `QuantumCell::Constant` cells and
    `assert_is_const` — and the grid gets n_cols + 1 columns.
    `instance_cells` (a list, possibly empty; requires `const_idx`): the grid gets column n_cols + 1 as well, the instance
    column, whose row i joins the cycle of stream cell instance_cells[i] (RangeWithInstanceCircuitBuilder's constrain_instance)."""
    copy_of = np.asarray(copy_of, dtype=np.int64)
    n_cells = copy_of.size
    bp = np.asarray(break_points, dtype=np.int64)
    starts = np.concatenate([[0], np.cumsum(bp)])
    with_consts = const_idx is not None
    root = copy_of.copy()
    if with_consts:
        const_idx = np.asarray(const_idx, dtype=np.int64)
        tied = np.flatnonzero(const_idx >= 0)
        if (copy_of[tied] != tied).any():
            raise ValueError("a cell tied to a constant must be the root of its copies")
        root = np.concatenate([root, n_cells + np.arange(n_consts, dtype=np.int64)])      # the fixed column's cells follow the stream
        root[tied] = n_cells + const_idx[tied]
    while True:                                                 # pointer jumping: sources are earlier cells or fixed cells
        nxt = root[root]
        if np.array_equal(nxt, root):
            break
        root = nxt
    s = np.arange(n_cells, dtype=np.int64)
    col = np.searchsorted(starts, s, side="right") - 1
    row = s - starts[col]
    # the overlap cell: stream offset starts[c + 1] also sits in column c at row bp[c]
    dup_s = starts[1:][starts[1:] < n_cells]
    dup_col = np.arange(dup_s.size, dtype=np.int64)
    pos_col = [col, dup_col]
    pos_row = [row, bp[: dup_s.size]]
    pos_root = [root[:n_cells], root[dup_s]]
    if lookup_src is not None and len(lookup_src):
        j = np.arange(len(lookup_src), dtype=np.int64)
        pos_col.append(bp.size + 1 + j // lookup_rows)
        pos_row.append(j % lookup_rows)
        pos_root.append(root[np.asarray(lookup_src, dtype=np.int64)])
    total_cols = n_cols + (1 if with_consts else 0)
    if with_consts:
        if n_consts > rows:
            raise ValueError("more distinct constants than rows in the fixed column")
        pos_col.append(np.full(n_consts, n_cols, dtype=np.int64))
        pos_row.append(np.arange(n_consts, dtype=np.int64))
        pos_root.append(root[n_cells:])
    if instance_cells is not None:
        if not with_consts:
            raise ValueError("the instance column follows the constants' column")
        inst = np.asarray(instance_cells, dtype=np.int64).reshape(-1)
        if inst.size > rows:
            raise ValueError("more public cells than rows in the instance column")
        total_cols += 1
        pos_col.append(np.full(inst.size, n_cols + 1, dtype=np.int64))
        pos_row.append(np.arange(inst.size, dtype=np.int64))
        pos_root.append(root[inst])
    pos_col, pos_row, pos_root = np.concatenate(pos_col), np.concatenate(pos_row), np.concatenate(pos_root)
    if int(root.size) * total_cols * rows < (1 << 62):           # one combined key sorts several times faster than three
        order = np.argsort(pos_root * (total_cols * rows) + pos_col * rows + pos_row, kind="stable")
    else:
        order = np.lexsort((pos_row, pos_col, pos_root))
    pc, prw, pr = pos_col[order], pos_row[order], pos_root[order]
    first = np.concatenate([[True], pr[1:] != pr[:-1]])
    group_start = np.maximum.accumulate(np.where(first, np.arange(pr.size), 0))
    last = np.concatenate([pr[1:] != pr[:-1], [True]])
    nxt_idx = np.where(last, group_start, np.arange(pr.size) + 1)
    mapping = (np.arange(total_cols, dtype=np.uint64)[:, None] << np.uint64(32)) | np.arange(rows, dtype=np.uint64)[None, :]
    mapping[pc, prw] = (pc[nxt_idx].astype(np.uint64) << np.uint64(32)) | prw[nxt_idx].astype(np.uint64)
    return mapping
