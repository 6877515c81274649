"""Which cells of a circuit does its constraint map bind?  A plain model over Python integers and numpy object arrays, for the
single-cell alteration sweeps of tests/test_alteration_cpu.py and tests/test_gpu_alteration.py.

The constraint map (copy_of, const_idx, lookup_src, the gate starts) is the input of keygen and of the device MockProver, and both
provers of the byte-equal comparison read the same one: a tie that is missing from it gives a circuit that proves, verifies and
matches the second prover while a prover may put any value into the untied cell.  This module takes the map as it is handed in —
it imports nothing from the product — and answers, for a witness that satisfies it, which cells can be replaced ALONE by any
other value without a single constraint noticing (`unnoticed`), whether such a cell is free in the reference's circuit too
(`explain`), and what the device MockProver has to report for any witness (`recount`, the recount of tests/test_gpu_sweep.py).

The one gate is halo2-base's a + b c = d over four consecutive cells from a gate start; values are canonical integers mod r."""
import numpy as np

R = 0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001
NONE = (1 << 64) - 1                       # vdb_mock_report's "no offender"
IS_ZERO_INVERSE = "is_zero inverse of a zero operand"
KINDS = (("gate_rows_violated", "first_gate_row"), ("lookup_cells_out_of_table", "first_lookup_cell"), ("copies_unequal", "first_copy"),
         ("lookup_copies_unequal", "first_lookup_copy"), ("constants_changed", "first_constant"), ("instances_unequal", "first_instance"))


def _obj(values):
    if isinstance(values, np.ndarray) and values.dtype == object:
        return values
    a = np.empty(len(values), dtype=object)
    a[:] = list(values)
    return a


def _nonzero(values, cells):
    return np.fromiter((int(values[c]) % R != 0 for c in cells), dtype=bool, count=len(cells))


def gates_of(cm, cell):
    """[(gate start, offset of `cell` inside that gate)]: a cell lies in up to four overlapping gates"""
    gate, n = np.asarray(cm.gate), cm.n_cells
    return [(s, cell - s) for s in range(max(cell - 3, 0), cell + 1) if gate[s] and s + 3 < n]


def recount(cm, values, lookup_values, L, public_cells=(), instances=(), touched=None):
    """What vdb_mock_check_dev (with vdb_mock_check_instances_dev) reports for this witness: the six violation counts and the first
    offender of each kind (NONE where the count is zero), under vdb_mock_report's field names.  Every index the map holds is tested
    before it is used, as the kernels do: a gate start on one of the last three cells, a copy source or a lookup source outside the
    stream and a constant index outside the table are violations of their kind.  L None: no range table.
    `touched` = (cells, lookup cells): the witness differs in these places only from one that satisfies every constraint, so only
    the constraints that read them are recounted — the same numbers for such a witness, in time that does not grow with the
    circuit's Python integers."""
    values, lks = _obj(values), _obj(lookup_values)
    n, nl = len(values), len(lks)
    gate, copy_of, const_idx, lsrc = np.asarray(cm.gate), np.asarray(cm.copy_of), np.asarray(cm.const_idx), np.asarray(cm.lookup_src)
    consts, pub = [int(v) % R for v in cm.consts], np.asarray(list(public_cells), dtype=np.int64)
    assert len(gate) == len(copy_of) == len(const_idx) == n and len(lsrc) == nl and len(pub) == len(instances)
    if touched is None:
        starts, copies, tied = np.flatnonzero(gate), np.flatnonzero(copy_of != np.arange(n)), np.flatnonzero(const_idx >= 0)
        lcells, insts = np.arange(nl), np.arange(len(pub))
    else:
        cells, lcells = (np.asarray(sorted(set(int(x) for x in t)), dtype=np.int64) for t in touched)
        near = np.unique((cells[:, None] - np.arange(4)[None, :]).reshape(-1))
        near = near[(near >= 0) & (near < n)]
        starts = near[gate[near]]
        users = np.flatnonzero(np.isin(copy_of, cells) & (copy_of != np.arange(n)))
        copies = np.union1d(users, cells[copy_of[cells] != cells])
        tied = cells[const_idx[cells] >= 0]
        lcells = np.union1d(lcells, np.flatnonzero(np.isin(lsrc, cells)))
        insts = np.flatnonzero(np.isin(pub, cells))
    starts, copies, tied, lcells, insts = (np.asarray(x, dtype=np.int64) for x in (starts, copies, tied, lcells, insts))
    table = _obj(consts + [None])

    def differ(a, b):
        return np.asarray(a != b, dtype=bool) if len(a) else np.zeros(0, dtype=bool)

    bad = {}
    inside = starts + 3 < n
    s = starts[inside]
    rows = np.asarray((values[s] + values[s + 1] * values[s + 2] - values[s + 3]) % R != 0, dtype=bool) if len(s) else np.zeros(0, dtype=bool)
    bad["gate_rows_violated"] = np.concatenate([starts[~inside], s[rows]])
    src = copy_of[copies]
    copies, src = copies[src >= 0], src[src >= 0]
    inside = src < n
    bad["copies_unequal"] = np.concatenate([copies[~inside], copies[inside][differ(values[copies[inside]], values[src[inside]])]])
    r = const_idx[tied]
    inside = r < len(consts)
    bad["constants_changed"] = np.concatenate([tied[~inside], tied[inside][differ(values[tied[inside]], table[r[inside]])]])
    src = lsrc[lcells]
    inside = (src >= 0) & (src < n)
    bad["lookup_copies_unequal"] = np.concatenate([lcells[~inside], lcells[inside][differ(lks[lcells[inside]], values[src[inside]])]])
    bad["lookup_cells_out_of_table"] = lcells[np.asarray(lks[lcells] >= (1 << L), dtype=bool)] if L is not None and len(lcells) else []
    c = pub[insts]
    inside = (c >= 0) & (c < n)
    claimed = _obj([int(v) % R for v in instances])[insts]
    bad["instances_unequal"] = np.concatenate([insts[~inside], insts[inside][differ(values[c[inside]], claimed[inside])]])
    out = {}
    for name, first in KINDS:
        out[name], out[first] = len(bad[name]), int(min(bad[name])) if len(bad[name]) else NONE
    return out


def violations(rep):
    return sum(rep[name] for name, _ in KINDS)


def unnoticed(cm, values, lookup_values, public_cells=()):
    """the sorted cells whose alteration, alone and to any other value, violates nothing.  A cell is noticed when it copies a cell or
    is copied by one, is tied to a constant, is the source of a lookup cell, is public, sits at offset 0 or 3 of a gate (the gate's
    sum changes with it) or at offset 1 (2) of a gate whose offset-2 (offset-1) cell is not zero (the product changes with it: r is
    prime).  The witness itself must satisfy the map, by this module's own recount."""
    values = _obj(values)
    honest = recount(cm, values, lookup_values, None, public_cells, [values[c] for c in public_cells])
    assert violations(honest) == 0, honest
    n = cm.n_cells
    gate, copy_of, const_idx, lsrc = np.asarray(cm.gate), np.asarray(cm.copy_of), np.asarray(cm.const_idx), np.asarray(cm.lookup_src)
    copies = np.flatnonzero(copy_of != np.arange(n))
    noticed = np.zeros(n, dtype=bool)
    noticed[copies] = True
    noticed[copy_of[copies]] = True
    noticed |= const_idx >= 0
    noticed[lsrc] = True
    noticed[np.asarray(list(public_cells), dtype=np.int64)] = True
    starts = np.flatnonzero(gate)
    noticed[starts] = True
    noticed[starts + 3] = True
    noticed[starts + 1] |= _nonzero(values, starts + 2)          # (the starts are distinct: no index twice in one statement)
    noticed[starts + 2] |= _nonzero(values, starts + 1)
    return np.flatnonzero(~noticed).tolist()


def unnoticed_lookups(cm, lookup_values):
    """the lookup cells that could be altered alone: those no advice cell is the source of (every other one is a copy)"""
    lsrc = np.asarray(cm.lookup_src)
    assert len(lsrc) == len(lookup_values)
    return np.flatnonzero((lsrc < 0) | (lsrc >= cm.n_cells)).tolist()


def explain(cm, values, cell):
    """why the reference's own circuit leaves `cell` free, or None: a cell without a reason is a missing tie of the map.

    IS_ZERO_INVERSE — GateChip::is_zero(a) assigns [z, a, inv, 1] with z = (a == 0) and inv = a^-1, or any value when a = 0, then
    [0, a, z, 0]: for a = 0 the first gate reads z + 0 inv = 1 and holds for every inv, and nothing else reads inv.  Told by: the
    cell lies in exactly one gate, at offset 2; that gate's offset-1 value is 0; its offset-3 cell is tied to the constant 1; its
    offset-0 cell is a witness that copies nothing (z; an assert_is_const on it, as check_power_of_two places, leaves it a witness:
    the map marks such a tie `asserted`).

    A further reason may be added only with the line of the reference that leaves the cell free, next to the rule."""
    g = gates_of(cm, cell)
    if len(g) == 1 and g[0][1] == 2:
        s = g[0][0]
        k = int(cm.const_idx[s + 3])
        z_is_witness = int(cm.copy_of[s]) == s and (int(cm.const_idx[s]) < 0 or bool(np.asarray(cm.asserted)[s]))
        if int(values[s + 1]) % R == 0 and k >= 0 and int(cm.consts[k]) % R == 1 and z_is_witness:
            return IS_ZERO_INVERSE
    return None


def summary(name, cm, free, reasons):
    """the line every sweep prints: cells, unnoticed cells with their share, reasons with counts"""
    counts = {}
    for r in reasons:
        counts[r] = counts.get(r, 0) + 1
    what = ", ".join(f"{k}: {v}" for k, v in sorted(counts.items(), key=str)) or "none"
    return f"{name}: {cm.n_cells} cells, {len(free)} unnoticed ({100.0 * len(free) / max(cm.n_cells, 1):.2f} %) — {what}"
