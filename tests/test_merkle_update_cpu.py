"""The Merkle path-update circuit without a GPU.  tests/merkle_update_model.py is the checker of the GPU streams, so nothing of it is
taken on trust: its templates are held against the oracle's own cells, its roots against the oracle's poseidon_merkle_root of the
updated database, update after update; the block-built constraint map (circuit_sym.build_merkle_update) is the cell-by-cell trace,
accepts the model's witness and notices an altered sibling and an altered chain root; and the library exports the entry points."""
import ctypes
import os

import numpy as np
import pytest

import merkle_update_model as MU
import topk_model as TM
from halo2_vectordb_amd import circuit_sym as CS
from test_batch_query_cpu import same_map

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P, L = 48, 11


def database(O, n, dim, seed):
    rng = np.random.default_rng(seed)
    return O.quantize(rng.integers(0, 219, size=(n, dim)).astype(np.float64), P)


def fetchers(m):
    vals = TM.to_ints(m["advice"])
    return (lambda lo, hi: m["flags"][lo:hi]), (lambda lo, hi: vals[lo:hi]), np.asarray(vals, dtype=object)


# ---------------------------------------------------------------------------------------------------------------- the templates
@pytest.mark.parametrize("x", [1.0, 5.5, 300.25])
def test_assert_bit_and_inner_product_templates_are_the_oracles_num_to_bits(O, x):
    """qlog2 runs check_power_of_two: num_to_bits = inner_product(bits, Constant(2^i)) over 2 P bits, then assert_bit of every bit"""
    c = O.Ctx(store=True, keygen=True)
    c.op("qlog2", O.quantize(np.asarray([x]), P)[0], P=P, L=L)
    assert c.err == 0
    adv, sel = TM.to_ints(c.advice()), list(c.selectors().astype(np.uint8) & 1)
    nb = 2 * P
    consts = [1 << i for i in range(nb)]
    starts = [i for i in range(len(adv) - 3 * nb) if adv[i + 2] == 2 and adv[i + 5] == 4 and adv[i + 8] == 8 and adv[i + 11] == 16 and adv[i] in (0, 1)]
    assert len(starts) >= 2
    for at in starts[:2]:
        bits = [adv[at]] + [adv[at + 1 + 3 * (i - 1)] for i in range(1, nb)]
        assert set(bits) <= {0, 1} and sum(bits) == 1
        cells, gates, out = MU.inner_product_const(bits, consts)
        assert cells == adv[at:at + len(cells)] and gates == sel[at:at + len(cells)]
        assert out == sum(b << i for i, b in enumerate(bits))
        at += len(cells)
        for b in bits:
            cells, gates = MU.assert_bit(b)
            assert cells == adv[at:at + 4] and gates == sel[at:at + 4]
            at += 4


def test_inner_product_template_without_a_leading_one():
    cells, gates, out = MU.inner_product_const([3, 4], [2, 5])
    assert cells == [0, 3, 2, 6, 4, 5, 26] and gates == [1, 0, 0, 1, 0, 0, 0] and out == 26
    cells, gates, out = MU.inner_product_const([1], [1])
    assert cells == [1] and gates == [0] and out == 1


@pytest.mark.parametrize("ln,cells", [(2, 4506), (3, 4509), (5, 6765), (128, 146634)])
def test_one_vector_commitment_is_one_sponge_stream(O, ln, cells):
    """Ctx.merkle_commitment of ONE vector: clear / update / squeeze, nothing else, and it returns H(v)"""
    v = database(O, 1, ln, ln)
    c = O.Ctx(store=True, keygen=True)
    out = c.merkle_commitment(v)
    assert len(c) == cells and c.n_lookup == 0
    assert np.array_equal(out, O.poseidon_hash_many(v)[0])


# ---------------------------------------------------------------------------------------------------------------- what it computes
CASES = {
    "replace": (6, 4, [2, 5, 0]),
    "insert_into_padding": (5, 3, [5, 6, 7]),
    "repeated_slot": (4, 5, [1, 1, 3, 1]),
    "sibling_pair": (8, 4, [2, 3, 6, 7, 3]),
    "two_leaves": (2, 4, [1, 0, 0]),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_roots_follow_the_oracles_commitment_of_the_updated_database(O, name):
    n, dim, indices = CASES[name]
    db = database(O, n, dim, 100 + n)
    new = database(O, len(indices), dim, 200 + n)
    levels = MU.build_tree(O, db)
    assert np.array_equal(levels[-1][0], O.poseidon_merkle_root(db))
    m = MU.update_model(O, levels, indices, new, plan_k=12)
    cur = [db[i] for i in range(n)]
    before = O.poseidon_merkle_root(db)
    for j, idx in enumerate(indices):
        if idx < len(cur):
            cur[idx] = new[j]
        else:
            assert idx == len(cur), "an insert takes the first free slot"
            cur.append(new[j])
        after = O.poseidon_merkle_root(np.stack(cur))
        assert np.array_equal(m["roots"][j][0], before) and np.array_equal(m["roots"][j][1], after), j
        assert np.array_equal(m["public"][2 + 3 * j], MU.ZERO) == (idx >= n and idx not in indices[:j]), j
        before = after
    assert np.array_equal(m["public"][0], O.poseidon_merkle_root(db)) and np.array_equal(m["public"][-1], before)
    assert np.array_equal(MU.flat_levels(levels), MU.flat_levels(MU.build_tree(O, np.stack(cur)))[: 2 * len(levels[0])])
    assert TM.to_ints(m["public"][1::3][: len(indices)]) == indices
    depth = len(levels) - 1
    assert m["advice"].shape[0] == CS.merkle_update_layout(len(indices), dim, depth)["total"]


# ---------------------------------------------------------------------------------------------------------------- the constraint map
def model(O, n, dim, indices, seed=7):
    db = database(O, n, dim, seed)
    levels = MU.build_tree(O, db)
    return MU.update_model(O, levels, indices, database(O, len(indices), dim, seed + 1)), levels


def kernel_like_flags(m, dim, depth, n_updates):
    """The flag bytes the kernels write for the model's stream: its gate bits, plus the constant bit on the constant cells of every
    permutation (the oracle keeps no constant bit).  The permutation template takes one thing from those bits — whether an
    inner_product starts with a constant zero or with its first operand — and that is read off the values here: the cell holds 0 and
    the first gate is 0 + a_0 c_0.  The tracer's gate bits must then equal the model's."""
    from halo2_vectordb_amd import copymap as CM
    lay = CS.merkle_update_layout(n_updates, dim, depth)
    flags = m["selectors"].astype(np.uint8).copy()
    vals = TM.to_ints(m["advice"])

    def mark(at, n_in):
        size = CM.perm_cells(n_in)
        t = CM._Tracer(None)
        t.next_is_const = lambda: vals[at + len(t.src)] == 0 and vals[at + len(t.src) + 3] == vals[at + len(t.src) + 1] * vals[at + len(t.src) + 2] % CS.R
        CM._trace_permutation(t, n_in)
        assert len(t.src) == size and np.array_equal(np.asarray(t.gate, dtype=np.uint8), flags[at:at + size] & 1)
        flags[at:at + size] |= np.asarray(t.cst, dtype=np.uint8) << 1

    for j in range(n_updates):
        at = lay["n_in"] + j * lay["per_update"]
        for p in range(lay["nperm"]):
            mark(at, lay["n_ins"][p])
            at += lay["sizes"][p]
        for l in range(depth):
            for off in (20, 36 + lay["node_cells"]):
                mark(at + off, 2)
                mark(at + off + CM.perm_cells(2), 0)
            at += lay["level_cells"]
    return flags


@pytest.mark.parametrize("n,dim,indices", [(6, 4, [2, 5, 2]), (3, 5, [3, 2]), (2, 3, [1])])
def test_map_is_the_trace_accepts_the_model_and_notices_tampering(O, n, dim, indices):
    m, levels = model(O, n, dim, indices)
    depth, k = len(levels) - 1, len(indices)
    m["flags"] = kernel_like_flags(m, dim, depth, k)
    ff, fv, vals = fetchers(m)
    tm, tpub = CS.trace_merkle_update(k, dim, depth, ff, fv)
    bm, bpub = CS.build_merkle_update(k, dim, depth, ff, fv)
    same_map(tm, bm)
    assert tpub == bpub and len(bpub) == 3 * k + 2
    assert bm.n_cells == m["advice"].shape[0] and len(bm.lookup_src) == 0
    rep = bm.check_witness(vals, [], flags=m["flags"])
    assert not any(rep.values()), rep
    assert [vals[c] for c in bpub] == TM.to_ints(m["public"])
    starts = np.flatnonzero(bm.gate)

    def gate_violations(w):
        return int(np.count_nonzero((w[starts] + w[starts + 1] * w[starts + 2] - w[starts + 3]) % CS.R))

    def violations(cell):
        alt = vals.copy()
        alt[cell] = (alt[cell] + 1) % CS.R
        rep = bm.check_witness(alt, [])
        return rep["copies_unequal"] + rep["constants_wrong"], gate_violations(alt)

    assert gate_violations(vals) == 0
    lay = CS.merkle_update_layout(k, dim, depth)
    # besides itself, every bit is copied into assert_bit (3), its four selects and the inner product; every sibling into both paths'
    # selects (once as `a`, twice as `b` per path); every word of a new vector into its leaf sponge
    for j in range(k):
        for l in range(depth):
            b, s = lay["bits"] + j * depth + l, lay["sibs"] + j * depth + l
            assert int((bm.copy_of == b).sum()) == 1 + 3 + 4 + 1 and int((bm.copy_of == s).sum()) == 1 + 6
            assert violations(s)[0] == 6
        for i in range(dim):
            assert int((bm.copy_of == j * dim + i).sum()) == 2
    # the chain: the top of update j's old path copies the top of update j - 1's new path
    for j in range(1, k):
        blk = m["regions"][j]["block"]
        tops = [c for c in np.flatnonzero(bm.copy_of != np.arange(bm.n_cells)) if c >= blk and lay["n_in"] <= bm.copy_of[c] < blk]
        assert len(tops) == 1 and vals[tops[0]] == TM.to_ints(m["roots"][j][0])[0] == TM.to_ints(m["roots"][j - 1][1])[0]
        assert violations(tops[0])[0] >= 1
    # power-of-two and Poseidon constants are fixed-column values
    held = {int(bm.consts[i]) for i in set(bm.const_idx[bm.const_idx >= 0].tolist())}
    assert {1 << l for l in range(depth)} <= held and (1 << 64) in held


def test_builder_refuses_empty_shapes():
    for args in ((0, 4, 2), (2, 4, 0), (2, 0, 2)):
        with pytest.raises(ValueError):
            CS.merkle_update_layout(*args)
    lay = CS.merkle_update_layout(64, 128, 14)
    assert lay["leaf_cells"] == 146634 and lay["level_cells"] == 9048 and lay["per_update"] == 146634 + 14 * 9048 + 40


def test_library_exports_the_update_entry_points():
    lib_path = os.path.join(ROOT, "halo2_vectordb_amd", "libvdb_hip.so")
    if not os.path.exists(lib_path):
        import __graft_entry__ as g
        g.build()
    lib = ctypes.CDLL(lib_path)
    names = ("vdb_merkle_tree_build_dev", "vdb_wit_merkle_update_size", "vdb_wit_merkle_update", "vdb_wit_merkle_update_dev")
    for name in names:
        assert hasattr(lib, name), name
    header = open(os.path.join(ROOT, "include", "vdb.h")).read()
    assert "VDB_MERKLE_UPDATE_MAX_UPDATES" in header and "int vdb_wit_merkle_update_dev(" in header
    from halo2_vectordb_amd import _lib, api, pipeline
    assert all(name in _lib._SIGNATURES for name in names)
    assert callable(api.merkle_tree_build) and callable(api.wit_merkle_update) and hasattr(pipeline, "UpdateHotPath")
    # the size entry needs no device: the limits of one call are refused there
    lib.vdb_wit_merkle_update_size.argtypes = [ctypes.c_size_t] * 3 + [ctypes.c_void_p] * 2
    cells, n_in = ctypes.c_uint64(), ctypes.c_uint64()
    assert lib.vdb_wit_merkle_update_size(16384, 128, 64, ctypes.byref(cells), ctypes.byref(n_in)) == 0
    assert cells.value == 64 * (128 + 1 + 28) + 64 * (146634 + 14 * 9048 + 40) and n_in.value == 64 * (128 + 1 + 28)
    for n, dim, m in ((1, 4, 1), (8, 4, 0), (8, 4, 4097), (0, 4, 1)):
        assert lib.vdb_wit_merkle_update_size(n, dim, m, ctypes.byref(cells), ctypes.byref(n_in)) != 0, (n, dim, m)
