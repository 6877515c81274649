"""The Merkle opening circuit without a GPU.  tests/merkle_open_model.py is the checker of the GPU streams, so nothing of it is taken on
trust: its hash blocks are the oracle's merkle_commitment contexts, its root the oracle's poseidon_merkle_root; the block-built
constraint map (circuit_sym.build_merkle_open) is the cell-by-cell trace, accepts the model's witness, ties every later read's top to
read 0's, and binds every cell (single-cell alteration sweep); and the library exports the entry points."""
import ctypes
import os

import numpy as np
import pytest

import alteration_model as AM
import merkle_open_model as MO
import merkle_update_model as MU
import topk_model as TM
from halo2_vectordb_amd import circuit_sym as CS
from test_batch_query_cpu import same_map
from test_merkle_update_cpu import database, fetchers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (n, dim, reads): depth 1 and 3, odd dim, a repeated slot, the first and last leaf, padding slots (leaf mode only where >= n)
CASES = {
    "depth1": (2, 4, [1]),
    "depth1_odd_dim": (2, 5, [0, 1]),
    "repeat_first_last": (8, 4, [0, 7, 0, 3]),
    "padding": (6, 5, [4, 5, 6, 7]),
    "sweep_shape": (6, 4, [2, 5, 2]),
}


def model(O, n, dim, reads, with_vectors, seed=7, plan_k=None):
    db = database(O, n, dim, seed)
    levels = MU.build_tree(O, db)
    reads = [i for i in reads if i < n] if with_vectors else reads
    m = MO.open_model(O, levels, reads, db[reads] if with_vectors else None, plan_k=plan_k)
    return m, levels, db, reads


def kernel_like_flags(m, dim, depth, n_reads, with_vectors):
    """test_merkle_update_cpu.kernel_like_flags for the opening's layout: the model's gate bits plus the constant bit on the constant
    cells of every permutation, found by the tracer whose gate bits must equal the model's"""
    from halo2_vectordb_amd import copymap as CM
    lay = CS.merkle_open_layout(n_reads, dim, depth, with_vectors)
    flags = m["selectors"].astype(np.uint8).copy()
    vals = TM.to_ints(m["advice"])

    def mark(at, n_in):
        size = CM.perm_cells(n_in)
        t = CM._Tracer(None)
        t.next_is_const = lambda: vals[at + len(t.src)] == 0 and vals[at + len(t.src) + 3] == vals[at + len(t.src) + 1] * vals[at + len(t.src) + 2] % CS.R
        CM._trace_permutation(t, n_in)
        assert len(t.src) == size and np.array_equal(np.asarray(t.gate, dtype=np.uint8), flags[at:at + size] & 1)
        flags[at:at + size] |= np.asarray(t.cst, dtype=np.uint8) << 1

    for j in range(n_reads):
        at = lay["n_in"] + j * lay["per_read"]
        for p in range(lay["nperm"]):
            mark(at, lay["n_ins"][p])
            at += lay["sizes"][p]
        for _ in range(depth):
            mark(at + 20, 2)
            mark(at + 20 + CM.perm_cells(2), 0)
            at += lay["level_cells"]
    return flags


@pytest.mark.parametrize("with_vectors", [True, False], ids=["vector", "leaf"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_hash_blocks_are_the_oracles_and_the_root_is_the_commitments(O, name, with_vectors):
    n, dim, reads = CASES[name]
    m, levels, db, reads = model(O, n, dim, reads, with_vectors, plan_k=12)
    k, depth = len(reads), len(levels) - 1
    lay = CS.merkle_open_layout(k, dim, depth, with_vectors)
    assert m["advice"].shape[0] == lay["total"] and m["n_in"] == lay["n_in"]
    assert np.array_equal(m["public"][0], O.poseidon_merkle_root(db))
    assert TM.to_ints(m["public"][1:1 + 2 * k:2]) == reads
    assert len(m["public"]) == 1 + 2 * k + (k * dim if with_vectors else 0)
    for j, idx in enumerate(reads):
        reg, leaf = m["regions"][j], m["public"][2 + 2 * j]
        assert reg["block"] == lay["n_in"] + j * lay["per_read"]
        assert np.array_equal(leaf, O.poseidon_hash_many(db[idx:idx + 1])[0] if idx < n else MU.ZERO), "a padding slot shows leaf 0"
        if with_vectors:
            # the leaf sponge is the oracle's merkle_commitment of the one vector, and the public words are the vector's
            c = O.Ctx(store=True, keygen=True)
            assert np.array_equal(c.merkle_commitment(db[idx:idx + 1]), leaf)
            assert np.array_equal(m["advice"][reg["block"]: reg["block"] + len(c)], c.advice()) and len(c) == lay["leaf_cells"]
            assert np.array_equal(m["public"][1 + 2 * k + j * dim: 1 + 2 * k + (j + 1) * dim], db[idx])
        for l, at in enumerate(reg["levels"]):
            assert at == reg["block"] + lay["leaf_cells"] + l * lay["level_cells"]
            node = idx >> l
            pair = [levels[l][node & ~1], levels[l][node | 1]]
            c = O.Ctx(store=True, keygen=True)
            assert np.array_equal(c.merkle_commitment(np.stack(pair)[None]), levels[l + 1][node >> 1])
            assert np.array_equal(m["advice"][at + 20: at + lay["level_cells"]], c.advice()) and len(c) == lay["node_cells"]
            assert np.array_equal(m["selectors"][at + 20: at + lay["level_cells"]], c.selectors().astype(np.uint8) & 1)
        assert reg["index"] + lay["ip_cells"] == reg["block"] + lay["per_read"]
        assert np.array_equal(m["advice"][reg["top"]], m["public"][0])


@pytest.mark.parametrize("with_vectors", [True, False], ids=["vector", "leaf"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_map_is_the_trace_and_accepts_the_model(O, name, with_vectors):
    n, dim, reads = CASES[name]
    m, levels, _db, reads = model(O, n, dim, reads, with_vectors)
    k, depth = len(reads), len(levels) - 1
    m["flags"] = kernel_like_flags(m, dim, depth, k, with_vectors)
    ff, fv, vals = fetchers(m)
    tm, tpub = CS.trace_merkle_open(k, dim, depth, with_vectors, ff, fv)
    bm, bpub = CS.build_merkle_open(k, dim, depth, with_vectors, ff, fv)
    same_map(tm, bm)
    assert tpub == bpub and len(bpub) == 1 + 2 * k + (k * dim if with_vectors else 0)
    assert bm.n_cells == m["advice"].shape[0] and len(bm.lookup_src) == 0
    inst = TM.to_ints(m["public"])
    assert [vals[c] for c in bpub] == inst
    rep = AM.recount(bm, vals, [], None, bpub, inst)
    assert AM.violations(rep) == 0, rep
    # the ties: the top of read j >= 1 copies the top of read 0, which is the public root; nothing else crosses between reads
    lay = CS.merkle_open_layout(k, dim, depth, with_vectors)
    assert bpub[0] == m["regions"][0]["top"]
    for j in range(1, k):
        blk = m["regions"][j]["block"]
        crossing = [c for c in range(blk, blk + lay["per_read"]) if lay["n_in"] <= bm.copy_of[c] < blk]
        assert crossing == [m["regions"][j]["top"]] and (crossing[0], int(bm.copy_of[crossing[0]])) == m["ties"][j - 1]
    held = {int(bm.consts[i]) for i in set(bm.const_idx[bm.const_idx >= 0].tolist())}
    assert {1 << l for l in range(depth)} <= held and (1 << 64) in held


@pytest.mark.parametrize("with_vectors", [True, False], ids=["vector", "leaf"])
def test_every_cell_altered_alone_is_noticed(O, with_vectors):
    """no cell of an opening is legitimately free: no is_zero is used, so alteration_model.explain's one reason cannot apply and the
    list of excused cells is empty"""
    n, dim, reads = CASES["sweep_shape"]
    m, levels, _db, reads = model(O, n, dim, reads, with_vectors)
    k, depth = len(reads), len(levels) - 1
    m["flags"] = kernel_like_flags(m, dim, depth, k, with_vectors)
    ff, fv, vals = fetchers(m)
    excused = {}                                              # cell -> reason; none
    for name, (cm, pub) in (("trace", CS.trace_merkle_open(k, dim, depth, with_vectors, ff, fv)), ("build", CS.build_merkle_open(k, dim, depth, with_vectors, ff, fv))):
        free = AM.unnoticed(cm, vals, [], pub)
        print(AM.summary(f"merkle open ({name}) n {n} dim {dim} m {k} {'vector' if with_vectors else 'leaf'} mode", cm, free, [excused.get(c) for c in free]))
        assert [c for c in free if c not in excused] == []
        # the model's verdict against a recount of the altered witness: an input bit, a sibling, the lead cell, the tied top, an index sum
        lay = CS.merkle_open_layout(k, dim, depth, with_vectors)
        inst = [vals[c] for c in pub]
        for cell in (lay["bits"] + depth + 1, lay["sibs"] + 2, 0, m["regions"][1]["top"], m["regions"][2]["index"] + lay["ip_cells"] - 1):
            alt = vals.copy()
            alt[cell] = (alt[cell] + 1) % CS.R
            assert AM.violations(AM.recount(cm, alt, [], None, pub, inst, touched=([cell], []))) >= 1, (name, cell)


def test_a_vector_that_is_not_the_committed_one_breaks_a_copy(O):
    """the entry point does not compare the vectors with the tree: with a foreign vector (or a stale tree) the `cur` cells of level 0
    hold the tree's leaf while the squeeze cell holds the vector's hash, and the copy between them is unequal"""
    n, dim, reads = 6, 4, [2, 5]
    m, levels, db, reads = model(O, n, dim, reads, True)
    depth = len(levels) - 1
    m["flags"] = kernel_like_flags(m, dim, depth, 2, True)
    ff, fv, vals = fetchers(m)
    cm, pub = CS.build_merkle_open(2, dim, depth, True, ff, fv)
    lay = CS.merkle_open_layout(2, dim, depth, True)
    squeeze = pub[2]
    users = np.flatnonzero(cm.copy_of == squeeze)
    users = users[users != squeeze]
    assert len(users) == 3 and (users >= lay["n_in"] + lay["leaf_cells"]).all() and (users < lay["n_in"] + lay["leaf_cells"] + 20).all()
    alt = vals.copy()
    alt[squeeze] = (alt[squeeze] + 1) % CS.R
    assert AM.recount(cm, alt, [], None, pub, [vals[c] for c in pub])["copies_unequal"] == 3


def test_layout_counts_and_refused_shapes():
    for args in ((0, 4, 2, True), (2, 4, 0, False), (2, 0, 2, True)):
        with pytest.raises(ValueError):
            CS.merkle_open_layout(*args)
    lay = CS.merkle_open_layout(64, 128, 14, True)
    assert lay["leaf_cells"] == 146634 and lay["level_cells"] == 4526 and lay["per_read"] == 146634 + 14 * 4526 + 40 == 210038
    assert lay["n_in"] == 64 * (128 + 28) and lay["total"] == lay["n_in"] + 64 * 210038
    lay = CS.merkle_open_layout(64, 128, 14, False)
    assert lay["leaf_cells"] == 0 and lay["per_read"] == 63404 and lay["n_in"] == 64 * 29


def test_library_exports_the_open_entry_points():
    lib_path = os.path.join(ROOT, "halo2_vectordb_amd", "libvdb_hip.so")
    if not os.path.exists(lib_path):
        import __graft_entry__ as g
        g.build()
    lib = ctypes.CDLL(lib_path)
    names = ("vdb_wit_merkle_open_size", "vdb_wit_merkle_open", "vdb_wit_merkle_open_dev")
    for name in names:
        assert hasattr(lib, name), name
    header = open(os.path.join(ROOT, "include", "vdb.h")).read()
    assert "VDB_MERKLE_OPEN_MAX_CELLS" in header and "int vdb_wit_merkle_open_dev(" in header
    from halo2_vectordb_amd import _lib, api, pipeline
    assert all(name in _lib._SIGNATURES for name in names)
    assert callable(api.wit_merkle_open) and hasattr(pipeline, "ReadHotPath")
    # the size entry needs no device: the cell counts are confirmed and the limits of one call refused there
    lib.vdb_wit_merkle_open_size.argtypes = [ctypes.c_size_t] * 3 + [ctypes.c_int] + [ctypes.c_void_p] * 2
    cells, n_in = ctypes.c_uint64(), ctypes.c_uint64()
    assert lib.vdb_wit_merkle_open_size(16384, 128, 64, 1, ctypes.byref(cells), ctypes.byref(n_in)) == 0
    assert cells.value == 64 * (128 + 28) + 64 * 210038 and n_in.value == 64 * (128 + 28)
    assert lib.vdb_wit_merkle_open_size(16384, 128, 64, 0, ctypes.byref(cells), ctypes.byref(n_in)) == 0
    assert cells.value == 64 * 29 + 64 * 63404 and n_in.value == 64 * 29
    assert lib.vdb_wit_merkle_open_size(16384, 128, 5000, 0, ctypes.byref(cells), ctypes.byref(n_in)) == 0, "no 4,096 cap on m"
    refused = ((8, 4, 0), (1, 4, 1), (0, 4, 1), (8, 0, 1), ((1 << 30) + 1, 4, 1), (8, (1 << 20) + 1, 1), (1 << 30, 4, 1 << 27), (8, 4, 1 << 31),
               (16384, 128, 1 << 17))
    for n, dim, m in refused:
        for mode in (0, 1):
            if (n, dim, m, mode) == (16384, 128, 1 << 17, 0):
                continue                                      # 2^17 leaf-mode reads at depth 14 are 8.3 G cells: allowed
            assert lib.vdb_wit_merkle_open_size(n, dim, m, mode, ctypes.byref(cells), ctypes.byref(n_in)) == -3, (n, dim, m, mode)
