"""The batch query circuit without a GPU: q queries against one assigned database — assign the queries, assign the database,
nearest_vector per query (src/gadget/vectordb.rs:122-163), the closure a user of the reference's chips would write.  The block-built
constraint map (circuit_sym.build_nearest_batch) is the whole-circuit trace (trace_nearest_batch), both accept the oracle's witness
of that closure and catch an altered result, indicator or distance input, q = 1 is the single-query circuit, and the library exports
the batch entry points."""
import ctypes
import os

import numpy as np
import pytest

from halo2_vectordb_amd import circuit_sym as CS
from test_circuit_sym_cpu import clean, to_ints

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P, L = 48, 11
SHAPES = [("euclidean", 3, 5, 4), ("cosine", 2, 4, 3), ("manhattan", 4, 3, 2)]
FIELDS = ("copy_of", "const_idx", "asserted", "gate", "lookup_src")


def same_map(a, b):
    """the two maps tie every cell to the same cell or the same constant VALUE (constants are numbered by first use)"""
    for name in FIELDS:
        x, y = getattr(a, name), getattr(b, name)
        if name == "const_idx":
            x = np.where(x >= 0, np.asarray(a.consts + [0], dtype=object)[x], -1)
            y = np.where(y >= 0, np.asarray(b.consts + [0], dtype=object)[y], -1)
        assert np.array_equal(x, y), name


def oracle_batch(O, metric, queries, db):
    """the oracle's context run in the circuit's order; -> (context, [(indicator, result)] per query)"""
    c = O.Ctx(store=True, keygen=True)
    c.assign_witnesses(queries)
    c.assign_witnesses(db)
    outs = [c.nearest_vector(metric, qq, db, P=P, L=L) for qq in queries]
    return c, outs


@pytest.mark.parametrize("metric,q,n,dim", SHAPES)
def test_block_built_map_is_the_whole_circuit_trace(metric, q, n, dim):
    cm, (ind, res) = CS.trace_nearest_batch(metric, q, n, dim, P, L)
    bm, (bind, bres) = CS.build_nearest_batch(metric, q, n, dim, P, L)
    same_map(cm, bm)
    assert np.array_equal(np.asarray(ind), bind) and np.array_equal(np.asarray(res), bres)
    assert bind.shape == (q, n) and bres.shape == (q, dim)
    # every query's distances read the SAME database cells: each is copied once per query at least (the selects copy them too)
    db_cells = q * dim + np.arange(n * dim)
    assert all(int((cm.copy_of == cell).sum()) >= 2 * q for cell in db_cells)
    # ... and a query's cells are read by its own n distances only
    single, _ = CS.trace_nearest(metric, n, dim, P, L)
    for cell in range(q * dim):
        assert int((cm.copy_of == cell).sum()) == int((single.copy_of == cell % dim).sum())


@pytest.mark.parametrize("metric,n,dim", [("euclidean", 5, 4), ("cosine", 4, 3), ("manhattan", 1, 2)])
def test_a_batch_of_one_is_the_single_query_circuit(metric, n, dim):
    one, (ind1, res1) = CS.trace_nearest(metric, n, dim, P, L)
    cm, (ind, res) = CS.trace_nearest_batch(metric, 1, n, dim, P, L)
    bm, (bind, bres) = CS.build_nearest_batch(metric, 1, n, dim, P, L)
    b1, (bind1, bres1) = CS.build_nearest(metric, n, dim, P, L)
    same_map(one, cm)
    same_map(one, bm)
    same_map(b1, bm)
    assert ind[0] == ind1 and res[0] == res1 and list(bind[0]) == list(bind1) and list(bres[0]) == list(bres1)


def test_builder_contract_leaves_room_for_the_commitment():
    """builder= / extra_cells= / finish= as for build_nearest: the builder comes back with the cells used, so that circuit_sym.place_merkle can follow"""
    metric, q, n, dim = SHAPES[0]
    whole, _ = CS.build_nearest_batch(metric, q, n, dim, P, L)
    B, (ind, res), used = CS.build_nearest_batch(metric, q, n, dim, P, L, builder=CS._Builder, extra_cells=77, finish=False)
    assert used == whole.n_cells and B.copy_of.shape[0] == used + 77
    cm = B.finish()
    assert np.array_equal(cm.copy_of[:used], whole.copy_of) and np.array_equal(cm.copy_of[used:], np.arange(used, used + 77))
    assert not cm.gate[used:].any() and (cm.const_idx[used:] == -1).all()


@pytest.mark.parametrize("metric,q,n,dim", SHAPES)
def test_map_accepts_the_oracles_witness_and_catches_altered_cells(O, metric, q, n, dim):
    rng = np.random.default_rng(q * 100 + n * 10 + dim)
    queries, db = O.quantize(rng.random((q, dim)) + 0.1, P), O.quantize(rng.random((n, dim)) + 0.1, P)
    c, outs = oracle_batch(O, metric, queries, db)
    assert c.err == 0
    bm, (ind, res) = CS.build_nearest_batch(metric, q, n, dim, P, L)
    assert len(c) == bm.n_cells and c.n_lookup == len(bm.lookup_src)
    vals, lk = to_ints(O, c.advice()), to_ints(O, c.lookup())
    ok, bad = clean(bm.check_witness(vals, lk, flags=c.selectors()))
    assert ok, bad
    for i, (o_ind, o_res) in enumerate(outs):                   # the map's output cells hold the oracle's outputs, query by query
        assert [vals[x] for x in ind[i]] == list(to_ints(O, o_ind)) and [vals[x] for x in res[i]] == list(to_ints(O, o_res))
        assert sum(int(v) for v in to_ints(O, o_ind)) >= 1

    starts = np.flatnonzero(bm.gate)

    def gate_violations(v):
        """halo2-base's one gate on the map's gate starts: a + b c = d over four consecutive cells"""
        return int(np.count_nonzero((v[starts] + v[starts + 1] * v[starts + 2] - v[starts + 3]) % CS.R))

    def violations(cell):
        """the cell altered alone: (what the copies, constants and lookups notice, what the gates notice)"""
        alt = vals.copy()
        alt[cell] = (alt[cell] + 1) % CS.R
        rep = bm.check_witness(alt, lk)
        return rep["copies_unequal"] + rep["constants_wrong"] + rep["asserts_violated"] + rep["lookup_copies_unequal"], gate_violations(alt)

    assert gate_violations(vals) == 0
    for i in (0, q - 1):
        # a result cell (the last cell of its running select; the instance column is what copies it in the whole circuit): its own gate
        assert violations(int(res[i][dim - 1]))[1] >= 1
        # an indicator cell: it copies is_zero's output and every select of that query copies it
        assert violations(int(ind[i][0]))[0] >= dim + 1
        # ... and one of those copies altered instead: unequal to the indicator
        users_of_ind = np.flatnonzero(bm.copy_of == ind[i][0])
        assert users_of_ind.size == dim and violations(int(users_of_ind[0]))[0] >= 1
        # a distance input: the query's own word 0 as its first distance holds it
        users_of_query = np.flatnonzero(bm.copy_of == i * dim)
        assert users_of_query.size >= n and violations(int(users_of_query[0]))[0] >= 1
    # a database word as the last query's distances hold it (every query copies the same assigned cell)
    users_of_db = np.flatnonzero(bm.copy_of == q * dim)
    assert users_of_db.size >= 2 * q and violations(int(users_of_db[-1]))[0] >= 1


def test_library_exports_the_batch_entry_points():
    lib_path = os.path.join(ROOT, "halo2_vectordb_amd", "libvdb_hip.so")
    if not os.path.exists(lib_path):
        import __graft_entry__ as g
        g.build()
    lib = ctypes.CDLL(lib_path)
    for name in ("vdb_wit_nearest_batch_size", "vdb_wit_nearest_batch", "vdb_wit_nearest_batch_dev"):
        assert hasattr(lib, name), name
    header = open(os.path.join(ROOT, "include", "vdb.h")).read()
    assert "VDB_NEAREST_BATCH_MAX_INSTANCES" in header and "int vdb_wit_nearest_batch_dev(" in header
    from halo2_vectordb_amd import _lib, api
    assert all(name in _lib._SIGNATURES for name in ("vdb_wit_nearest_batch_size", "vdb_wit_nearest_batch", "vdb_wit_nearest_batch_dev"))
    assert callable(api.wit_nearest_batch)
