"""The device's verdict on single altered cells, for every hot path: the constraint map as the device placed it (downloaded from
ProverRounds.circuit after keygen) and the bytes the witness kernels wrote go through tests/alteration_model.py on the host — which
cells may be altered alone without notice, and is each of them free in the reference's circuit too (today: the inverse witness of an
is_zero whose operand is zero) — and then the device MockProver (vdb_mock_check_dev, vdb_mock_check_instances_dev) is asked on the
witness where it lies in HBM, 32 bytes overwritten at a time: every cell the model calls free must pass, a seeded sample of the
others must not and must give the six counts and first offenders of the model's recount, every public cell must miss its instance,
sampled lookup cells must miss their source.  Two alterations per cell, + 1 and a seeded random field element, with one verdict.
The Manhattan distance at dim 5 (933 cells) is swept whole.  tests/test_alteration_cpu.py does the same on host-built maps and the
oracle's witnesses, for every cell.

Per-call time of the device check, measured on an MI355X on the k-means circuit below (827,354 cells, mean of 8 calls): 0.09 ms
through the bare entry points with the map, the table and the public cells uploaded once, 0.42 ms through ProverRounds.mock_check,
which uploads the table and the public cells at every call.  The sweeps use the bare form (the recount on the host, not the device,
is what a sampled cell costs: about a millisecond) and send the first few cells of every circuit through ProverRounds.mock_check as
well; test_kmeans prints both times again."""
import time

import numpy as np
import pytest

import alteration_model as AM
import examples_common as E
from test_circuit_sym_cpu import to_ints
from test_gpu_rounds import TAU
from test_topk_cpu import separated_inputs

pytestmark = pytest.mark.gpu

CAP = 0.01
N_NOTICED, N_LOOKUP, N_THROUGH_ROUNDS = 1024, 64, 4


@pytest.fixture(scope="module")
def api():
    from halo2_vectordb_amd import api as a
    a.init(0)
    return a


class Checker:
    """vdb_mock_check_dev + vdb_mock_check_instances_dev on a stream and a lookup stream that stay where they are, the map, the
    constants' table, the public cells and their honest values uploaded once"""

    def __init__(self, api, O, d_stream, d_lookup, cm, L, public, instances):
        self.api, self.d_stream, self.d_lookup, self.L = api, d_stream, d_lookup, L
        self.n_cells, self.n_lookup, self.n_consts, self.n_public = cm.n_cells, len(cm.lookup_src), len(cm.consts), len(public)
        self.bufs = []
        self.p_flags = self._dev(np.asarray(cm.gate).astype(np.uint8))
        self.p_copy, self.p_cidx = self._dev(np.asarray(cm.copy_of, dtype=np.int64)), self._dev(np.asarray(cm.const_idx, dtype=np.int64))
        self.p_src = self._dev(np.asarray(cm.lookup_src, dtype=np.int64)) if self.n_lookup else None
        self.p_table = self._dev(O.fr_from_ints([int(v) for v in cm.consts]) if self.n_consts else np.zeros((1, 4), dtype=np.uint64))
        self.p_pub = self._dev(np.asarray(public, dtype=np.int64))
        self.p_inst = self._dev(O.fr_from_ints([int(v) for v in instances]) if self.n_public else np.zeros((1, 4), dtype=np.uint64))

    def _dev(self, a):
        a = np.ascontiguousarray(a)
        b = self.api.DeviceBuffer(max(a.nbytes, 32))
        if a.nbytes:
            b.upload(a)
        self.bufs.append(b)
        return b.ptr

    def __call__(self):
        rep = self.api.mock_check_dev(self.d_stream.ptr, self.n_cells, self.p_flags, self.d_lookup.ptr, self.n_lookup, self.L, self.p_copy, self.p_src, None,
                                      self.p_cidx, self.p_table, self.n_consts)
        return self.api.mock_check_instances_dev(rep, self.d_stream.ptr, self.n_cells, self.p_pub, self.p_inst, self.n_public)

    def free(self):
        for b in self.bufs:
            b.free()


def altered(O, rng, limbs):
    """the two replacements of one cell: + 1, and a random field element"""
    one = O.fr_add(limbs.reshape(1, 4), O.fr_from_ints([1]))
    while True:
        rnd = O.random_fr(rng, 1)
        if not np.array_equal(rnd[0], limbs):
            return [np.ascontiguousarray(one), np.ascontiguousarray(rnd)]


def verdicts(O, rng, d_buf, limbs, index, check):
    """`check()` with cell `index` of the device buffer replaced, both ways, the cell restored after each: [(new limbs, report)]"""
    out = []
    for new in altered(O, rng, limbs[index]):
        d_buf.upload(new, offset=index * 32)
        try:
            rep = check()
        finally:
            d_buf.upload(np.ascontiguousarray(limbs[index:index + 1]), offset=index * 32)
        out.append((new, rep))
    return out


def device_sweep(api, O, name, hp, measure=False):
    from halo2_vectordb_amd import circuit_sym as CS
    from halo2_vectordb_amd.rounds import ProverRounds
    pr = ProverRounds(hp).keygen()
    chk = d_flags = None
    try:
        assert pr.keygen_report.violations() == 0, pr.keygen_report.as_dict()
        dm = pr.circuit
        cm = CS.CopyMap(np.array(dm.copy_of), np.array(dm.const_idx), [int(v) for v in dm.consts], np.array(dm.asserted), np.array(dm.gate),
                        np.array(dm.lookup_src))
        hp._witness()
        api.sync()
        stream = hp.d_stream.download((hp.n_cells, 4))
        lookup = hp.d_lookup.download((hp.n_lookup, 4)) if hp.n_lookup else np.zeros((0, 4), dtype=np.uint64)
        vals, lks, public = to_ints(O, stream), to_ints(O, lookup), [int(c) for c in pr.instance_cells]
        inst = [vals[c] for c in public]
        assert cm.n_cells == hp.n_cells and len(cm.lookup_src) == hp.n_lookup and len(public) >= 1
        free = AM.unnoticed(cm, vals, lks, public)
        reasons = [AM.explain(cm, vals, c) for c in free]
        print(AM.summary(name, cm, free, reasons))
        unexplained = [c for c, r in zip(free, reasons) if r is None]
        assert not unexplained, f"{name}: cells {unexplained[:8]} ({len(unexplained)} in all) are tied to nothing and no gate notices them"
        assert len(free) <= CAP * cm.n_cells, (name, len(free), cm.n_cells)
        assert AM.unnoticed_lookups(cm, lks) == [], name

        chk = Checker(api, O, hp.d_stream, hp.d_lookup, cm, hp.L, public, inst)
        d_flags = api.DeviceBuffer(hp.n_cells)
        d_flags.upload(np.asarray(cm.gate).astype(np.uint8))
        through_rounds = lambda: pr.mock_check(d_flags, inst)
        assert chk().violations() == 0 and through_rounds().violations() == 0
        if measure:
            t0 = time.perf_counter()
            for _ in range(8):
                chk()
            t1 = time.perf_counter()
            for _ in range(8):
                through_rounds()
            t2 = time.perf_counter()
            print(f"per-call time of the device check, {hp.n_cells} cells: bare entry points {(t1 - t0) / 8 * 1e3:.2f} ms, "
                  f"ProverRounds.mock_check {(t2 - t1) / 8 * 1e3:.2f} ms")

        rng = np.random.default_rng(hp.n_cells)
        # every cell the model calls free: the device agrees, both ways
        for i, c in enumerate(free):
            for _new, rep in verdicts(O, rng, hp.d_stream, stream, c, through_rounds if i < N_THROUGH_ROUNDS else chk):
                assert rep.violations() == 0, (name, c, rep.as_dict())
        # a sample of the others: noticed, with the counts and first offenders of the recount
        is_free = np.zeros(cm.n_cells, dtype=bool)
        is_free[free] = True
        bound = np.flatnonzero(~is_free)
        for i, c in enumerate(rng.choice(bound, size=min(N_NOTICED, len(bound)), replace=False).tolist()):
            for new, rep in verdicts(O, rng, hp.d_stream, stream, c, through_rounds if i < N_THROUGH_ROUNDS else chk):
                honest, vals[c] = vals[c], to_ints(O, new)[0]
                want = AM.recount(cm, vals, lks, hp.L, public, inst, touched=([c], []))
                vals[c] = honest
                assert rep.violations() >= 1 and rep.as_dict() == want, (name, c, rep.as_dict(), want)
        # every public cell misses the value claimed for it
        for c in sorted(set(public)):
            for _new, rep in verdicts(O, rng, hp.d_stream, stream, c, chk):
                assert rep.instances_unequal >= 1 and rep.first_instance == public.index(c), (name, c, rep.as_dict())
        # lookup cells: each is a copy of its source
        for j in rng.choice(hp.n_lookup, size=min(N_LOOKUP, hp.n_lookup), replace=False).tolist() if hp.n_lookup else []:
            for new, rep in verdicts(O, rng, hp.d_lookup, lookup, j, chk):
                honest, lks[j] = lks[j], to_ints(O, new)[0]
                want = AM.recount(cm, vals, lks, hp.L, public, inst, touched=([], [j]))
                lks[j] = honest
                assert rep.lookup_copies_unequal == 1 and rep.as_dict() == want, (name, j, rep.as_dict(), want)
        # everything is back where it was
        assert np.array_equal(hp.d_stream.download((hp.n_cells, 4)), stream)
        assert chk().violations() == 0 and through_rounds().violations() == 0
    finally:
        if chk is not None:
            chk.free()
        if d_flags is not None:
            d_flags.free()
        pr.free()
        hp.free()


def test_kmeans(api, O):
    from halo2_vectordb_amd.pipeline import KmeansHotPath
    device_sweep(api, O, "k-means cosine n 8 dim 4 K 2 I 1", KmeansHotPath(n=8, dim=4, K=2, I=1, k=12, L=11, metric="cosine", tau=TAU).setup(), measure=True)


def test_query(api, O):
    from halo2_vectordb_amd.pipeline import QueryHotPath
    device_sweep(api, O, "query cosine n 6 dim 4", QueryHotPath(n=6, dim=4, k=12, L=11, metric="cosine", tau=TAU).setup())


def test_topk_query(api, O):
    from halo2_vectordb_amd.pipeline import TopKQueryHotPath
    v = separated_inputs("euclidean", 2, 4, 3, 2, seed=21)
    device_sweep(api, O, "top-k euclidean q 2 n 4 dim 3 t 2", TopKQueryHotPath(q=2, n=4, dim=3, topk=2, k=12, L=11, metric="euclidean", tau=TAU, vectors=v).setup())


def test_batch_query(api, O):
    from halo2_vectordb_amd.pipeline import BatchQueryHotPath
    v = separated_inputs("euclidean", 2, 4, 3, 2, seed=21)
    device_sweep(api, O, "batch euclidean q 2 n 4 dim 3", BatchQueryHotPath(q=2, n=4, dim=3, k=12, L=11, metric="euclidean", tau=TAU, vectors=v).setup())


def test_merkle(api, O):
    from halo2_vectordb_amd.pipeline import MerkleHotPath
    device_sweep(api, O, "merkle n 6 dim 5", MerkleHotPath(n=6, dim=5, k=11, tau=TAU).setup())


def test_merkle_update(api, O):
    from test_gpu_merkle_update import _hot_path
    device_sweep(api, O, "merkle update n 6 dim 4 m 4", _hot_path(6, 4, [4, 5, 6, 4], 21).setup())


def test_distances(api, O):
    from halo2_vectordb_amd.pipeline import DistancesHotPath
    d, cfg = E.load("distances"), E.README["distances"]
    hp = DistancesHotPath(dim=len(d["a"]), k=cfg["k"], L=cfg["L"], tau=TAU, vectors=np.array([d["a"], d["b"]], dtype=np.float64)).setup()
    device_sweep(api, O, "distances example", hp)


def test_fixed_point(api, O):
    from halo2_vectordb_amd.pipeline import FixedPointHotPath
    device_sweep(api, O, "fixed-point example", FixedPointHotPath(x=1.128, k=13, P=32, L=12, tau=TAU).setup())


def test_every_cell_of_a_manhattan_distance(api, O):
    """all 933 cells of the Manhattan distance at dim 5 (P 48, L 11), the map traced on the host and the witness from the library's
    host entry point: each cell both ways, the report against the recount of the whole witness, no violation exactly on the cells
    the model calls free"""
    from halo2_vectordb_amd import circuit_sym as CS
    dim, P, L = 5, 48, 11
    cm, outs = CS.trace_distance("manhattan", dim, P, L)
    v = np.random.default_rng(933).uniform(-3.0, 3.0, size=(2, dim))
    v[1, 0] = v[0, 0]
    qv = api.quantize(v, P)
    got = api.wit_distance("manhattan", qv[:1], qv[1:], P=P, L=L, selectors=True)
    stream = np.ascontiguousarray(np.concatenate([qv[0], qv[1], got["stream"]]))
    lookup = np.ascontiguousarray(got["lookup"])
    flags = np.concatenate([np.zeros(2 * dim, dtype=np.uint8), got["flags"]])
    assert stream.shape[0] == cm.n_cells == 933 and lookup.shape[0] == len(cm.lookup_src) and np.array_equal(flags & 1, cm.gate.astype(np.uint8))
    vals, lks, public = to_ints(O, stream), to_ints(O, lookup), [int(c) for c in outs]
    inst = [vals[c] for c in public]
    free = AM.unnoticed(cm, vals, lks, public)
    reasons = [AM.explain(cm, vals, c) for c in free]
    print(AM.summary("manhattan dim 5, every cell on the device", cm, free, reasons))
    assert None not in reasons and 1 <= len(free) <= CAP * cm.n_cells
    d_stream, d_lookup = api.DeviceBuffer(stream.nbytes), api.DeviceBuffer(max(lookup.nbytes, 32))
    chk = None
    try:
        d_stream.upload(stream)
        d_lookup.upload(lookup)
        chk = Checker(api, O, d_stream, d_lookup, cm, L, public, inst)
        assert chk().violations() == 0
        rng = np.random.default_rng(5)
        for c in range(cm.n_cells):
            for new, rep in verdicts(O, rng, d_stream, stream, c, chk):
                alt = vals.copy()
                alt[c] = to_ints(O, new)[0]
                assert rep.as_dict() == AM.recount(cm, alt, lks, L, public, inst), (c, rep.as_dict())
                assert (rep.violations() == 0) == (c in free), (c, rep.as_dict())
        for j in range(len(lks)):
            for new, rep in verdicts(O, rng, d_lookup, lookup, j, chk):
                alt = lks.copy()
                alt[j] = to_ints(O, new)[0]
                assert rep.lookup_copies_unequal == 1 and rep.as_dict() == AM.recount(cm, vals, alt, L, public, inst), (j, rep.as_dict())
        assert chk().violations() == 0
    finally:
        if chk is not None:
            chk.free()
        d_stream.free()
        d_lookup.free()


def test_guards_of_the_mock_kernels(api, O):
    """k_mock_cells and k_mock_lookups test every index they are handed before they load through it: a gate flag on one of the last
    three cells, a copy source outside the stream, a constant index outside the table, a lookup source below zero or outside the stream,
    and lookup cells with no stream at all — each reported as a violation of its own kind and nothing else, as the recount counts
    them.  (The indices are just outside: a check that failed to guard them would still read inside the allocation's granule.)"""
    from halo2_vectordb_amd import circuit_sym as CS
    L, n = 4, 8
    vals = np.array([1, 2, 3, 7, 5, 0, 9, 5], dtype=object)                          # gates at 0 and 4: 1 + 2 * 3 = 7, 5 + 0 * 9 = 5
    stream = O.fr_from_ints([int(v) for v in vals])

    def base():
        gate = np.zeros(n, dtype=bool)
        gate[[0, 4]] = True
        const_idx = np.full(n, -1, dtype=np.int64)
        const_idx[7] = 0
        return CS.CopyMap(np.arange(n, dtype=np.int64), const_idx, [5], np.zeros(n, dtype=bool), gate, np.array([2, 2], dtype=np.int64)), [3, 3]

    def run(cm, lks, n_cells=n):
        lookup = O.fr_from_ints(lks)
        d_stream, d_lookup = api.DeviceBuffer(stream.nbytes), api.DeviceBuffer(lookup.nbytes)
        chk = None
        try:
            d_stream.upload(stream)
            d_lookup.upload(lookup)
            chk = Checker(api, O, d_stream, d_lookup, cm, L, [], [])
            got = chk().as_dict()
        finally:
            if chk is not None:
                chk.free()
            d_stream.free()
            d_lookup.free()
        want = AM.recount(cm, vals[:n_cells], lks, L)
        assert got == want, (got, want)
        return got

    def only(rep, name, count, first):
        assert rep[name] == count and rep[dict(AM.KINDS)[name]] == first, rep
        assert AM.violations(rep) == count, rep

    cm, lks = base()
    only(run(cm, lks), "gate_rows_violated", 0, AM.NONE)
    cm, lks = base()
    cm.gate[[5, 6, 7]] = True
    only(run(cm, lks), "gate_rows_violated", 3, 5)
    cm, lks = base()
    cm.copy_of[3], cm.copy_of[6] = n, n + 1
    only(run(cm, lks), "copies_unequal", 2, 3)
    cm, lks = base()
    cm.const_idx[4], cm.const_idx[5] = 1, 2
    only(run(cm, lks), "constants_changed", 2, 4)
    cm, lks = base()
    cm.lookup_src[:] = [-1, n]
    only(run(cm, lks), "lookup_copies_unequal", 2, 0)
    # no stream at all: every lookup cell is without its source
    none = np.zeros(0, dtype=np.int64)
    empty = CS.CopyMap(none, none, [], np.zeros(0, dtype=bool), np.zeros(0, dtype=bool), np.array([0, 0], dtype=np.int64))
    only(run(empty, [3, 3], n_cells=0), "lookup_copies_unequal", 2, 0)
