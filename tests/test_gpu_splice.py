"""The splice sweep of tests/splice_model.py on the hot paths, and the device's verdict on witnesses that differ from an honest one in
MANY cells.  Per hot path of tests/test_gpu_alteration.py, at its size there: keygen once (the map is data independent), then the
witness kernels run on the inputs and again on inputs that differ in one coordinate (HotPath.set_vectors); the map as the device
placed it and both streams the kernels wrote come back, the model finds the pieces and the cuts, and tests/test_splice_cpu.py's
assertions hold: the altered input is among the changed cells, some perturbation reaches a public cell, no cut is unexplained, the
is_zero cuts are at most 1 % of the circuit, a Hamming distance has exactly its tail after `ab_sum_q` (the reference's
src/gadget/distance.rs:165-169 loads it with load_witness).  Both streams are honest by the device's own check.

Then the device MockProver (vdb_mock_check_dev, vdb_mock_check_instances_dev, through test_gpu_alteration.Checker) is asked on
hybrids written into HBM over the honest stream, the instance column being the hybrid's own public cells:
  every explained cut's hybrid gives 0 violations;
  64 seeded suffix splices per circuit — the changed cells at or after a sampled changed cell, with the lookup cells they feed,
    taken from the other stream — give exactly the six counts and first offenders of alteration_model.recount, and at least one
    violation unless the suffix is a union of explained cuts; every eighth is also held against the honest instance column.  These
    are the suite's many-cell alterations: hundreds of simultaneous violations, first offenders from different workgroups of
    k_mock_cells and k_mock_lookups;
  one copy constraint that alone holds a part of the changed cells to the input (splice_model.bridge_ties) is removed from a copy
    of the downloaded map, never from the product: the sweep names the cut it opens, its hybrid passes the device check under the
    weakened map with 0 violations and is noticed under the real one, with the recount's numbers;
  afterwards the stream is byte-equal to the honest one and the honest check is clean.

Wall time of one circuit's sweep on an MI355X, both perturbations with the suffix splices and the dropped tie (set-up, keygen and the
witness runs excluded; every test prints its own, "splice sweep of ..."): k-means cosine (827,354 cells) 1.59 s, query cosine (379,919)
0.74 s, top-k (226,664) 0.87 s, batch (225,358) 0.59 s, Merkle (72,163) 0.33 s, Merkle update (135,696) 0.36 s, the distances example
(73,980) 0.37 s, the fixed-point example (25,381) 0.10 s, the ANN query (220,558) 1.29 s.  Nearly all of it is the host's integers: the
links of the changed cells and the recount of every splice; a device check is a fraction of a millisecond.  The suffix splices put up
to 278 simultaneous violations through one check (batch; 261 top-k, 270 distances, 58 k-means).

Of the ANN hot paths that call device_sweep, the query is swept at its shape "5" (K 1, five members): its `query` is a free vector.
Not swept here:
  the ANN query at "1-1" (K 2, one member each): within the cluster the hot path was built for, no move of the query reaches a public
    cell (the result is that cluster's only member, the index root does not read the query), which assertion (3) refuses;
  ANN update: its new rows lie inside the update block, not at the head of the stream, and the old leaves and siblings of later writes
    follow an earlier row as further inputs — the one-input form of this sweep does not describe it;
  ANN delete: its inputs are slots, which lay the stream out;
  ANN audit, mean, recentre, cover: the constructors take an index and a cluster; the members and centroids are read from the resident
    index (the `members=` / `centroids=` overrides are quantized copies for the binding tests and would have to be moved together:
    a mean with its members, a centroid with its routing), so no single input value can be varied through them."""
import time

import numpy as np
import pytest

import alteration_model as AM
import examples_common as E
import splice_model as SM
from test_circuit_sym_cpu import to_ints
from test_gpu_alteration import Checker
from test_gpu_rounds import TAU
from test_splice_cpu import judge
from test_topk_cpu import separated_inputs

pytestmark = pytest.mark.gpu

N_SUFFIX = 64


@pytest.fixture(scope="module")
def api():
    from halo2_vectordb_amd import api as a
    a.init(0)
    return a


class Device:
    """the stream and the lookup stream in HBM with host mirrors of what lies there; `show` uploads the span that differs"""

    def __init__(self, O, chk, d_stream, d_lookup, stream, lookup, public):
        self.O, self.chk, self.bufs, self.public = O, chk, (d_stream, d_lookup), public
        self.now = [stream.copy(), lookup.copy()]

    def show(self, stream, lookup):
        for k, want in enumerate((stream, lookup)):
            rows = np.flatnonzero((self.now[k] != want).any(axis=1)) if len(want) else []
            if len(rows):
                lo, hi = int(rows[0]), int(rows[-1]) + 1
                self.bufs[k].upload(np.ascontiguousarray(want[lo:hi]), offset=lo * 32)
                self.now[k][lo:hi] = want[lo:hi]

    def report(self, claimed=None):
        """the device's report on what lies in HBM; the instance column: `claimed` limbs, None: the stream's own public cells"""
        inst = self.now[0][self.public] if claimed is None else claimed
        if len(self.public):
            self.chk.bufs[-1].upload(np.ascontiguousarray(inst))
        return self.chk().as_dict()


def hybrid(base, other, piece):
    """(stream, lookup) limbs of `base` with `other` written into the piece (cells, lookup cells)"""
    s, l = base[0].copy(), base[1].copy()
    s[piece[0]] = other[0][piece[0]]
    if len(piece[1]):
        l[piece[1]] = other[1][piece[1]]
    return s, l


def downloaded_map(pr):
    from halo2_vectordb_amd import circuit_sym as CS
    dm = pr.circuit
    return CS.CopyMap(np.array(dm.copy_of), np.array(dm.const_idx), [int(v) for v in dm.consts], np.array(dm.asserted), np.array(dm.gate),
                      np.array(dm.lookup_src))


def streams(api, hp):
    hp._witness()
    api.sync()
    return hp.d_stream.download((hp.n_cells, 4)), hp.d_lookup.download((hp.n_lookup, 4)) if hp.n_lookup else np.zeros((0, 4), dtype=np.uint64)


def device_splice(api, O, name, hp, moves, hamming_ends=()):
    """`hp`: the hot path, set up (freed here); `moves`: its input rows -> [(what, row, place, new value)]; `hamming_ends`: per
    Hamming distance of the circuit the first cell after it"""
    from halo2_vectordb_amd.rounds import ProverRounds
    pr = ProverRounds(hp).keygen()
    chk = None
    try:
        assert pr.keygen_report.violations() == 0, pr.keygen_report.as_dict()
        cm, public, n, L = downloaded_map(pr), [int(c) for c in pr.instance_cells], hp.n_cells, hp.L
        assert cm.n_cells == n and len(cm.lookup_src) == hp.n_lookup and len(public) >= 1
        loaded = SM.loaded_witnesses(cm, hp.n_in)
        assert len(loaded) == 2 * len(hamming_ends), loaded
        hamming = [(a, b, e) for a, b, e in zip(loaded[::2], loaded[1::2], hamming_ends)]
        rows = hp.vectors_f64.copy()
        honest = streams(api, hp)
        chk = Checker(api, O, hp.d_stream, hp.d_lookup, cm, L, public, [0] * len(public))
        dev = Device(O, chk, hp.d_stream, hp.d_lookup, honest[0], honest[1], public)
        assert AM.violations(dev.report()) == 0
        reached, spent = False, 0.0
        checker_for = lambda m: Checker(api, O, hp.d_stream, hp.d_lookup, m, L, public, [0] * len(public))
        for first, (what, i, j, new) in enumerate(moves(rows)):
            w = rows.copy()
            w[i, j] = new
            hp.set_vectors(w)
            other = streams(api, hp)
            hp.set_vectors(rows)
            dev.now = [other[0].copy(), other[1].copy()]
            assert AM.violations(dev.report()) == 0, (name, what)                       # (1) the second stream is honest too
            dev.show(*honest)
            t0 = time.perf_counter()
            D, DL = SM.changed(honest[0], other[0], honest[1], other[1])
            need = SM.needed(cm, D, DL, public)
            W, W2 = (SM.sparse(n, need, to_ints(O, s[0][need])) for s in (honest, other))
            LK, LK2 = (SM.sparse(hp.n_lookup, DL, to_ints(O, s[1][DL]) if len(DL) else []) for s in (honest, other))
            got = judge(f"{name}, {what}", cm, hp.n_in, W, W2, LK, LK2, D, DL, i * rows.shape[1] + j, public, L, hamming)
            reached |= got["public"]
            sides = ((honest, other, W, W2, LK, LK2), (other, honest, W2, W, LK2, LK))
            # every explained cut's hybrid passes on the device
            for c in got["found"]:
                base, alt = sides[c["direction"]][:2]
                dev.show(*hybrid(base, alt, (c["cells"], c["lookups"])))
                rep = dev.report()
                assert AM.violations(rep) == 0, (name, what, SM.describe(cm, c), rep)
            dev.show(*honest)
            if first == 0:
                suffix_splices(name, cm, dev, honest, other, W, W2, LK, LK2, D, DL, got, public, L)
                dropped_tie(name, cm, dev, checker_for, hp.n_in, honest, other, W, W2, LK, LK2, D, DL, i * rows.shape[1] + j, public, L)
            spent += time.perf_counter() - t0
        assert reached, f"{name}: no perturbation reaches a public cell"                  # (3)
        # everything is back where it was
        assert np.array_equal(hp.d_stream.download((n, 4)), honest[0])
        assert not hp.n_lookup or np.array_equal(hp.d_lookup.download((hp.n_lookup, 4)), honest[1])
        assert AM.violations(dev.report()) == 0
        print(f"splice sweep of {name}: {n} cells, {first + 1} perturbations, {spent:.2f} s")
    finally:
        if chk is not None:
            chk.free()
        pr.free()
        hp.free()


def suffix_splices(name, cm, dev, honest, other, W, W2, LK, LK2, D, DL, got, public, L):
    """N_SUFFIX seeded suffixes of D from the other stream written over the honest one"""
    rng = np.random.default_rng(cm.n_cells)
    lsrc = np.asarray(cm.lookup_src)
    explained = [set(c["cells"].tolist()) for c in got["found"] if c["direction"] == 0]
    honest_inst = honest[0][public]
    worst = 0
    for k, p in enumerate(rng.choice(D, size=min(N_SUFFIX, len(D)), replace=False).tolist()):
        S = D[D >= p]
        SL = DL[lsrc[DL] >= p] if len(DL) else DL
        dev.show(*hybrid(honest, other, (S, SL)))
        keep, lkeep = W[S].copy(), LK[SL].copy() if len(SL) else None
        try:
            W[S] = W2[S]
            if len(SL):
                LK[SL] = LK2[SL]
            claims = [None] + ([honest_inst] if k % 8 == 0 else [])
            for claimed in claims:
                inst = [W[c] for c in public] if claimed is None else to_ints(dev.O, claimed)
                want = AM.recount(cm, W, LK, L, public, inst, touched=(S, SL))
                rep = dev.report(claimed)
                assert rep == want, (name, p, len(S), rep, want)
                if claimed is None:
                    inside, cells = [e for e in explained if e <= set(S.tolist())], set(S.tolist())
                    a_union = bool(inside) and set().union(*inside) == cells
                    assert AM.violations(rep) >= 1 or a_union, (name, p, len(S), rep)
                    worst = max(worst, AM.violations(rep))
        finally:
            W[S] = keep
            if len(SL):
                LK[SL] = lkeep
    dev.show(*honest)
    print(f"{name}: {min(N_SUFFIX, len(D))} suffix splices, up to {worst} violations at once")


def dropped_tie(name, cm, dev, checker_for, n_in, honest, other, W, W2, LK, LK2, D, DL, altered, public, L):
    """the copy constraint that alone holds the largest part of D to the altered input, removed from a copy of the map: the sweep finds
    the part behind it as a cut without a reason, the device passes its hybrid under the weakened map and refuses it under the real one"""
    from halo2_vectordb_amd import circuit_sym as CS
    ties = SM.bridge_ties(cm, W, W2, LK, LK2, D, DL, altered)
    assert ties, f"{name}: no single copy constraint holds a part of the changed cells"
    size, cell = ties[0]
    weak = CS.CopyMap(np.array(cm.copy_of), cm.const_idx, cm.consts, cm.asserted, cm.gate, cm.lookup_src)
    weak.copy_of[cell] = cell
    _parts, found = SM.cuts(weak, W, W2, LK, LK2, range(n_in), public, L, D, DL)
    ends = (cell, int(cm.copy_of[cell]))                      # behind the tie: the copying cell, or its source
    mine = [c for c in found if c["direction"] == 0 and len(c["cells"]) + len(c["lookups"]) == size and any(e in c["cells"] for e in ends)]
    assert len(mine) == 1, (name, cell, size, [SM.describe(weak, c) for c in found][:4])
    cut = mine[0]
    assert SM.explain_cut(weak, W, cut) is None, (name, SM.describe(weak, cut))
    weak_chk = checker_for(weak)
    real = dev.chk
    try:
        piece = (cut["cells"], cut["lookups"])
        dev.show(*hybrid(honest, other, piece))
        dev.chk = weak_chk
        rep = dev.report()
        assert AM.violations(rep) == 0, (name, cell, rep)
        dev.chk = real
        rep = dev.report()
        want = SM.splice_report(cm, W, W2, LK, LK2, piece, public, L)
        assert AM.violations(rep) >= 1 and rep == want and rep["copies_unequal"] >= 1, (name, cell, rep, want)
    finally:
        dev.chk = real
        weak_chk.free()
        dev.show(*honest)
    print(f"{name}: without the copy of cell {int(cm.copy_of[cell])} into cell {cell}, {size} cells and lookup cells are written alone; the real map notices")


def test_kmeans(api, O):
    """a place of vector 0 and of vector 1: the first centroids, each a member of its own cluster"""
    from halo2_vectordb_amd.pipeline import KmeansHotPath
    hp = KmeansHotPath(n=8, dim=4, K=2, I=1, k=12, L=11, metric="cosine", tau=TAU).setup()
    device_splice(api, O, "k-means cosine n 8 dim 4 K 2 I 1", hp,
                  lambda r: [("a place of vector 0", 0, 1, r[0, 1] + 2.0 ** -7), ("a place of vector 1", 1, 0, r[1, 0] + 2.0 ** -7)])


def test_query(api, O):
    from halo2_vectordb_amd.pipeline import QueryHotPath
    hp = QueryHotPath(n=6, dim=4, k=12, L=11, metric="cosine", tau=TAU).setup()
    device_splice(api, O, "query cosine n 6 dim 4", hp, lambda r: [("a database place", 3, 1, r[3, 1] + 1.0), ("a query place", 0, 3, r[0, 3] + 2.0 ** -7)])


def test_topk_query(api, O):
    from halo2_vectordb_amd.pipeline import TopKQueryHotPath
    v = separated_inputs("euclidean", 2, 4, 3, 2, seed=21)
    hp = TopKQueryHotPath(q=2, n=4, dim=3, topk=2, k=12, L=11, metric="euclidean", tau=TAU, vectors=v).setup()
    device_splice(api, O, "top-k euclidean q 2 n 4 dim 3 t 2", hp,
                  lambda r: [("a database place, far", 3, 0, r[3, 0] + 2.5), ("a place of query 1", 1, 2, r[1, 2] + 2.0 ** -9)])


def test_batch_query(api, O):
    from halo2_vectordb_amd.pipeline import BatchQueryHotPath
    v = separated_inputs("euclidean", 2, 4, 3, 2, seed=21)
    hp = BatchQueryHotPath(q=2, n=4, dim=3, k=12, L=11, metric="euclidean", tau=TAU, vectors=v).setup()
    device_splice(api, O, "batch euclidean q 2 n 4 dim 3", hp,
                  lambda r: [("a database place, far", 5, 1, r[5, 1] + 2.5), ("a place of query 0", 0, 0, r[0, 0] + 2.0 ** -9)])


def test_merkle(api, O):
    from halo2_vectordb_amd.pipeline import MerkleHotPath
    hp = MerkleHotPath(n=6, dim=5, k=11, tau=TAU).setup()
    device_splice(api, O, "merkle n 6 dim 5", hp, lambda r: [("word 0 of leaf 0", 0, 0, r[0, 0] + 1.0), ("word 4 of leaf 5", 5, 4, r[5, 4] + 1.0)])


def test_merkle_update(api, O):
    """words of the last update's new vector: an earlier update's new leaf is a sibling or the old leaf of a later one here, and those
    are inputs of their own (they change the head of the stream in several cells)"""
    from test_gpu_merkle_update import _hot_path
    device_splice(api, O, "merkle update n 6 dim 4 m 4", _hot_path(6, 4, [4, 5, 6, 4], 21).setup(),
                  lambda r: [("word 2 of new vector 3", 3, 2, r[3, 2] + 1.0), ("word 0 of new vector 3", 3, 0, r[3, 0] + 1.0)])


def test_distances(api, O):
    """a's place 0 is moved onto b's, or off it where the example has them equal (the Hamming sum changes); b's last place moves a little"""
    from halo2_vectordb_amd.pipeline import DistancesHotPath
    d, cfg = E.load("distances"), E.README["distances"]
    v = np.array([d["a"], d["b"]], dtype=np.float64)
    hp = DistancesHotPath(dim=v.shape[1], k=cfg["k"], L=cfg["L"], tau=TAU, vectors=v).setup()
    assert hp.metrics.index("hamming") == len(hp.metrics) - 1                          # the last distance: its tail runs to the end
    last = v.shape[1] - 1
    device_splice(api, O, "distances example", hp,
                  lambda r: [("a[0] onto or off b[0]", 0, 0, r[1, 0] if r[1, 0] != r[0, 0] else r[0, 0] + 0.375), ("b's last place + 2^-10", 1, last, r[1, last] + 2.0 ** -10)],
                  [hp.n_cells])


def test_fixed_point(api, O):
    from halo2_vectordb_amd.pipeline import FixedPointHotPath
    hp = FixedPointHotPath(x=1.128, k=13, P=32, L=12, tau=TAU).setup()
    device_splice(api, O, "fixed-point example", hp, lambda r: [("x + 0.5", 0, 0, r[0, 0] + 0.5), ("x + 2^-10", 0, 0, r[0, 0] + 2.0 ** -10)])


def test_ann_query(api, O):
    """the query of the nearest cluster at (K 1, five members): a query place moved so far that another member wins (found on the f64
    rows, with a margin), and one moved a little"""
    from test_gpu_ann import DIM, _hot_path, _setup
    _n, _K, _ids, f, _db, _cent, _query = _setup(O, "5")
    near = lambda q: np.sort(((f["db"] - q) ** 2).sum(axis=1))
    first = int(np.argmin(((f["db"] - f["query"]) ** 2).sum(axis=1)))
    moves = [(j, v) for j in range(DIM) for v in np.arange(-400.0, 700.0, 25.0)
             if int(np.argmin(((f["db"] - np.where(np.arange(DIM) == j, v, f["query"])) ** 2).sum(axis=1))) != first
             and np.diff(near(np.where(np.arange(DIM) == j, v, f["query"]))[:2])[0] > 1.0]
    assert moves
    j, v = moves[0]
    index, hp = _hot_path(O, "5")
    try:
        device_splice(api, O, f"ann euclidean 5 dim {DIM}", hp.setup(),
                      lambda r: [(f"query place {j}: another member wins", 0, j, v), ("a query place", 0, (j + 1) % DIM, r[0, (j + 1) % DIM] + 2.0 ** -9)])
    finally:
        index.free()
