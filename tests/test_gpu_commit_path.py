"""The entry points every proof step commits through (HotPath.step: the commit() and ntt() closures), called the way pipeline.py calls
them — ctypes on the library with api.DeviceBuffer — and held bit exact to the oracle on columns materialised by the plain model
(tests/commit_path_model.py): column descriptors built by the library and written by hand, the MSM that reads through them with a skip
mask and per-column constant points, its batch loop (more than one batch only under vdb_msm_set_scratch_cap), the deferred begin / end
contract, the entry statistic of the shard balancing, the first transform pass that reads through the same descriptors, and the keygen
side mask kernels.  No tolerances anywhere."""
import os
import subprocess
import sys

import numpy as np
import pytest

import commit_path_model as CM
from test_gpu_msm import witness_like

pytestmark = pytest.mark.gpu

R = CM.R
ERR_ARG = -3
FR = 32                         # bytes of a field element
K = 11                          # the MSM tests' SRS: the smallest with the default 11-bit window and two 1,024-thread strides of rows
ROWS = 1 << K
MIX = 8192                      # cells of the scalar mix at the head of the synthetic stream; then ROWS cells of r - 1, then ROWS zeros
DESC = np.dtype([("src", "<u8"), ("len", "<u8"), ("blind", "<u8")])       # vdb_colsrc: 24 bytes


def scalar_mix(O, rng, n, windows):
    """witness-like scalars on the even lanes, the edges of the recoding (for every window size in `windows`) on the odd ones: short and
    long scalars share every wavefront of the source fetch"""
    v = witness_like(O, rng, n)
    edges = sorted({e for c in windows for e in CM.edge_scalars(c)})
    order = rng.permutation(len(edges))
    v[1::2] = O.fr_from_ints([edges[int(order[i % len(edges)])] for i in range(len(range(1, n, 2)))])
    return v


def fast_fr(rng, n):
    """n valid Montgomery words without a Python loop (any value below r is the Montgomery form of some element)"""
    a = rng.integers(0, 1 << 64, size=(n, 4), dtype=np.uint64)
    a[:, 3] %= np.uint64(R >> 192)          # top word below r's top word
    return a


def ptr(buf):
    return None if buf is None else buf.ptr


def records(d_stream, specs, d_blind, n_blind):
    """hand-written descriptors: specs = [(start cell, len, row of d_blind or None)]"""
    rec = np.zeros(len(specs), dtype=DESC)
    for i, (start, length, b) in enumerate(specs):
        rec[i] = (d_stream.ptr.value + start * FR, length, 0 if b is None else d_blind.ptr.value + b * n_blind * FR)
    return rec


# ------------------------------------------------------------------ G1 on the host: the oracle's Python addition
def pt_int(O, p):
    x, y = O.fq_to_ints(np.asarray(p, dtype=np.uint64).reshape(2, 4))
    return None if x == 0 and y == 0 else (x, y)


def pt_arr(O, p):
    return np.zeros(8, dtype=np.uint64) if p is None else O.fq_from_ints(list(p)).reshape(8)


def pt_add(O, PY, a, b):
    return pt_arr(O, PY.g1_add(pt_int(O, a), pt_int(O, b)))


def pt_neg(O, PY, a):
    p = pt_int(O, a)
    return pt_arr(O, None if p is None else (p[0], (-p[1]) % PY.Q))


# ------------------------------------------------------------------ fixtures
class Env:
    pass


class Pool:
    """device buffers of one test, freed when it ends"""

    def __init__(self, api):
        self.api, self.bufs = api, []

    def alloc(self, nbytes):
        b = self.api.DeviceBuffer(max(int(nbytes), 64))
        self.bufs.append(b)
        return b

    def new(self, arr):
        arr = np.ascontiguousarray(arr)
        b = self.alloc(arr.nbytes)
        if arr.nbytes:
            b.upload(arr)
        return b

    def free(self):
        self.api.init().vdb_msm_batch_end(None, 0)        # a test that failed between _begin and _end leaves nothing open
        self.api.sync()
        for b in self.bufs:
            b.free()
        self.bufs = []


@pytest.fixture(scope="module")
def env(O, PY):
    from halo2_vectordb_amd import api
    e = Env()
    e.api, e.lib, e.O, e.PY = api, api.init(), O, PY
    e.g, e.gl = O.srs_from_tau(K, 0xC0117A7)
    e.srs = {11: api.Srs(K, e.g, e.gl), 13: api.Srs(K, e.g, e.gl, window_bits=13)}
    assert e.srs[11].info()[1] == 11 and e.srs[13].info()[1] == 13
    rng = np.random.default_rng(20261018)
    e.stream = np.concatenate([scalar_mix(O, rng, MIX, (11, 13)), np.tile(O.fr_from_ints([R - 1]), (ROWS, 1)), np.zeros((ROWS, 4), dtype=np.uint64)])
    e.pool = Pool(api)
    e.d_stream = e.pool.new(e.stream)
    yield e
    e.pool.free()
    for s in e.srs.values():
        s.free()


@pytest.fixture
def pool(env):
    p = Pool(env.api)
    yield p
    p.free()


def msm_end(env, n_cols):
    out = np.zeros((n_cols, 8), dtype=np.uint64)
    env.api.check(env.lib.vdb_msm_batch_end(env.api._p(out), n_cols))
    return out


def msm_src(env, srs, basis, d_src, n_cols, n, n_blind, d_mask=None, d_pts=None):
    env.api.check(env.lib.vdb_msm_batch_src_dev_begin(srs.h, basis, d_src.ptr, n_cols, n, n_blind, ptr(d_mask), ptr(d_pts)))
    return msm_end(env, n_cols)


def msm_deferred(env, srs, basis, d_cols, n_cols, n, d_mask=None, d_pts=None):
    env.api.check(env.lib.vdb_msm_batch_masked_dev_begin(srs.h, basis, d_cols.ptr, n_cols, n, ptr(d_mask), ptr(d_pts)))
    return msm_end(env, n_cols)


def msm_masked(env, srs, basis, d_cols, n_cols, n, d_mask, d_pts):
    out = np.zeros((n_cols, 8), dtype=np.uint64)
    env.api.check(env.lib.vdb_msm_batch_masked_dev(srs.h, basis, d_cols.ptr, n_cols, n, d_mask.ptr, d_pts.ptr, env.api._p(out)))
    return out


def msm_plain(env, srs, basis, d_cols, n_cols, n):
    out = np.zeros((n_cols, 8), dtype=np.uint64)
    env.api.check(env.lib.vdb_msm_batch_dev(srs.h, basis, d_cols.ptr, n_cols, n, env.api._p(out)))
    return out


def edge_lens(n, n_blind):
    return [0, 1, 63, 64, 65, 1024, 1025, n - n_blind - 1, n - n_blind]


def blinds(O, rng, n_cols, n_blind):
    """(n_cols, n_blind, 4) random blinding scalars with r - 1 and zero among them"""
    b = O.random_fr(rng, n_cols * max(n_blind, 1)).reshape(n_cols, max(n_blind, 1), 4)[:, :n_blind].copy()
    if n_blind and n_cols > 3:
        b[2, 0] = O.fr_from_ints([R - 1])[0]
        b[3, n_blind - 1] = 0
    return b


# ------------------------------------------------------------------ a. the MSM through column sources
@pytest.mark.parametrize("ragged", [0, 37])
@pytest.mark.parametrize("window_bits", [11, 13])
def test_src_msm_hand_written_descriptors(env, pool, window_bits, ragged):
    """descriptors uploaded by the test: every edge length, two columns that overlap in the stream, an all-(r - 1) and an all-zero
    column, blind pointers null on some columns, n_blind 0 / 1 / 6, columns as long as the SRS and 37 rows shorter, both bases, the
    11-bit window (short / long records and queue) and the 13-bit one (dense walk, two-phase scatter): the oracle's MSM of the
    materialised columns"""
    O, srs, n = env.O, env.srs[window_bits], ROWS - ragged
    rng = np.random.default_rng(100 * window_bits + ragged)
    for n_blind in (0, 1, 6):
        lens = edge_lens(n, n_blind) + [n - n_blind, n - n_blind]
        starts = [7, 0, 3, 40, 41, 100, 1100, 2000, 1, MIX, MIX + ROWS]           # [40, 104) and [41, 106) overlap
        assert all(s + ln <= (MIX if s < MIX else len(env.stream)) for s, ln in zip(starts, lens))
        n_cols = len(lens)
        blind = blinds(O, rng, n_cols, n_blind)
        with_blind = [c % 3 != 1 for c in range(n_cols)]
        d_blind = pool.new(blind)
        d_src = pool.new(records(env.d_stream, [(s, ln, c if with_blind[c] else None) for c, (s, ln) in enumerate(zip(starts, lens))], d_blind, n_blind))
        cols = np.stack([CM.materialise(env.stream, s, ln, blind[c] if with_blind[c] else None, n, n_blind) for c, (s, ln) in enumerate(zip(starts, lens))])
        for basis, bases in ((1, env.gl), (0, env.g)):
            got = msm_src(env, srs, basis, d_src, n_cols, n, n_blind)
            want = O.msm_batch(cols, bases[:n], threads=8)
            assert np.array_equal(got, want), (window_bits, n, n_blind, basis, np.flatnonzero((got != want).any(axis=1)))
            assert not got[10].any() and (n_blind or not got[0].any())        # the all-zero column, the empty one: identity (0, 0)


@pytest.mark.parametrize("window_bits", [11, 13])
def test_src_msm_built_descriptors_against_the_copied_layout(env, pool, window_bits):
    """descriptors from vdb_colsrc_build_dev, break points that give the edge lengths (but 0: the cell on a break row opens the next column,
    so no column is empty) and a short last column: the MSM through them,
    vdb_layout_columns_dev + vdb_msm_batch_dev on the same stream and the oracle on the model's columns agree, and the copied columns
    are the model's"""
    O, api, lib, srs, n = env.O, env.api, env.lib, env.srs[window_bits], ROWS
    rng = np.random.default_rng(200 + window_bits)
    for n_blind, given in ((0, False), (1, True), (6, True), (6, False)):
        bp = np.array([ln - 1 for ln in edge_lens(n, n_blind)[1:]], dtype=np.uint64)
        n_cells, n_cols = int(bp.sum()) + 37, len(bp) + 1
        assert n_cells <= MIX
        blind = blinds(O, rng, n_cols, n_blind) if given else None
        d_blind = pool.new(blind) if given else None
        d_src = pool.alloc(n_cols * 24)
        api.check(lib.vdb_colsrc_build_dev(env.d_stream.ptr, n_cells, api._p(bp), len(bp), K, 0, n_cols, ptr(d_blind), n_blind, d_src.ptr))
        d_cols = pool.alloc(n_cols * n * FR)
        api.check(lib.vdb_layout_columns_dev(env.d_stream.ptr, n_cells, api._p(bp), len(bp), K, d_cols.ptr, ptr(d_blind), n_blind))
        desc = CM.descriptors(n_cells, bp, K, 0, n_cols)
        assert [ln for _, ln in desc] == edge_lens(n, n_blind)[1:] + [37]
        cols = np.stack([CM.materialise(env.stream, s, ln, blind[c] if given else None, n, n_blind) for c, (s, ln) in enumerate(desc)])
        assert np.array_equal(d_cols.download((n_cols, n, 4)), cols)
        for basis, bases in ((1, env.gl), (0, env.g)):
            want = O.msm_batch(cols, bases, threads=8)
            assert np.array_equal(msm_src(env, srs, basis, d_src, n_cols, n, n_blind), want), (window_bits, n_blind, given, basis)
            assert np.array_equal(msm_plain(env, srs, basis, d_cols, n_cols, n), want), (window_bits, n_blind, given, basis)


# ------------------------------------------------------------------ b. the descriptor builders
def built(env, d_out, n_max, call):
    """runs a builder on a pattern-filled buffer of n_max records; returns (rc, records)"""
    d_out.upload(np.full(n_max * 24, 0xAB, dtype=np.uint8))
    rc = call(d_out.ptr)
    return rc, d_out.download((n_max,), dtype=DESC)


def untouched(rec):
    return bool((rec.view(np.uint8) == 0xAB).all())


def test_descriptor_builders_every_sub_range(env, pool):
    """random break points (one column exactly as long as the blinding rows allow) and three stream tails, lookup streams shorter than a
    column, ending on a column boundary and ragged: every [col_lo, col_hi), the records as offsets from the stream base, len, and the
    blind pointer by absolute column; refused arguments write nothing"""
    api, lib = env.api, env.lib
    k, n_blind, min_rows = 6, 3, 9
    rows = 1 << k
    rng = np.random.default_rng(61)
    base = env.d_stream.ptr.value
    d_blind = pool.alloc(8 * n_blind * FR)
    d_out = pool.alloc(8 * 24)
    bp = rng.integers(1, rows - n_blind - 1, size=5).astype(np.uint64)
    bp[3] = rows - n_blind - 1                                                # len + n_blind == rows: still accepted
    n_cols = len(bp) + 1
    for tail in (1, 17, rows - n_blind):
        n_cells = int(bp.sum()) + tail
        for d_b in (d_blind, None):
            for lo in range(n_cols + 1):
                for hi in range(lo, n_cols + 1):
                    rc, rec = built(env, d_out, 8, lambda out: lib.vdb_colsrc_build_dev(env.d_stream.ptr, n_cells, api._p(bp), len(bp), k, lo, hi, ptr(d_b), n_blind, out))
                    assert rc == 0, (tail, lo, hi)
                    want = CM.descriptors(n_cells, bp, k, lo, hi)
                    assert [(int(r["src"]) - base, int(r["len"])) for r in rec[: hi - lo]] == [(s * FR, ln) for s, ln in want], (tail, lo, hi)
                    assert [int(r["blind"]) for r in rec[: hi - lo]] == [d_b.ptr.value + c * n_blind * FR if d_b else 0 for c in range(lo, hi)]
                    assert untouched(rec[hi - lo:])
    n_cells = int(bp.sum()) + 17
    build = lambda out, cells=n_cells, b=bp, hi=n_cols: lib.vdb_colsrc_build_dev(env.d_stream.ptr, cells, api._p(b), len(b), k, 0, hi, d_blind.ptr, n_blind, out)
    bad_bp = bp.copy()
    bad_bp[2] = rows
    for what, call in (("col_hi > n_bp + 1", lambda out: build(out, hi=n_cols + 1)),
                       ("a break point >= rows", lambda out: build(out, b=bad_bp)),
                       ("the stream is shorter than the break points' sum", lambda out: build(out, cells=int(bp.sum()) - 1)),
                       ("no cell on the last break row", lambda out: build(out, cells=int(bp.sum()))),
                       ("a column overruns the stream", lambda out: build(out, cells=int(bp[:3].sum()), hi=3))):
        rc, rec = built(env, d_out, 8, call)
        assert rc == ERR_ARG and untouched(rec), what
    # lookup columns of rows - min_rows = 55 cells
    per = rows - min_rows
    for n_cells in (30, 2 * per, 2 * per + 27):
        for d_b in (d_blind, None):
            for lo in range(5):
                for hi in range(lo, 5):
                    rc, rec = built(env, d_out, 8, lambda out: lib.vdb_colsrc_build_lookup_dev(env.d_stream.ptr, n_cells, k, min_rows, lo, hi, ptr(d_b), n_blind, out))
                    assert rc == 0, (n_cells, lo, hi)
                    want = CM.descriptors_lookup(n_cells, k, min_rows, lo, hi)
                    assert [(int(r["src"]) - base, int(r["len"])) for r in rec[: hi - lo]] == [(s * FR, ln) for s, ln in want], (n_cells, lo, hi)
                    assert [int(r["blind"]) for r in rec[: hi - lo]] == [d_b.ptr.value + c * n_blind * FR if d_b else 0 for c in range(lo, hi)]
                    assert untouched(rec[hi - lo:])
    rc, rec = built(env, d_out, 8, lambda out: lib.vdb_colsrc_build_lookup_dev(env.d_stream.ptr, 30, k, rows, 0, 1, d_blind.ptr, n_blind, out))
    assert rc == ERR_ARG and untouched(rec)


# ------------------------------------------------------------------ c. cells and blinding rows do not overlap
def test_cells_do_not_reach_into_the_blinding_rows(env, pool):
    """The pinned behaviour (include/vdb.h, vdb_colsrc): both readers — colsrc_fetch and the copying layout — take a row below len from
    the stream before they look at the blinding rows, so for len in n - n_blind + 1 .. n they agree with each other (the cell wins), but
    not with "the last n_blind rows come from blind".  The builders therefore refuse such a column when blinds are given (the pipeline's
    break points leave MINIMUM_ROWS = 9 >= N_BLIND = 7 rows free and never produce one) and accept it without blinds."""
    from halo2_vectordb_amd.protocol import MINIMUM_ROWS, N_BLIND
    assert MINIMUM_ROWS >= N_BLIND
    O, api, lib, srs, n, n_blind = env.O, env.api, env.lib, env.srs[11], ROWS, 6
    rng = np.random.default_rng(31)
    blind = blinds(O, rng, 2, n_blind)
    d_blind = pool.new(blind)
    d_out = pool.alloc(2 * 24)
    base = env.d_stream.ptr.value
    over = list(range(n - n_blind + 1, n + 1))
    for ln in [n - n_blind] + over:
        bp = np.array([ln - 1], dtype=np.uint64)
        build = lambda out, b: lib.vdb_colsrc_build_dev(env.d_stream.ptr, ln + 3, api._p(bp), 1, K, 0, 2, b, n_blind, out)
        rc, rec = built(env, d_out, 2, lambda out: build(out, d_blind.ptr))
        if ln in over:
            assert rc == ERR_ARG and untouched(rec), ln
            rc, rec = built(env, d_out, 2, lambda out: lib.vdb_colsrc_build_dev(env.d_stream.ptr, ln + 3, api._p(bp), 1, K, 1, 2, d_blind.ptr, n_blind, out))
            assert rc == 0 and int(rec[0]["len"]) == 4, ln                    # the range built does not hold the long column
        else:
            assert rc == 0 and [int(r["len"]) for r in rec] == [ln, 4]
        rc, rec = built(env, d_out, 2, lambda out: build(out, None))
        assert rc == 0 and [(int(r["src"]) - base, int(r["len"]), int(r["blind"])) for r in rec] == [(0, ln, 0), ((ln - 1) * FR, 4, 0)], ln
    # lookup columns: minimum_rows below n_blind lets a full column reach into the blinding rows
    for min_rows, cells, ok in ((3, n, False), (3, n - n_blind, True), (n_blind, n, True), (0, n, False)):
        rc, rec = built(env, d_out, 2, lambda out: lib.vdb_colsrc_build_lookup_dev(env.d_stream.ptr, cells, K, min_rows, 0, 1, d_blind.ptr, n_blind, out))
        assert (rc == 0 and not untouched(rec)) if ok else (rc == ERR_ARG and untouched(rec)), (min_rows, cells)
        rc, rec = built(env, d_out, 2, lambda out: lib.vdb_colsrc_build_lookup_dev(env.d_stream.ptr, cells, K, min_rows, 0, 1, None, n_blind, out))
        assert rc == 0 and int(rec[0]["len"]) == min(cells, n - min_rows)
    # the two readers on hand-written descriptors of these lengths: the same column, the stream cell on every row below len
    start = 11
    d_src = pool.new(records(env.d_stream, [(start, ln, 0) for ln in over], d_blind, n_blind))
    d_cols = pool.alloc(len(over) * n * FR)
    cols = []
    for i, ln in enumerate(over):
        bp = np.array([ln - 1], dtype=np.uint64)
        api.check(lib.vdb_layout_columns_range_dev(env.d_stream.at(start * FR), ln + 3, api._p(bp), 1, K, 0, 1, d_cols.at(i * n * FR), d_blind.ptr, n_blind))
        col = CM.materialise(env.stream, start, 0, blind[0], n, n_blind)
        col[:ln] = env.stream[start:start + ln]
        cols.append(col)
    cols = np.stack(cols)
    assert np.array_equal(d_cols.download((len(over), n, 4)), cols)
    want = O.msm_batch(cols, env.gl, threads=8)
    assert np.array_equal(msm_src(env, srs, 1, d_src, len(over), n, n_blind), want)
    assert np.array_equal(msm_plain(env, srs, 1, d_cols, len(over), n), want)


# ------------------------------------------------------------------ d, e, f: mask, constant points, batches, the deferred contract
def differing_columns(env, pool, rng, n, n_blind, n_cols):
    """n_cols columns that all differ, as descriptors into the stream (blind null on every fourth), materialised on the host and
    uploaded"""
    lens = [n - n_blind, 1025, 64, n - n_blind - 1, 1500, 65, 1024]
    specs = [(13 + 211 * c, lens[c % 7], None if c % 4 == 3 else c) for c in range(n_cols)]
    blind = blinds(env.O, rng, n_cols, n_blind)
    d_blind = pool.new(blind)
    c = Env()
    c.n, c.n_blind, c.n_cols = n, n_blind, n_cols
    c.cols = np.stack([CM.materialise(env.stream, s, ln, None if b is None else blind[b], n, n_blind) for s, ln, b in specs])
    assert len({col.tobytes() for col in c.cols}) == n_cols
    c.d_src = pool.new(records(env.d_stream, specs, d_blind, n_blind))
    c.d_cols = pool.new(c.cols)
    return c


def masked_sum(O, cols, mask, bases):
    kept = cols.copy()
    kept[mask.astype(bool)] = 0
    return O.msm_batch(kept, bases, threads=8)


def test_mask_and_constant_points(env, pool):
    """six mask patterns (nothing, everything, random, every 64th row, exactly the zero cells, the blinding rows) times four constant
    points (identity, a random point, minus the unmasked sum, the unmasked sum itself), all per-column points different, through the
    three masked entry points: the oracle's MSM with the masked cells zeroed plus the point, by the oracle's group addition"""
    O, PY, srs, n, n_blind, n_cols = env.O, env.PY, env.srs[11], ROWS, 6, 6
    rng = np.random.default_rng(41)
    C = differing_columns(env, pool, rng, n, n_blind, n_cols)
    mask = np.zeros((n_cols, n), dtype=np.uint8)
    mask[1] = 1
    mask[2] = rng.integers(0, 2, size=n)
    mask[3, ::64] = 1
    mask[4] = ~C.cols[4].any(axis=1)
    mask[5, n - n_blind:] = 1
    assert mask[4].any() and not mask[4].all() and C.cols[5, n - n_blind:].any()
    d_mask = pool.new(mask)
    S = {1: masked_sum(O, C.cols, mask, env.gl), 0: masked_sum(O, C.cols, mask, env.g)}
    assert not S[1][1].any() and not S[0][1].any()                            # everything masked
    rand = O.g1_mul_generator([int(v) for v in rng.integers(2, 1 << 62, size=n_cols)])
    for shift in range(6):                                                       # every column meets every kind of point
        basis = 1 - shift % 2
        kinds = [(0, 1, 2, 3, 1, 3)[(c + shift) % 6] for c in range(n_cols)]
        pts = np.stack([(np.zeros(8, dtype=np.uint64), rand[c], pt_neg(O, PY, S[basis][c]), S[basis][c])[kinds[c]] for c in range(n_cols)])
        distinct = [p.tobytes() for p in pts if p.any()]                         # (the identity: kind 0, and -0 = 0 of the fully masked column)
        assert len(set(distinct)) == len(distinct) >= 4
        want = np.stack([pt_add(O, PY, S[basis][c], pts[c]) for c in range(n_cols)])
        for c in range(n_cols):
            if kinds[c] == 2:
                assert not want[c].any()                                          # P + (-P): the identity, (0, 0)
            if kinds[c] == 3 and c != 1:
                assert want[c].any() and not np.array_equal(want[c], pts[c])      # a doubling
        assert np.array_equal(want[1], pts[1])                                    # a fully masked column gives its point
        d_pts = pool.new(pts)
        assert np.array_equal(msm_masked(env, srs, basis, C.d_cols, n_cols, n, d_mask, d_pts), want), (shift, "masked_dev")
        assert np.array_equal(msm_deferred(env, srs, basis, C.d_cols, n_cols, n, d_mask, d_pts), want), (shift, "masked_dev_begin")
        assert np.array_equal(msm_src(env, srs, basis, C.d_src, n_cols, n, n_blind, d_mask, d_pts), want), (shift, "src_dev_begin")


def test_constant_factoring_identity_and_refused_pairs(env, pool):
    """production's identity: with the constant point the MSM of exactly the masked cells (vdb_mask_select_dev(keep_const = 1) +
    vdb_msm_batch_dev, as keygen does), the masked MSM is the plain MSM of the column.  A mask without points, or points without a
    mask, is refused and leaves nothing open."""
    O, api, lib, srs, n, n_blind, n_cols = env.O, env.api, env.lib, env.srs[11], ROWS - 37, 6, 5
    rng = np.random.default_rng(42)
    C = differing_columns(env, pool, rng, n, n_blind, n_cols)
    mask = (rng.random((n_cols, n)) < 0.4).astype(np.uint8)
    mask[3] = 0
    d_mask = pool.new(mask)
    d_const = pool.alloc(n_cols * n * FR)
    api.check(lib.vdb_mask_select_dev(C.d_cols.ptr, d_mask.ptr, n_cols * n, 1, d_const.ptr))
    pts = msm_plain(env, srs, 1, d_const, n_cols, n)
    const = C.cols.copy()
    const[~mask.astype(bool)] = 0
    assert np.array_equal(pts, O.msm_batch(const, env.gl[:n], threads=8)) and not pts[3].any()
    d_pts = pool.new(pts)
    want = O.msm_batch(C.cols, env.gl[:n], threads=8)
    assert np.array_equal(msm_plain(env, srs, 1, C.d_cols, n_cols, n), want)
    assert np.array_equal(msm_masked(env, srs, 1, C.d_cols, n_cols, n, d_mask, d_pts), want)
    assert np.array_equal(msm_deferred(env, srs, 1, C.d_cols, n_cols, n, d_mask, d_pts), want)
    assert np.array_equal(msm_src(env, srs, 1, C.d_src, n_cols, n, n_blind, d_mask, d_pts), want)
    out = np.zeros((n_cols, 8), dtype=np.uint64)
    for m, p in ((d_mask.ptr, None), (None, d_pts.ptr)):
        assert lib.vdb_msm_batch_masked_dev_begin(srs.h, 1, C.d_cols.ptr, n_cols, n, m, p) == ERR_ARG
        assert lib.vdb_msm_batch_src_dev_begin(srs.h, 1, C.d_src.ptr, n_cols, n, n_blind, m, p) == ERR_ARG
        assert lib.vdb_msm_batch_masked_dev(srs.h, 1, C.d_cols.ptr, n_cols, n, m, p, api._p(out)) == ERR_ARG
    assert np.array_equal(msm_deferred(env, srs, 1, C.d_cols, n_cols, n), want)   # nothing was left open; mask and points both null


def one_column_batches(env):
    """with the work space released the MSM's budget is the cap: one byte, one column per batch"""
    env.api.check(env.lib.vdb_scratch_release())
    env.api.check(env.lib.vdb_msm_set_scratch_cap(1))


def default_batches(env):
    env.lib.vdb_msm_batch_end(None, 0)
    env.api.check(env.lib.vdb_msm_set_scratch_cap(0))
    env.api.check(env.lib.vdb_scratch_release())


def profiled(env, run):
    """(result, per-kernel launch counts) of run() in the profiling mode that keeps the deferred tail"""
    env.api.profile_begin(deferred=True)
    try:
        got = run()
    finally:
        prof = env.api.profile_end()
    return got, {k: v["launches"] for k, v in prof.items()}


def test_seven_batches_of_one_column(env, pool):
    """the batch loop of msm_batch_dev: seven columns that all differ — scalars, descriptors, masks, constant points — in seven batches,
    all four entry points; scalars, sources, mask, points and outputs each advance per batch, and only the last batch's tail is deferred.
    The launch count proves that seven batches ran."""
    O, PY, srs, n, n_blind, n_cols = env.O, env.PY, env.srs[11], ROWS - 37, 6, 7
    rng = np.random.default_rng(51)
    C = differing_columns(env, pool, rng, n, n_blind, n_cols)
    mask = (rng.random((n_cols, n)) < 0.3).astype(np.uint8)
    assert len({m.tobytes() for m in mask}) == n_cols
    pts = O.g1_mul_generator([int(v) for v in rng.integers(2, 1 << 62, size=n_cols)])
    assert len({p.tobytes() for p in pts}) == n_cols
    d_mask, d_pts = pool.new(mask), pool.new(pts)
    plain = {1: O.msm_batch(C.cols, env.gl[:n], threads=8), 0: O.msm_batch(C.cols, env.g[:n], threads=8)}
    assert len({p.tobytes() for p in plain[1]}) == n_cols
    masked = {b: np.stack([pt_add(O, PY, s, p) for s, p in zip(masked_sum(O, C.cols, mask, bases[:n]), pts)]) for b, bases in ((1, env.gl), (0, env.g))}
    entries = [("msm_batch_dev", lambda: msm_plain(env, srs, 1, C.d_cols, n_cols, n), plain[1]),
               ("msm_batch_masked_dev", lambda: msm_masked(env, srs, 1, C.d_cols, n_cols, n, d_mask, d_pts), masked[1]),
               ("msm_batch_masked_dev_begin", lambda: msm_deferred(env, srs, 0, C.d_cols, n_cols, n, d_mask, d_pts), masked[0]),
               ("msm_batch_src_dev_begin", lambda: msm_src(env, srs, 1, C.d_src, n_cols, n, n_blind, d_mask, d_pts), masked[1]),
               ("msm_batch_src_dev_begin, no mask", lambda: msm_src(env, srs, 0, C.d_src, n_cols, n, n_blind), plain[0])]
    try:
        for name, run, want in entries:
            one_column_batches(env)
            got, launches = profiled(env, run)
            assert launches.get("k_msm_sort") == n_cols and launches.get("k_msm_reduce") == n_cols, (name, launches)
            assert np.array_equal(got, want), (name, np.flatnonzero((got != want).any(axis=1)))
    finally:
        default_batches(env)
    got, launches = profiled(env, entries[3][1])                                  # and the default policy: one batch again
    assert launches.get("k_msm_sort") == 1 and np.array_equal(got, entries[3][2])


@pytest.mark.parametrize("overwrite", ["lagrange_to_coeff", "memset"])
@pytest.mark.parametrize("batches", [1, 7])
def test_scalars_may_be_overwritten_after_begin(env, pool, batches, overwrite):
    """include/vdb.h: once _begin has returned the scalars are no longer read.  The buffer is transformed in place (what the prover
    queues next) or filled with 0xff on the library's stream before _end: the commitments are those of the original scalars, with one
    batch and with seven"""
    O, PY, api, lib, srs, n, n_blind, n_cols = env.O, env.PY, env.api, env.lib, env.srs[11], ROWS, 6, 7
    rng = np.random.default_rng(60 + batches)
    C = differing_columns(env, pool, rng, n, n_blind, n_cols)
    mask = (rng.random((n_cols, n)) < 0.3).astype(np.uint8)
    pts = O.g1_mul_generator([int(v) for v in rng.integers(2, 1 << 62, size=n_cols)])
    d_mask, d_pts = pool.new(mask), pool.new(pts)
    want = np.stack([pt_add(O, PY, s, p) for s, p in zip(masked_sum(O, C.cols, mask, env.gl), pts)])

    def run():
        api.check(lib.vdb_msm_batch_masked_dev_begin(srs.h, 1, C.d_cols.ptr, n_cols, n, d_mask.ptr, d_pts.ptr))
        if overwrite == "memset":
            api.check(lib.vdb_memset_dev(C.d_cols.ptr, 0xFF, n_cols * n * FR))
        else:
            api.check(lib.vdb_lagrange_to_coeff_dev(C.d_cols.ptr, n_cols, K))
        return msm_end(env, n_cols)
    try:
        if batches > 1:
            one_column_batches(env)
        got, launches = profiled(env, run)
        assert launches.get("k_msm_sort") == batches, launches
        assert np.array_equal(got, want), np.flatnonzero((got != want).any(axis=1))
        after = C.d_cols.download((n_cols, n, 4))
        if overwrite == "memset":
            assert (after == np.uint64(0xFFFFFFFFFFFFFFFF)).all()
        else:
            assert np.array_equal(after, O.lde_batch(C.cols, ext=0, threads=8)[0])
    finally:
        default_batches(env)


def test_one_deferred_msm_at_a_time(env, pool):
    """while a batch is open a second _begin (a wider one, which would need a larger output buffer), the column-source _begin and the
    blocking MSMs return VDB_ERR_ARG and the open batch is still collected correctly; _end(NULL, 0) drops an open batch and the next
    MSM works"""
    O, PY, api, lib, srs, n, n_blind, n_cols = env.O, env.PY, env.api, env.lib, env.srs[11], ROWS, 6, 7
    rng = np.random.default_rng(70)
    C = differing_columns(env, pool, rng, n, n_blind, n_cols)
    mask = (rng.random((n_cols, n)) < 0.3).astype(np.uint8)
    pts = O.g1_mul_generator([int(v) for v in rng.integers(2, 1 << 62, size=n_cols)])
    d_mask, d_pts = pool.new(mask), pool.new(pts)
    want = np.stack([pt_add(O, PY, s, p) for s, p in zip(masked_sum(O, C.cols, mask, env.gl), pts)])
    plain = O.msm_batch(C.cols, env.gl, threads=8)
    wide = 64
    d_wide = pool.new(np.zeros((wide, n, 4), dtype=np.uint64))
    out = np.zeros((wide, 8), dtype=np.uint64)
    api.check(lib.vdb_msm_batch_masked_dev_begin(srs.h, 1, C.d_cols.ptr, n_cols, n, d_mask.ptr, d_pts.ptr))
    assert lib.vdb_msm_batch_masked_dev_begin(srs.h, 1, d_wide.ptr, wide, n, None, None) == ERR_ARG
    assert b"not been collected" in lib.vdb_last_error()
    assert lib.vdb_msm_batch_src_dev_begin(srs.h, 1, C.d_src.ptr, n_cols, n, n_blind, None, None) == ERR_ARG
    assert lib.vdb_msm_batch_dev(srs.h, 1, C.d_cols.ptr, n_cols, n, api._p(out)) == ERR_ARG
    assert lib.vdb_msm_batch_masked_dev(srs.h, 1, C.d_cols.ptr, n_cols, n, d_mask.ptr, d_pts.ptr, api._p(out)) == ERR_ARG
    assert not out.any()
    assert np.array_equal(msm_end(env, n_cols), want)
    # dropped without being collected
    api.check(lib.vdb_msm_batch_masked_dev_begin(srs.h, 1, C.d_cols.ptr, n_cols, n, d_mask.ptr, d_pts.ptr))
    assert lib.vdb_msm_batch_end(None, 0) == 0
    assert np.array_equal(msm_plain(env, srs, 1, C.d_cols, n_cols, n), plain)
    assert np.array_equal(msm_src(env, srs, 1, C.d_src, n_cols, n, n_blind, d_mask, d_pts), want)
    assert lib.vdb_msm_batch_end(None, 0) == 0                                    # nothing open: still fine


# ------------------------------------------------------------------ g. the entry statistic of the shard balancing
@pytest.mark.parametrize("c", [2, 8, 11, 14])
def test_count_entries(env, pool, c):
    """vdb_msm_count_entries_dev against the model's count of non-zero signed digits: the scalar mix with the edges of this window size,
    an all-zero and an all-(r - 1) column, full and ragged length, with and without a mask"""
    O, api, lib = env.O, env.api, env.lib
    k = 10
    srs = api.Srs(k, env.g[: 1 << k], None, window_bits=c)
    try:
        assert srs.info()[1:] == (c, CM.windows(c))
        W = CM.windows(c)
        rng = np.random.default_rng(80 + c)
        for n in (1 << k, (1 << k) - 37):
            cols = np.stack([scalar_mix(O, rng, n, (c,)), np.zeros((n, 4), dtype=np.uint64), np.tile(O.fr_from_ints([R - 1]), (n, 1))])
            ints = [O.fr_to_ints(col) for col in cols]
            mask = (rng.random((3, n)) < 0.5).astype(np.uint8)
            mask[0, cols[0].any(axis=1).argmax()] = 1                              # at least one non-zero cell is masked
            d_cols, d_mask = pool.new(cols), pool.new(mask)
            for m, d_m in ((None, None), (mask, d_mask)):
                got = np.zeros(3, dtype=np.uint64)
                api.check(lib.vdb_msm_count_entries_dev(srs.h, d_cols.ptr, 3, n, ptr(d_m), api._p(got)))
                want = [CM.count_entries(ints[i], None if m is None else m[i], c, W) for i in range(3)]
                assert [int(v) for v in got] == want, (c, n, m is not None)
                assert want[1] == 0 and want[2] == (n if m is None else int((m[2] == 0).sum())) and want[0] > 0
    finally:
        srs.free()


# ------------------------------------------------------------------ h. the transform that reads through the descriptors
NTT_CASES = {        # k: (n_blind, [(len as a function of n and n_blind, blind given)]); "r-1": the all-(r - 1) column
    11: (6, [(lambda n, b: n - b, True), (lambda n, b: 1, False), (lambda n, b: 65, True), (lambda n, b: n // 2 + 1, False), ("r-1", True)]),
    13: (1, [(lambda n, b: 63, True), (lambda n, b: 0, True), (lambda n, b: n // 2 + 1, False)]),
    16: (6, [(lambda n, b: n - b, True), ("r-1", True)]),
    17: (0, [(lambda n, b: n // 2, False), (lambda n, b: n, True)]),
    18: (6, [(lambda n, b: n - b - 1, True)]),
}


def ntt_src_case(api, O, k):
    """runs vdb_lagrange_to_coeff_src_dev on the case of size 2^k; returns (coefficients from the library, from the oracle)"""
    lib = api.init()
    n = 1 << k
    n_blind, spec = NTT_CASES[k]
    rng = np.random.default_rng(900 + k)
    stream = np.concatenate([fast_fr(rng, n + 4096), np.tile(O.fr_from_ints([R - 1]), (n, 1))])
    n_cols = len(spec)
    blind = fast_fr(rng, n_cols * max(n_blind, 1)).reshape(n_cols, max(n_blind, 1), 4)[:, :n_blind].copy()
    specs = []
    for c, (ln, given) in enumerate(spec):
        if ln == "r-1":
            blind[c] = O.fr_from_ints([R - 1])[0]
            specs.append((n + 4096, n - n_blind, c))
        else:
            specs.append((17 + 1031 * c, ln(n, n_blind), c if given else None))
    pool = Pool(api)
    try:
        d_stream, d_blind = pool.new(stream), pool.new(blind)
        d_src = pool.new(records(d_stream, specs, d_blind, n_blind))
        d_out = pool.alloc(n_cols * n * FR)
        api.check(lib.vdb_lagrange_to_coeff_src_dev(d_src.ptr, d_out.ptr, n_cols, k, n_blind))
        got = d_out.download((n_cols, n, 4))
    finally:
        pool.free()
    cols = np.stack([CM.materialise(stream, s, ln, None if b is None else blind[b], n, n_blind) for s, ln, b in specs])
    if "r-1" in [s[0] for s in spec]:
        assert (cols[-1] == O.fr_from_ints([R - 1])[0]).all()
    return got, O.lde_batch(cols, ext=0, threads=8)[0]


@pytest.mark.parametrize("k", sorted(NTT_CASES))
def test_lagrange_to_coeff_src(env, k):
    """k = 11 (the smallest accepted size, two passes) and 13, and the specialised first passes of 2^16, 2^17 and 2^18 rows: edge
    lengths scaled to the size, blinds given and null, n_blind 0 / 1 / 6, an all-(r - 1) column; the oracle's coefficients"""
    got, want = ntt_src_case(env.api, env.O, k)
    assert got.shape[0] == {11: 5, 13: 3, 16: 2, 17: 2, 18: 1}[k]
    assert np.array_equal(got, want), (k, np.flatnonzero((got != want).any(axis=(1, 2))))


def test_lagrange_to_coeff_src_refuses_single_pass_sizes(env, pool):
    k, n = 10, 1024
    d_src = pool.new(records(env.d_stream, [(5, 1000, None)], None, 6))
    pattern = np.full(n * FR, 0xA5, dtype=np.uint8)
    d_out = pool.new(pattern)
    assert env.lib.vdb_lagrange_to_coeff_src_dev(d_src.ptr, d_out.ptr, 1, k, 6) == ERR_ARG
    assert np.array_equal(d_out.download((n * FR,), dtype=np.uint8), pattern)


def test_lagrange_to_coeff_src_small_pass_sizes_in_a_subprocess():
    """VDB_NTT_MAX_S = 4 (read once per process): the source read in front of three- and four-digit decompositions, k = 11 and 13"""
    script = (
        "import numpy as np\n"
        "from halo2_vectordb_amd import api\n"
        "from oracle import oracle as O\n"
        "import test_gpu_commit_path as T\n"
        "api.init(0)\n"
        "for k in (11, 13):\n"
        "    got, want = T.ntt_src_case(api, O, k)\n"
        "    assert np.array_equal(got, want), k\n"
        "print('ok')\n")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, VDB_NTT_MAX_S="4", PYTHONPATH=root + os.pathsep + os.path.join(root, "tests"))
    r = subprocess.run([sys.executable, "-c", script], env=env, cwd=root, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout + r.stderr


# ------------------------------------------------------------------ i. the keygen side mask kernels
def test_const_mask_and_mask_select(env, pool):
    """vdb_layout_const_mask_dev: bit 1 of the flag bytes laid out by the model's descriptors, zero outside every column's cells; vdb_mask_select_dev with keep_const 0 and 1 against numpy, out of place and in place (keygen aliases them)"""
    O, api, lib = env.O, env.api, env.lib
    k = 8
    rows = 1 << k
    rng = np.random.default_rng(91)
    for tail in (1, 100, rows):
        bp = rng.integers(1, rows - 9, size=5).astype(np.uint64)
        bp[1] = rows - 1
        n_cells = int(bp.sum()) + tail
        flags = rng.integers(0, 8, size=n_cells + 8).astype(np.uint8)             # (the bytes past n_cells are never laid out)
        d_flags = pool.new(flags)
        d_mask = pool.new(np.full((len(bp) + 1) * rows, 0xCC, dtype=np.uint8))
        api.check(lib.vdb_layout_const_mask_dev(d_flags.ptr, n_cells, api._p(bp), len(bp), k, d_mask.ptr))
        got = d_mask.download((len(bp) + 1, rows), dtype=np.uint8)
        want = CM.const_mask(flags, n_cells, bp, k)
        assert np.array_equal(got, want), tail
        assert want.any() and not want.all()
    n = 3 * 256 + 77
    vals = O.random_fr(rng, n)
    vals[::5] = 0
    mask = rng.integers(0, 4, size=n).astype(np.uint8)                             # any non-zero byte flags the cell
    d_mask = pool.new(mask)
    for keep in (0, 1):
        want = vals.copy()
        want[(mask != 0) != bool(keep)] = 0
        d_in, d_out = pool.new(vals), pool.new(np.full((n + 1, 4), 7, dtype=np.uint64))
        api.check(lib.vdb_mask_select_dev(d_in.ptr, d_mask.ptr, n, keep, d_out.ptr))
        out = d_out.download((n + 1, 4))
        assert np.array_equal(out[:n], want) and (out[n] == 7).all(), keep
        assert np.array_equal(d_in.download((n, 4)), vals)
        api.check(lib.vdb_mask_select_dev(d_in.ptr, d_mask.ptr, n, keep, d_in.ptr))
        assert np.array_equal(d_in.download((n, 4)), want), keep
