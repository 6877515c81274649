"""The MSM's bucket folding (k_msm_combine, k_msm_reduce on the nine-limb xyzz_add_l9; k_msm_normalise, one lane per column) on
columns built to walk its branches, bit exact against the oracle's msm_batch — with constant points, against the oracle's sum plus the
point.  2^11 and 2^12 rows, 11-bit and 14-bit windows, 67 columns (not a multiple of the 64 lanes of a normalising wavefront), the
deferred and the non-deferred tail, with and without per-column constant points, with and without the constant mask.

The SRS repeats and negates bases: g[17] = g[40] = g[50] = g[3] = P, g[18] = g[41] = g[60] = -P, and every base of the upper half of the
rows is P.  On the upper half every segment of a bucket then sums to a multiple of P whatever order the sort leaves the entries in, so
the combine tree adds equal partials (all scalars equal: P + P at every level) and opposite ones (s on one half of the rows, r - s on the
other).  Single cells on rows 3, 17, 18, 40, 41 put P and -P into chosen buckets of one lane's slice of k_msm_reduce, or of two lanes:
`running` meets its own value (doubling) and its negative (back to the identity), `total` meets `running` right after the first
non-empty bucket with and without a gap, `total` meets -`running`, and the lane scan and tree meet equal and opposite lane sums."""
import numpy as np
import pytest

from test_gpu_commit_path import Pool, msm_deferred, msm_masked, msm_plain, pt_add, pt_neg
from test_gpu_msm import witness_like

pytestmark = pytest.mark.gpu

R = 0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001
N_COLS = 67
KS = (11, 12)
WINDOWS = (11, 14)
P_ROWS, N_ROWS = (3, 17, 40, 50), (18, 41, 60)


def sparse(O, n, cells):
    v = [0] * n
    for row, s in cells.items():
        v[row] = s % R
    return O.fr_from_ints(v)


def upper(O, n, vals):
    """zeros on the lower half of the rows, vals on the upper half (every base there is P)"""
    return O.fr_from_ints([0] * (n // 2) + [x % R for x in vals])


def columns(O, rng, n):
    h = n // 2
    s = int(O.fr_to_ints(O.random_fr(rng, 1))[0])
    t = int(O.fr_to_ints(O.random_fr(rng, 1))[0])
    cols = [
        np.zeros((n, 4), dtype=np.uint64),                                   # 0: the identity, (0, 0)
        sparse(O, n, {5: 1}),                                                # one cell, digit 1: the last bucket of lane 0's walk
        sparse(O, n, {6: 1 << 10}), sparse(O, n, {7: 1 << 13}),              # the top bucket of an 11-bit and of a 14-bit window
        sparse(O, n, {8: 88}), sparse(O, n, {9: 704}),                       # the middle of a lane's slice (16 resp. 128 buckets a lane)
        sparse(O, n, {10: s}),                                               # one full-width scalar: one bucket per window, all over the lanes
        O.fr_from_ints([s] * n), O.fr_from_ints([3] * n),                    # all equal: one bucket, many segments, the whole combine tree
        O.fr_from_ints([R - 1] * n),
        O.fr_from_ints([s if i % 2 == 0 else R - s for i in range(n)]),
        witness_like(O, rng, n), O.random_fr(rng, n),
        # equal bases: the combine tree on equal and on opposite partials
        upper(O, n, [7] * h), upper(O, n, [7 if i % 2 == 0 else -7 for i in range(h)]),
        upper(O, n, [7] * (h // 2) + [-7] * (h // 2)), upper(O, n, [9] * (3 * h // 4) + [-9] * (h // 4)),
        upper(O, n, [t] * (h // 2) + [-t] * (h // 2)),
        # k_msm_reduce, one lane's slice (ids 97 .. 112 of lane 6 with 11-bit windows, of lane 0 with 14-bit ones)
        sparse(O, n, {3: 101, 17: 100}),                                     # running = P meets the bucket sum P: doubling
        sparse(O, n, {3: 101, 18: 100}),                                     # ... meets -P: running back to the identity, total stays
        sparse(O, n, {3: 101, 18: 100, 41: 100}),                            # running = -P, total = P: total + running cancels
        sparse(O, n, {3: 101, 17: 99}),                                      # total = running over a gap, then the same point again
        sparse(O, n, {3: 112, 17: 97}), sparse(O, n, {3: 112, 18: 97}),      # the ends of the slice
        # two and three lanes: the suffix scan and the tree on equal and opposite lane sums
        sparse(O, n, {3: 100, 17: 116, 40: 228}), sparse(O, n, {3: 100, 18: 116, 41: 228}), sparse(O, n, {3: 100, 18: 116}),
        sparse(O, n, {3: 100, 17: 116, 18: 228, 41: 356}),
        # all of a column's weight cancels: the identity out of the reduce tree
        sparse(O, n, {3: s, 18: s}), sparse(O, n, {3: s, 17: s, 18: s, 41: s}),
    ]
    while len(cols) < N_COLS:                                                # a few cells each, short and long scalars
        cells = {int(r): (int(rng.integers(1, 1 << 14)) if i % 2 else int(O.fr_to_ints(O.random_fr(rng, 1))[0]))
                 for i, r in enumerate(rng.choice(n, size=5, replace=False))}
        cols.append(sparse(O, n, cells))
    return np.stack(cols)


class Ref:
    pass


@pytest.fixture(scope="module")
def refs(O, PY):
    """per row count: the bases, the columns, a mask, constant points, and the oracle's answers — computed once, never written to"""
    out = {}
    for k in KS:
        n = 1 << k
        rng = np.random.default_rng(20261019 + k)
        r = Ref()
        g, _ = O.srs_from_tau(k, 0xF01D + k)
        P = g[3].copy()
        Pn = pt_neg(O, PY, P)
        for i in P_ROWS[1:]:
            g[i] = P
        for i in N_ROWS:
            g[i] = Pn
        g[n // 2:] = P
        r.g, r.n = g, n
        r.cols = columns(O, rng, n)
        assert r.cols.shape == (N_COLS, n, 4) and N_COLS % 64
        r.want = O.msm_batch(r.cols, g, threads=8)
        assert not any(r.want[c].any() for c in (0, 14, 15, 17, 28, 29)) and all(r.want[c].any() for c in (13, 16, 18, 19, 27))
        r.mask = (rng.random((N_COLS, n)) < 0.3).astype(np.uint8)
        r.mask[:, list(P_ROWS + N_ROWS)] = 0                                 # the cells that build the exceptional cases stay
        r.mask[2] = 1                                                        # a column with every cell masked: the constant point alone
        masked = r.cols.copy()
        masked[r.mask.astype(bool)] = 0
        r.want_masked = O.msm_batch(masked, g, threads=8)
        # constant points: random, the identity, the column's own sum (a doubling in the last addition) and its negative (the identity)
        pts = O.g1_mul_generator([int(x) for x in rng.integers(1, 1 << 62, size=N_COLS)])
        pts[1] = 0
        pts[4] = 0
        for c in (5, 11, 18):
            pts[c] = r.want[c]
        for c in (6, 12, 19):
            pts[c] = pt_neg(O, PY, r.want[c])
        r.pts = pts
        r.want_pts = np.stack([pt_add(O, PY, r.want[c], pts[c]) for c in range(N_COLS)])
        r.want_masked_pts = np.stack([pt_add(O, PY, r.want_masked[c], pts[c]) for c in range(N_COLS)])
        assert not r.want_pts[6].any() and not r.want_pts[12].any() and r.want_pts[5].any()
        for a in (r.g, r.cols, r.want, r.want_masked, r.mask, r.pts, r.want_pts, r.want_masked_pts):
            a.setflags(write=False)
        out[k] = r
    return out


class Env:
    pass


@pytest.fixture(scope="module")
def env(O, PY):
    from halo2_vectordb_amd import api
    e = Env()
    e.api, e.lib, e.O, e.PY = api, api.init(), O, PY
    return e


@pytest.fixture(params=[(k, c) for k in KS for c in WINDOWS], ids=lambda p: f"rows2^{p[0]}-window{p[1]}")
def case(request, env, refs):
    k, c = request.param
    r = refs[k]
    srs = env.api.Srs(k, np.array(r.g), None, window_bits=c)
    assert srs.info()[1] == c
    pool = Pool(env.api)
    d_cols = pool.new(r.cols)
    d_mask = pool.new(r.mask)
    d_pts = pool.new(r.pts)
    # the library takes the mask and the constant points together: no cell masked, resp. every point the identity, stand for "without"
    d_none, d_ident = pool.new(np.zeros_like(r.mask)), pool.new(np.zeros_like(r.pts))
    yield r, srs, d_cols, d_mask, d_pts, d_none, d_ident
    pool.free()
    srs.free()


def same(got, want, what):
    assert np.array_equal(got, want), (what, np.flatnonzero((got != want).any(axis=1)))


def test_fold_plain_and_deferred(env, case):
    r, srs, d_cols = case[:3]
    same(msm_plain(env, srs, 0, d_cols, N_COLS, r.n), r.want, "non-deferred")
    same(msm_deferred(env, srs, 0, d_cols, N_COLS, r.n), r.want, "deferred")
    # fewer columns than one normalising wavefront has lanes, and exactly that many
    for m in (1, 64):
        same(msm_plain(env, srs, 0, d_cols, m, r.n), r.want[:m], ("non-deferred", m))


def test_fold_with_constant_points(env, case):
    r, srs, d_cols, _, d_pts, d_none, _ = case
    got = msm_deferred(env, srs, 0, d_cols, N_COLS, r.n, d_none, d_pts)
    same(got, r.want_pts, "deferred, constant points")
    same(msm_masked(env, srs, 0, d_cols, N_COLS, r.n, d_none, d_pts), r.want_pts, "non-deferred, constant points")
    assert not got[6].any() and not got[12].any() and not got[19].any()      # the sum and its negative: (0, 0)


def test_fold_with_constant_mask_and_points(env, case):
    r, srs, d_cols, d_mask, d_pts, _, d_ident = case
    same(msm_masked(env, srs, 0, d_cols, N_COLS, r.n, d_mask, d_pts), r.want_masked_pts, "non-deferred, mask and points")
    same(msm_deferred(env, srs, 0, d_cols, N_COLS, r.n, d_mask, d_pts), r.want_masked_pts, "deferred, mask and points")
    same(msm_deferred(env, srs, 0, d_cols, N_COLS, r.n, d_mask, d_ident), r.want_masked, "deferred, mask alone")
    assert np.array_equal(r.want_masked_pts[2], r.pts[2])                    # every cell masked: the constant point alone
