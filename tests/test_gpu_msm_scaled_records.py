"""k_msm_sort's scaled-short records on the card: commitments of columns built around the record's edges against oracle.msm_batch on the
same columns, exactly.  n = 2,048 rows (the smallest size at which the 1,024-thread walk makes two trips and the queue of long scalars
is filled from both), 24 columns in one batch per window size (several workgroups share the segment and range counters), window sizes
11 (the default), 5 and 8 through the records and the queue, 14 once through the dense walk.

Columns: the scalar families of tests/msm_digits_model.py (tests/test_msm_digits_cpu.py holds their digit lists to integers), one or
more columns each, laid so that every 64-row group — one wavefront of the walk — mixes zeros, values short as they stand, values short
only after scaling, and long ones; one scaled-short value repeated down all rows (one heavy bucket in a high window); a column in which
every row is long (the queue holds n entries); one with no long value (empty queue); one all zero; one of random full-width scalars.
Then the two entry points the proof step commits through, vdb_msm_batch_src_dev_begin and the masked one, over the same columns."""
import random

import numpy as np
import pytest

import commit_path_model as CM
import msm_digits_model as M
from test_gpu_commit_path import Pool, blinds, masked_sum, msm_deferred, msm_src, pt_add, records

pytestmark = pytest.mark.gpu

R = M.R
K = 11
ROWS = 1 << K
N_COLS = 24
N_BLIND = 6


def plain_short(rng, c):
    """short as it stands: bit length within the limit, lowest window not empty (j0 = 0)"""
    return rng.getrandbits(rng.randint(1, M.short_bits(c))) | 1


def scaled_short(rng, c):
    """short only by scaling: a mantissa within the limit at a window j0 >= 1 that puts the value's bit length past the limit"""
    W = M.windows(c)
    while True:
        nbp = rng.randint(1, M.short_bits(c))
        a = rng.getrandbits(nbp) | 1 << (nbp - 1) | 1
        v = a << (c * rng.randint(1, W - 1))
        if v <= M.HALF and v.bit_length() > M.short_bits(c):
            return v


def long_value(rng, c):
    while True:
        v = rng.randrange(R)
        if M.classify(v, c)[0] == M.LONG:
            return v


def signed(rng, v):
    return v if rng.random() < 0.5 else (R - v) % R


def kind_of(v, c):
    """0 zero, 1 short as it stands, 2 short only by scaling, 3 long"""
    k, j0, _, _ = M.classify(v, c)
    if k == M.ZERO:
        return 0
    if k == M.LONG:
        return 3
    return 1 if M.fold(v)[0].bit_length() <= M.short_bits(c) else 2


def mixed_column(rng, c, members):
    """ROWS scalars: per 64-row group 36 members of the family and 7 each of zero, short, scaled-short and long, shuffled"""
    col, it = [], 0
    for _ in range(ROWS // 64):
        grp = [members[(it + i) % len(members)] for i in range(36)]
        it += 36
        grp += [0] * 7 + [signed(rng, plain_short(rng, c)) for _ in range(7)] + [signed(rng, scaled_short(rng, c)) for _ in range(7)]
        grp += [long_value(rng, c) for _ in range(7)]
        rng.shuffle(grp)
        col += grp
    return col


def build_columns(c, seed):
    """(N_COLS x ROWS canonical integers, names)"""
    rng = random.Random(seed)
    fam = M.families(c, rng, n_random=ROWS)
    cols, names = [], []
    heavy = scaled_short(rng, c)
    cols.append([heavy] * ROWS), names.append("one scaled-short value")
    cols.append([R - heavy] * ROWS), names.append("one scaled-short value, negated")
    cols.append([long_value(rng, c) for _ in range(ROWS)]), names.append("all long")
    cols.append([signed(rng, plain_short(rng, c) if i % 3 else scaled_short(rng, c)) if i % 5 else 0 for i in range(ROWS)]), names.append("no long")
    cols.append([0] * ROWS), names.append("all zero")
    cols.append([rng.randrange(R) for _ in range(ROWS)]), names.append("random full-width")
    # fixed-point shaped: small integers times 2^48, 2^96, 2^144, both signs (what the circuits' advice cells look like)
    cols.append([signed(rng, rng.getrandbits(rng.randint(1, 20)) << (48 * rng.randint(0, 3))) for _ in range(ROWS)]), names.append("fixed-point")
    order = ["edge", "pow", "ones", "reach-W", "random", "sparse"]
    shuffled = {k: rng.sample(v, len(v)) for k, v in fam.items()}
    used = {k: 0 for k in order}
    i = 0
    while len(cols) < N_COLS:
        k = order[i % len(order)]
        i += 1
        vs = shuffled[k]
        take = 36 * (ROWS // 64)
        members = [vs[(used[k] + t) % len(vs)] for t in range(take)]
        used[k] += take
        cols.append(mixed_column(rng, c, members)), names.append("family " + k)
    for name, col in zip(names, cols):
        assert len(col) == ROWS and all(0 <= v < R for v in col)
        kinds = [kind_of(v, c) for v in col]
        if name.startswith("family"):
            for g in range(0, ROWS, 64):
                assert set(kinds[g: g + 64]) == {0, 1, 2, 3}, (name, g)
    k3 = [kind_of(v, c) for v in cols[2]]
    assert set(k3) == {3} and 3 not in {kind_of(v, c) for v in cols[3]} and kind_of(heavy, c) == 2
    assert {n for n in names if n.startswith("family")} == {"family " + k for k in order}
    return cols, names


class Env:
    pass


@pytest.fixture(scope="module")
def env(O, PY):
    from halo2_vectordb_amd import api
    e = Env()
    e.api, e.lib, e.O, e.PY = api, api.init(), O, PY
    e.g, e.gl = O.srs_from_tau(K, 0x5CA1ED)
    e.cache = {}
    return e


def columns(env, c):
    """the columns of window size c, their Montgomery words and the oracle's commitments: computed once, shared, never changed"""
    if c not in env.cache:
        ints, names = build_columns(c, 20261020 + c)
        cols = np.stack([env.O.fr_from_ints(col) for col in ints])
        want = env.O.msm_batch(cols, env.gl, threads=8)
        cols.setflags(write=False)
        want.setflags(write=False)
        env.cache[c] = (cols, names, want, ints)
    return env.cache[c]


@pytest.fixture
def pool(env):
    p = Pool(env.api)
    yield p
    p.free()


@pytest.mark.parametrize("window_bits", [0, 5, 8, 14])
def test_commitments_of_the_record_edges(env, window_bits):
    c = window_bits or 11
    cols, names, want, _ = columns(env, c)
    srs = env.api.Srs(K, env.g, env.gl, window_bits=window_bits)
    try:
        assert srs.info()[1:] == (c, M.windows(c))
        got = env.api.msm_batch(srs, cols, basis=1)
    finally:
        srs.free()
    bad = [names[i] for i in np.flatnonzero((got != want).any(axis=1))]
    assert not bad, (c, bad)
    assert not got[names.index("all zero")].any()


def test_column_source_entry_with_scaled_short_values(env, pool):
    """vdb_msm_batch_src_dev_begin: every column a descriptor into one stream, N_BLIND blinding rows at its end (null on every third)"""
    O, c = env.O, 11
    cols, names, _, _ = columns(env, c)
    n = ROWS
    stream = np.ascontiguousarray(cols.reshape(N_COLS * ROWS, 4))
    rng = np.random.default_rng(77)
    blind = blinds(O, rng, N_COLS, N_BLIND)
    specs = [(col * ROWS, n - N_BLIND - (col % 5), None if col % 3 == 2 else col) for col in range(N_COLS)]
    d_stream, d_blind = pool.new(stream), pool.new(blind)
    d_src = pool.new(records(d_stream, specs, d_blind, N_BLIND))
    mat = np.stack([CM.materialise(stream, s, ln, None if b is None else blind[b], n, N_BLIND) for s, ln, b in specs])
    want = O.msm_batch(mat, env.gl, threads=8)
    srs = env.api.Srs(K, env.g, env.gl)
    try:
        got = msm_src(env, srs, 1, d_src, N_COLS, n, N_BLIND)
    finally:
        srs.free()
    bad = [names[i] for i in np.flatnonzero((got != want).any(axis=1))]
    assert not bad, bad


def test_masked_entry_with_scaled_short_values_in_the_unmasked_rows(env, pool):
    """vdb_msm_batch_masked_dev_begin: a mask that flags the plain-short and the long cells of the even columns and a random half of the odd
    ones' cells, so what stays is scaled-short (and zero) on the even columns; a constant point per column"""
    O, PY, c = env.O, env.PY, 11
    cols, names, _, ints = columns(env, c)
    rng = np.random.default_rng(78)
    mask = (rng.random((N_COLS, ROWS)) < 0.5).astype(np.uint8)
    for col in range(0, N_COLS, 2):
        mask[col] = [kind_of(v, c) in (1, 3) for v in ints[col]]
    kept_scaled = sum(kind_of(v, c) == 2 and not mask[col, i] for col in range(0, N_COLS, 2) for i, v in enumerate(ints[col]))
    assert kept_scaled > 1000
    pts = O.g1_mul_generator([int(v) for v in rng.integers(2, 1 << 62, size=N_COLS)])
    S = masked_sum(O, np.array(cols), mask, env.gl)
    want = np.stack([pt_add(O, PY, S[col], pts[col]) for col in range(N_COLS)])
    d_cols, d_mask, d_pts = pool.new(np.array(cols)), pool.new(mask), pool.new(pts)
    srs = env.api.Srs(K, env.g, env.gl)
    try:
        got = msm_deferred(env, srs, 1, d_cols, N_COLS, ROWS, d_mask, d_pts)
    finally:
        srs.free()
    bad = [names[i] for i in np.flatnonzero((got != want).any(axis=1))]
    assert not bad, bad
