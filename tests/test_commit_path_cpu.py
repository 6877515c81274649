"""The commit path's plain model (tests/commit_path_model.py) checked against itself and against the oracle's column layout, so that
tests/test_gpu_commit_path.py can hold the library to it."""
import numpy as np
import pytest

import commit_path_model as CM

R = CM.R


@pytest.mark.parametrize("c", range(2, 15))
def test_signed_digits_recompose_to_the_scalar(c):
    """every edge scalar of the recoding and a few random ones: the signed sum of d_j 2^(c j) is the scalar modulo r, every digit is
    non-zero, at most 2^(c-1) in magnitude, one per window, windows below W"""
    W = CM.windows(c)
    rng = np.random.default_rng(1400 + c)
    scalars = CM.edge_scalars(c) + [int.from_bytes(rng.bytes(32), "little") % R for _ in range(64)]
    assert {0, 1, R - 1, (R - 1) // 2, (R + 1) // 2, (1 << 32) - 1, 1 << 32, R - (1 << 32), (1 << 253) % R} <= set(scalars)
    for s in scalars:
        digs = CM.signed_digits(s, c, W)
        assert sum(d << (c * j) for j, d in digs) % R == s, (c, hex(s))
        assert all(d != 0 and abs(d) <= 1 << (c - 1) for _, d in digs), (c, hex(s))
        js = [j for j, _ in digs]
        assert js == sorted(set(js)) and all(0 <= j < W for j in js), (c, hex(s))
    assert CM.signed_digits(0, c, W) == []
    assert CM.signed_digits(1, c, W) == [(0, 1)] and CM.signed_digits(R - 1, c, W) == [(0, -1)]
    # the largest digit that does not carry, and the first that does
    assert CM.signed_digits(1 << (c - 1), c, W) == [(0, 1 << (c - 1))]
    assert CM.signed_digits((1 << (c - 1)) + 1, c, W) == [(0, -((1 << (c - 1)) - 1)), (1, 1)]


def test_count_entries_counts_unmasked_digits():
    c, W = 11, CM.windows(11)
    col = [0, 1, R - 1, (1 << 11) - 1, 1 << 10, (1 << 10) + 1, 0, 5]
    per_cell = [0, 1, 1, 2, 1, 2, 0, 1]          # 2^11 - 1: digit -1 and a carry; 2^10 + 1 = 2^11 - (2^10 - 1): the same
    assert [len(CM.signed_digits(v, c, W)) for v in col] == per_cell
    assert CM.count_entries(col, None, c, W) == sum(per_cell)
    mask = [0, 1, 0, 1, 0, 0, 1, 0]
    assert CM.count_entries(col, mask, c, W) == sum(n for n, m in zip(per_cell, mask) if not m)
    assert CM.count_entries(col, [1] * len(col), c, W) == 0


def test_descriptors_by_hand():
    # three break points at k = 4: columns of 13, 14 and 12 cells and a last one with the rest
    assert CM.descriptors(50, [12, 13, 11], 4, 0, 4) == [(0, 13), (12, 14), (25, 12), (36, 14)]
    assert CM.descriptors(50, [12, 13, 11], 4, 1, 3) == [(12, 14), (25, 12)]
    assert CM.descriptors(50, [12, 13, 11], 4, 2, 2) == []
    assert CM.descriptors(5, [], 4, 0, 1) == [(0, 5)]
    # lookup columns of 16 - 9 = 7 cells: a stream that ends on a column boundary, one shorter than a column, columns past the end
    assert CM.descriptors_lookup(14, 4, 9, 0, 3) == [(0, 7), (7, 7), (0, 0)]
    assert CM.descriptors_lookup(3, 4, 9, 0, 2) == [(0, 3), (0, 0)]
    assert CM.descriptors_lookup(15, 4, 9, 1, 3) == [(7, 7), (14, 1)]


def test_materialise_by_hand():
    stream = np.arange(40, dtype=np.uint64).reshape(10, 4) + 1
    blind = np.full((2, 4), 99, dtype=np.uint64)
    col = CM.materialise(stream, 3, 4, blind, 8, 2)
    assert np.array_equal(col[:4], stream[3:7]) and not col[4:6].any() and np.array_equal(col[6:], blind)
    col = CM.materialise(stream, 3, 4, None, 8, 2)
    assert np.array_equal(col[:4], stream[3:7]) and not col[4:].any()
    assert not CM.materialise(stream, 0, 0, None, 8, 0).any()
    assert np.array_equal(CM.materialise(stream, 2, 8, blind, 8, 0), stream[2:10])


def test_materialise_agrees_with_the_oracle_layout(O):
    """a small k-means context planned at k = 10: the model's descriptors, materialised, are the oracle's advice and lookup columns;
    with blinds the rows outside the blinding rows stay what they were"""
    k, min_rows = 10, 9
    rows = 1 << k
    qv = O.quantize(np.random.default_rng(8).integers(0, 219, size=(12, 8)).astype(np.float64), 48)
    c = O.Ctx(store=True, keygen=True, plan_k=k)
    c.assign_witnesses(qv)
    c.kmeans("euclidean", qv, 2, 2, P=48, L=9)
    stream, lookup, bp = c.advice(), c.lookup(), c.break_points()
    assert len(bp) >= 1, "more than one advice column is what this test is about"
    n_adv = len(bp) + 1
    want = O.layout_columns(stream, bp, k, n_adv)
    assert want.shape[0] == n_adv
    desc = CM.descriptors(len(stream), bp, k, 0, n_adv)
    got = np.stack([CM.materialise(stream, s, ln, None, rows, 7) for s, ln in desc])
    assert np.array_equal(got, want)
    for col in range(len(bp)):                      # the cell on the break row opens the next column
        assert np.array_equal(got[col, int(bp[col])], got[col + 1, 0])
    assert CM.descriptors(len(stream), bp, k, 1, n_adv) == desc[1:]
    n_lk = -(-len(lookup) // (rows - min_rows))
    want_lk = O.layout_lookup(lookup, k, n_lk, min_rows)
    desc_lk = CM.descriptors_lookup(len(lookup), k, min_rows, 0, n_lk + 1)
    assert desc_lk[-1] == (0, 0) and want_lk.shape[0] == n_lk
    got_lk = np.stack([CM.materialise(lookup, s, ln, None, rows, 7) for s, ln in desc_lk[:n_lk]])
    assert np.array_equal(got_lk, want_lk)
    blind = np.random.default_rng(9).integers(1, 1 << 62, size=(n_adv, 7, 4)).astype(np.uint64)
    for col, (s, ln) in enumerate(desc):
        assert ln + 7 <= rows                       # minimum_rows = 9 leaves the blinding rows free
        b = CM.materialise(stream, s, ln, blind[col], rows, 7)
        assert np.array_equal(b[: rows - 7], want[col, : rows - 7]) and np.array_equal(b[rows - 7:], blind[col])
    # the mask image follows the same descriptors
    flags = np.random.default_rng(10).integers(0, 8, size=len(stream)).astype(np.uint8)
    m = CM.const_mask(flags, len(stream), bp, k)
    for col, (s, ln) in enumerate(desc):
        assert np.array_equal(m[col, :ln], (flags[s:s + ln] >> 1) & 1) and not m[col, ln:].any()
