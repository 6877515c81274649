"""Every cell of the approximate-nearest-neighbour query circuit altered alone, without a GPU: circuit_sym.build_ann_query on the host
builder and tests/ann_model.py's witness through tests/alteration_model.py, by the sweep of tests/test_alteration_cpu.py, at the two
smallest shapes (n 2, K 2: two one-leaf trees and a sponge over three words; n 5, K 1: a one-word indicator, a padded tree and a sponge
over two words).  This file keeps no allow-list of its own: a cell may stay unnoticed only for a reason alteration_model.explain
states with the reference's line, and the cells of the blocks this circuit adds — the selection, the tie of the selected root, the
sponge's absorbed words, the zero cell the second tree's padding copies — are required to be noticed without exception."""
import numpy as np
import pytest

import alteration_model as AM
import ann_model as AN
import topk_model as TM
from halo2_vectordb_amd import circuit_sym as CS
from test_alteration_cpu import sweep
from test_ann_cpu import P, L, _setup, _winner
from test_merkle_update_cpu import fetchers

SHAPES = [(2, 2, [1, 0]), (1, 5, [0] * 5)]               # K, n, ids


def ann_case(O, K, n, ids):
    db, ids, cent, query = _setup(O, seed=9 + K, n=n, K=K, ids=ids)
    ix = AN.index_model(O, db, ids, cent)
    members, _ = AN.select_cluster(db, ids, _winner(O, query, cent))
    assert AN.distances_distinct(O, "euclidean", query, cent, P, L) and AN.distances_distinct(O, "euclidean", query, members, P, L)
    m = AN.query_model(O, "euclidean", query, cent, members, ix["roots"][1:1 + K], P, L)
    ff, fv, vals = fetchers(m)
    cm, public, info = CS.build_ann_query("euclidean", K, members.shape[0], 4, P, L, ff, fv)
    return m, cm, public, info, vals


def new_ground(info):
    """[lo, hi) spans of what only this circuit places: everything from the selection to the end, and the assigned cluster roots"""
    lay = info["layout"]
    return [(lay["roots"], lay["n_in"]), (lay["select"], lay["total"])]


@pytest.mark.parametrize("K,n,ids", SHAPES)
def test_every_cell_altered_alone(O, K, n, ids):
    m, cm, public, info, vals = ann_case(O, K, n, ids)
    free = sweep(f"ann euclidean K {K} n {n} dim 4", cm, vals, TM.to_ints(m["lookup"]), public, L, m["flags"])
    # the only cells that stay free are the reference's own, inside the two nearest_vector blocks (GateChip::is_zero of a zero operand)
    assert [AM.explain(cm, vals, c) for c in free] == [AM.IS_ZERO_INVERSE] * len(free), free
    lay = info["layout"]
    assert all(lay["nearest_c"] <= c < lay["merkle_c"] or lay["nearest_m"] <= c < lay["merkle_m"] for c in free), free
    for lo, hi in new_ground(info):
        assert not [c for c in free if lo <= c < hi]
