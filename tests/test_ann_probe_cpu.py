"""The query over the p nearest clusters without a GPU: tests/ann_probe_model.py held against the single-probe model at p = t = 1,
circuit_sym.ann_probe_layout against the model's regions on every test shape, circuit_sym.build_ann_probe on the host builder against the
model's witness (nothing violated, the public cells, every sel_r = mroot_r tie), every cell altered alone at the smallest shape, and three
altered witnesses the map has to notice: clusters swapped against round order, an unprobed cluster, an altered cluster root."""
import numpy as np
import pytest

import alteration_model as AM
import ann_model as AN
import ann_probe_model as PM
import topk_model as TM
from halo2_vectordb_amd import circuit_sym as CS
from ann_probe_model import DIM, L, P
from test_alteration_cpu import sweep
from test_merkle_update_cpu import fetchers


def _layout(c):
    return CS.ann_probe_layout("euclidean", c["K"], c["sizes"], DIM, c["p"], c["t"], P, L)


def _build(c, m, sizes=None):
    ff, fv, vals = fetchers(m)
    cm, public, info = CS.build_ann_probe("euclidean", c["K"], c["sizes"] if sizes is None else sizes, DIM, c["p"], c["t"], P, L, ff, fv)
    return cm, public, info, vals


def test_one_probe_one_neighbour_is_the_single_probe_model(O):
    c = PM.case(O, "1-4-7")
    want = AN.query_model(O, "euclidean", c["query"], c["cent"], c["members"][0], c["roots"], P, L, plan_k=13)
    got = PM.probe_model(O, "euclidean", c["query"], c["cent"], c["members"][:1], c["roots"], 1, P, L, plan_k=13)
    for key in ("advice", "lookup", "flags", "selectors", "public", "break_points"):
        assert np.array_equal(got[key], want[key]), key
    assert got["n_in"] == want["n_in"] and got["selected"] == [want["selected"]] and got["members_roots"] == [want["members_root"]]
    lay, one = CS.ann_probe_layout("euclidean", 3, [7], DIM, 1, 1, P, L), CS.ann_query_layout("euclidean", 3, 7, DIM, P, L)
    assert (lay["total"], lay["total_l"], lay["merkle_m"], lay["select"], lay["sponge"]) == (one["total"], one["total_l"], [one["merkle_m"]], [one["select"]],
                                                                                             one["sponge"])


@pytest.mark.parametrize("name", list(PM.CASES))
def test_layout_is_the_models_regions(O, name):
    c, m = PM.case(O, name), PM.case_model(O, name)
    lay = _layout(c)
    assert {k: lay[k] for k in m["regions"]} == m["regions"]
    assert lay["total"] == m["advice"].shape[0] and lay["total_l"] == m["lookup"].shape[0] and lay["n_in"] == m["n_in"]
    assert lay["zero_cell"] == m["zero_cell"] and lay["N"] == sum(c["sizes"])
    if m["zero_cell"] is not None:
        assert m["flags"][m["zero_cell"]] == 2 and not m["advice"][m["zero_cell"]].any()


def test_zero_chain_shape_is_what_it_is_for(O):
    """K a power of two: the centroids' tree loads no zero cell; the probed sizes are (power of two, padded, padded) in round order, the
    first padded members' tree emits the cell and the next copies it"""
    c = PM.case(O, "zero-chain")
    lay = _layout(c)
    leaf = CS.merkle_leaf_layout(DIM)["leaf_cells"]
    assert c["K"] == 4 and c["sizes"] == [2, 3, 3] and lay["zero_cached"] == [False, False, True]
    assert lay["zero_cell"] == lay["merkle_m"][1] + 3 * leaf
    assert lay["merkle_m"][2] - lay["merkle_m"][1] == CS.merkle_cells(3, DIM) == lay["select"][0] - lay["merkle_m"][2] + 1


@pytest.mark.parametrize("name", list(PM.CASES))
def test_host_map_holds_the_models_witness(O, name):
    c, m = PM.case(O, name), PM.case_model(O, name)
    cm, public, info, vals = _build(c, m)
    assert cm.n_cells == m["advice"].shape[0] and len(cm.lookup_src) == m["lookup"].shape[0]
    rep = cm.check_witness(vals, TM.to_ints(m["lookup"]), m["flags"])
    assert not any(rep.values()), rep
    assert [vals[x] for x in public] == TM.to_ints(m["public"]) and len(public) == c["t"] * DIM + 1
    assert np.array_equal(np.asarray(cm.gate), m["selectors"].astype(bool))
    lay = info["layout"]
    for r in range(c["p"]):
        assert cm.copy_of[info["selected"][r]] == info["members_roots"][r] < info["selected"][r] == lay["select"][r] + 3 * c["K"]
        assert vals[info["selected"][r]] == m["selected"][r] == m["members_roots"][r] == TM.to_ints(c["roots"][c["rounds"][r]][None])[0]
    for key, want in (("centroid_indicators", m["centroid_indicators"]), ("candidate_indicators", m["candidate_indicators"]), ("results", m["results"])):
        assert [vals[x] for x in info[key].reshape(-1)] == TM.to_ints(want), key
    if lay["zero_cell"] is not None:                         # every padded tree behind the first copies the one zero cell
        users = np.flatnonzero(cm.copy_of == lay["zero_cell"])
        assert cm.const_idx[lay["zero_cell"]] >= 0 and len(users) >= 1 + sum(lay["zero_cached"][r] and (c["sizes"][r] & (c["sizes"][r] - 1)) != 0
                                                                              for r in range(c["p"]))


def test_every_cell_altered_alone(O):
    """tests/alteration_model.py's method at "1-1", p = t = 2: the only cells that stay free are the reference's own — the inverse witness
    of an is_zero with zero operand inside one of the two nearest blocks; none lies in the assigned inputs, the selections or the sponge"""
    c, m = PM.case(O, "1-1"), PM.case_model(O, "1-1")
    cm, public, info, vals = _build(c, m)
    free = sweep("ann probe euclidean 1-1 p 2 t 2 dim 4", cm, vals, TM.to_ints(m["lookup"]), public, L, m["flags"])
    lay = info["layout"]
    assert [AM.explain(cm, vals, x) for x in free] == [AM.IS_ZERO_INVERSE] * len(free), free
    assert all(lay["nearest_c"] <= x < lay["merkle_c"] or lay["nearest_m"] <= x < lay["merkle_m"][0] for x in free), free
    assert not [x for x in free if x < lay["n_in"] or x >= lay["select"][0]]


def _violations(O, c, members, roots, sizes):
    m = PM.probe_model(O, "euclidean", c["query"], c["cent"], members, roots, c["t"], P, L)
    cm, _, info, vals = _build(c, m, sizes=sizes)
    return cm.check_witness(vals, TM.to_ints(m["lookup"]), m["flags"]), m, info, vals


def test_altered_witnesses_break_a_copy_or_change_the_index_root(O):
    c = PM.case(O, "1-4-7")                                  # rounds [2, 0], sizes [7, 1]
    good = PM.case_model(O, "1-4-7")
    # the two clusters swapped against round order: both selections meet the other cluster's root
    rep, m, info, vals = _violations(O, c, c["members"][::-1], c["roots"], c["sizes"][::-1])
    assert rep["copies_unequal"] == 2 and all(vals[info["selected"][r]] != vals[info["members_roots"][r]] for r in range(2))
    assert np.array_equal(m["public"][-1], good["public"][-1])
    # a probed cluster replaced by the one no round states
    other = AN.select_cluster(c["db"], c["ids"], 1)[0]
    rep, m, info, vals = _violations(O, c, [c["members"][0], other], c["roots"], [7, 4])
    assert rep["copies_unequal"] == 1 and vals[info["selected"][1]] != vals[info["members_roots"][1]]
    # one altered cluster root: its selection no longer meets the members' root, and the index root is another
    roots = c["roots"].copy()
    roots[2] = O.fr_add(roots[2:3], O.fr_from_ints([1]))[0]
    rep, m, info, vals = _violations(O, c, c["members"], roots, c["sizes"])
    assert rep["copies_unequal"] >= 1 and vals[info["selected"][0]] != vals[info["members_roots"][0]]
    assert not np.array_equal(m["public"][-1], good["public"][-1])


TIE_CENTROIDS = [[10, 20, 30, 40], [14, 20, 30, 40], [100, 100, 100, 100]]
TIE_QUERY = [12, 20, 30, 40]


def test_values_model_of_the_rounds_is_the_circuits_and_the_tie_case(O):
    """ann_probe_model.rounds_fold against the last set indicator of every round of topk_model, on a database with exact ties and on the
    tie case: two centroids tied nearest leave in round 0, which states the later one; round 1 states the third"""
    import ann_assign_model as AS
    from test_ann_assign_cpu import pool
    queries, vectors = pool(21, 3, 48)
    qq, qv = O.quantize(queries, P), O.quantize(vectors, P)
    idx, _ = PM.rounds_fold(AS.distance_table(O, "euclidean", qq, qv, P, L), 5, P)
    for j in range(3):
        assert PM.centroid_rounds(O, "euclidean", qq[j], qv, 5, P, L) == idx[j].tolist(), j
    cent, query = O.quantize(np.asarray(TIE_CENTROIDS, dtype=np.float64), P), O.quantize(np.asarray(TIE_QUERY, dtype=np.float64), P)
    a = TM.topk_model(O, "euclidean", query[None], cent, 2, P, L, inputs=False)
    assert a["indicator_bits"][0].tolist() == [[1, 1, 0], [0, 0, 1]]
    assert PM.rounds_fold(AS.distance_table(O, "euclidean", query[None], cent, P, L), 2, P)[0].tolist() == [[1, 2]]
    assert PM.rounds_fold(AS.distance_table(O, "euclidean", query[None], cent[:2], P, L), 2, P)[0].tolist() == [[1, 1]]    # nothing left: K - 1 again
