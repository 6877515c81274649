"""The query over the p nearest clusters on the GPU (pipeline.AnnProbeQueryHotPath, AnnIndex.probe_many; vdb_wit_ann_probe*,
vdb_nearest_topk_values*): the witness streams are tests/ann_probe_model.py's bit for bit (tests/test_ann_probe_cpu.py holds that model
against the single-probe model and the map first) and vdb_wit_ann_query's at p = t = 1; the hot path with a resident forest, its
neighbours, the proof, the device-built map, the binding of every probed cluster to its round, launch counts, refused arguments, and the
values-only round winners against the model's."""
import ctypes

import numpy as np
import pytest

import ann_assign_model as AS
import ann_model as AN
import ann_probe_model as PM
import topk_model as TM
from ann_probe_model import DIM, L, P
from test_ann_probe_cpu import TIE_CENTROIDS, TIE_QUERY
from test_gpu_rounds import TAU

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def api():
    from halo2_vectordb_amd import api as a
    a.init(0)
    return a


def _padded(n):
    return (1 << (n - 1).bit_length()) > n


@pytest.mark.parametrize("name", list(PM.CASES))
def test_host_witness_is_the_models(api, O, name):
    c, m = PM.case(O, name), PM.case_model(O, name)
    got = api.wit_ann_probe("euclidean", c["query"], c["cent"], c["members"], c["roots"], c["t"], P, L, selectors=True)
    assert got["n_in"] == m["n_in"] and got["stream"].shape == m["advice"].shape
    assert np.array_equal(got["stream"], m["advice"]) and np.array_equal(got["lookup"], m["lookup"])
    assert np.array_equal(got["selectors"], m["selectors"])
    # the flag bytes beyond the gate bit, of which the oracle keeps none, are the generators': every block's are those of the block
    # emitted alone (a members' tree copies the zero cell where an earlier tree has loaded it); the assigned inputs and the selections
    # hold no constant cell
    r, K, p, t, block = m["regions"], c["K"], c["p"], c["t"], np.zeros(got["flags"].shape[0], dtype=bool)
    cand = np.concatenate(c["members"])
    words = np.concatenate([c["ix"]["roots"][:1], c["roots"]])[None]
    alone = [(r["nearest_c"], r["merkle_c"], api.wit_nearest_topk("euclidean", c["query"][None], c["cent"], p, P, L, selectors=True)),
             (r["merkle_c"], r["nearest_m"], api.wit_merkle(c["cent"], selectors=True)),
             (r["nearest_m"], r["merkle_m"][0], api.wit_nearest_topk("euclidean", c["query"][None], cand, t, P, L, selectors=True)),
             (r["sponge"], got["flags"].shape[0], api.wit_merkle(words, selectors=True))]
    zero = _padded(K)
    for j, mem in enumerate(c["members"]):
        alone.append((r["merkle_m"][j], r["merkle_m"][j + 1] if j + 1 < p else r["select"][0], api.wit_merkle(mem, zero_cached=zero, selectors=True)))
        zero = zero or _padded(len(mem))
    for lo, hi, a in alone:
        assert np.array_equal(got["flags"][lo:hi], a["flags"]) and np.array_equal(got["stream"][lo:hi], a["stream"]), lo
        block[lo:hi] = True
    assert np.array_equal(got["flags"][~block], m["selectors"][~block])
    assert np.array_equal(got["centroid_indicators"], m["centroid_indicators"]) and np.array_equal(got["candidate_indicators"], m["candidate_indicators"])
    assert np.array_equal(got["results"], m["results"])
    assert np.array_equal(got["public"], m["public"]) and np.array_equal(got["index_root"], c["ix"]["roots"][-1])


@pytest.mark.parametrize("name", ["1-4-7", "1-1", "wave"])
def test_one_probe_one_neighbour_is_the_single_probe_call(api, O, name):
    c = PM.case(O, name)
    one = api.wit_ann_query("euclidean", c["query"], c["cent"], c["members"][0], c["roots"], P, L, selectors=True)
    got = api.wit_ann_probe("euclidean", c["query"], c["cent"], c["members"][:1], c["roots"], 1, P, L, selectors=True)
    for key in ("stream", "lookup", "flags", "selectors", "public"):
        assert got[key].tobytes() == one[key].tobytes(), key
    assert got["n_in"] == one["n_in"]
    assert np.array_equal(got["centroid_indicators"][0], one["centroid_indicator"]) and np.array_equal(got["candidate_indicators"][0], one["member_indicator"])


def _hot_path(O, name, k=13, **kw):
    from halo2_vectordb_amd.pipeline import AnnIndex, AnnProbeQueryHotPath
    c = PM.case(O, name)
    index = AnnIndex(c["n"], DIM, c["K"], c["f"]["db"], c["ids"], c["f"]["cent"], P=P, L=L)
    try:
        return index, AnnProbeQueryHotPath(index, c["f"]["query"], probes=kw.pop("probes", c["p"]), topk=kw.pop("topk", c["t"]), k=k, P=P, L=L, tau=TAU, **kw)
    except Exception:
        index.free()
        raise


def test_hot_path_is_the_model_split_windows_and_neighbours(api, O):
    from halo2_vectordb_amd._lib import check
    c, m = PM.case(O, "1-4-7"), PM.case_model(O, "1-4-7", plan_k=13)
    index, hp = _hot_path(O, "1-4-7")
    try:
        assert hp.clusters == c["rounds"] and hp.sizes.tolist() == c["sizes"]
        hp.setup()
        assert hp.resident and hp.n_cells == m["advice"].shape[0] and hp.n_in == m["n_in"] and hp.n_lookup == m["lookup"].shape[0]
        assert np.array_equal(hp.bp, m["break_points"])
        d_flags = hp.keygen_flags()
        assert np.array_equal(d_flags.download((hp.n_cells,), dtype=np.uint8) & 1, m["selectors"])
        d_flags.free()
        hp._witness()
        api.sync()
        assert np.array_equal(hp.d_stream.download((hp.n_cells, 4)), m["advice"]) and np.array_equal(hp.d_lookup.download((hp.n_lookup, 4)), m["lookup"])
        ind_c, ind_m, res, root = hp.results()
        assert np.array_equal(ind_c, m["centroid_indicators"]) and np.array_equal(ind_m, m["candidate_indicators"])
        assert np.array_equal(res, m["results"]) and np.array_equal(root, c["ix"]["roots"][-1])
        # the database slots of the results: a brute-force ranking of the candidates by the model's distances
        cand_slots = np.concatenate([AN.select_cluster(c["db"], c["ids"], w)[1] for w in c["rounds"]])
        cand = np.concatenate(c["members"])
        d = [AS.signed(x, P) for x in TM.to_ints(AS.distance_table(O, "euclidean", c["query"][None], cand, P, L)[0])]
        want = cand_slots[np.argsort(np.asarray(d, dtype=object), kind="stable")[:c["t"]]]
        assert hp.neighbours().tolist() == want.tolist()
        assert np.array_equal(c["db"][hp.neighbours()], res)
        # a two-way window split reproduces the unsplit stream
        lib, cut, lcut = hp.lib, hp.n_cells // 2 + 3, hp.n_lookup // 2 + 1
        check(lib.vdb_memset_dev(hp.d_stream.ptr, 0xA5, ctypes.c_size_t(hp.n_cells * 32)))
        check(lib.vdb_memset_dev(hp.d_lookup.ptr, 0xA5, ctypes.c_size_t(hp.n_lookup * 32)))
        for adv, lk in (((0, cut), (0, lcut)), ((cut, hp.n_cells), (lcut, hp.n_lookup))):
            with api.wit_window(adv=adv, lookup=lk):
                hp._witness()
        api.sync()
        assert np.array_equal(hp.d_stream.download((hp.n_cells, 4)), m["advice"]) and np.array_equal(hp.d_lookup.download((hp.n_lookup, 4)), m["lookup"])
    finally:
        hp.free()
        index.free()


def test_proof_is_accepted_and_bound_to_the_index_root(api, O):
    from halo2_vectordb_amd import verifier
    from halo2_vectordb_amd.rounds import ProverRounds
    c, m = PM.case(O, "1-4-7"), PM.case_model(O, "1-4-7")
    index, hp = _hot_path(O, "1-4-7")
    pr = None
    try:
        pr = ProverRounds(hp.setup()).keygen()
        assert pr.keygen_report.violations() == 0, pr.keygen_report.as_dict()
        out = pr.prove(None, seed=17)
        want = TM.to_ints(m["public"])
        assert out["instances"] == want and len(want) == c["t"] * DIM + 1
        vk = verifier.VerifyingKey.from_prover(pr, out["opened"])
        assert verifier.verify(out["proof"], want, vk)
        wrong = list(want)
        wrong[-1] = (wrong[-1] + 1) % O.R_MOD
        assert not verifier.verify(out["proof"], wrong, vk)
        wrong = list(want)
        wrong[0] = (wrong[0] + 1) % O.R_MOD
        assert not verifier.verify(out["proof"], wrong, vk)
    finally:
        if pr is not None:
            pr.free()
        hp.free()
        index.free()


@pytest.mark.parametrize("name", ["1-4-7", "zero-chain"])
def test_device_built_map_is_the_host_built_map(api, O, name):
    index, hp = _hot_path(O, name)
    dev = None
    try:
        hp.setup()
        d_flags = hp.keygen_flags()
        hp._witness()
        api.sync()
        host, pub_h, _ = hp.constraint_map(d_flags, on_device=False)
        dev, pub_d, _ = hp.constraint_map(d_flags, on_device=True)
        d_flags.free()
        assert pub_h == pub_d and dev.n_cells == host.n_cells and dev.consts == host.consts
        for field in ("copy_of", "const_idx", "gate", "asserted", "lookup_src"):
            assert np.array_equal(getattr(dev, field), getattr(host, field)), field
    finally:
        if dev is not None:
            dev.free()
        hp.free()
        index.free()


def test_wrong_cluster_order_and_altered_root_are_noticed(api, O):
    """the binding: the two probed clusters against round order break both sel_r = mroot_r copies, an altered cluster root breaks its
    own; the witness call itself succeeds on either"""
    from halo2_vectordb_amd import circuit_sym as CS
    from halo2_vectordb_amd.pipeline import AnnIndex, AnnProbeQueryHotPath
    from halo2_vectordb_amd.rounds import ProverRounds
    c = PM.case(O, "1-4-7")
    index = AnnIndex(c["n"], DIM, c["K"], c["f"]["db"], c["ids"], c["f"]["cent"], P=P, L=L)
    roots = index.roots()[1:1 + c["K"]].copy()
    roots[c["rounds"][1]] = O.fr_add(roots[c["rounds"][1]:c["rounds"][1] + 1], O.fr_from_ints([1]))[0]
    try:
        assert index.probe_many(c["f"]["query"], 2).tolist() == c["rounds"]
        for kw, sizes, broken in ((dict(clusters=c["rounds"][::-1]), c["sizes"][::-1], [0, 1]), (dict(cluster_roots=roots), c["sizes"], [1])):
            hp = AnnProbeQueryHotPath(index, c["f"]["query"], probes=2, topk=3, k=13, P=P, L=L, tau=TAU, **kw).setup()
            pr = ProverRounds(hp).keygen()
            try:
                rep = pr.keygen_report
                lay = CS.ann_probe_layout("euclidean", c["K"], sizes, DIM, 2, 3, P, L)
                selected = [lay["select"][r] + 3 * c["K"] for r in broken]
                assert rep.copies_unequal == len(broken) and rep.first_copy == selected[0], (list(kw), rep.as_dict())
                if "cluster_roots" in kw:
                    assert not np.array_equal(hp.results()[3], index.roots()[-1])
            finally:
                pr.free()
                hp.free()
    finally:
        index.free()


def _dev_call(hp, index, **over):
    """the arguments of the hot path's own vdb_wit_ann_probe_dev call, some replaced"""
    a = dict(metric=hp.metric, query=hp.d_vec.ptr, cent=hp.p_cent, members=hp.p_members, roots=hp.p_roots, levels_c=index.levels_ptr(hp.K),
             levels_m=hp.p_levels, K=hp.K, dim=DIM, p=hp.probes, sizes=hp.sizes, t=hp.topk)
    a.update(over)
    sizes = None if a["sizes"] is None else np.ascontiguousarray(a["sizes"], dtype=np.uint64)
    return hp.lib.vdb_wit_ann_probe_dev(a["metric"], P, L, a["query"], a["cent"], a["members"], a["roots"], a["levels_c"], a["levels_m"], a["K"], a["dim"],
                                        a["p"], None if sizes is None else sizes.ctypes.data_as(ctypes.c_void_p), a["t"], hp.d_stream.ptr,
                                        hp.d_lookup.ptr, None, hp.d_ind_c.ptr, hp.d_ind_m.ptr, hp.d_pub.ptr)


def test_launch_count_depends_on_neither_K_the_cluster_sizes_nor_topk_and_refused_arguments_launch_nothing(api, O):
    """with every tree read from the forest the witness call launches the same kernels the same number of times at K 3, sizes (7, 1) and
    at K 5, sizes (65, 1), and at t = 1 and t = 3; every refused argument is refused before anything is launched"""
    from halo2_vectordb_amd._lib import check
    counts = {}
    for name, t in (("1-4-7", 3), ("1-4-7", 1), ("wave", 3)):
        index, hp = _hot_path(O, name, topk=t)
        try:
            hp.setup()
            hp._witness()
            api.sync()
            api.profile_begin(deferred=True)
            hp._witness()
            api.sync()
            counts[name, t] = (hp.K, hp.sizes.tolist(), {kern: int(v["launches"]) for kern, v in api.profile_end().items()})
            if (name, t) != ("1-4-7", 3):
                continue
            api.profile_begin(deferred=True)
            one_null = (ctypes.c_void_p * 2)(hp.p_levels[0], None)
            four = lambda ptrs: (ctypes.c_void_p * 4)(ptrs[0], ptrs[1], ptrs[0], ptrs[1])      # (the call reads p entries of either array)
            refused = [dict(levels_c=None), dict(levels_m=None), dict(levels_m=one_null),            # the resident trees: all or none
                       dict(p=0, sizes=[]), dict(p=hp.K + 1, sizes=[7, 1, 7, 1], members=four(hp.p_members), levels_m=four(hp.p_levels)),      # 1 <= p <= K
                       dict(p=17, K=32, sizes=[1] * 17),                                              # p <= VDB_ANN_PROBE_MAX
                       dict(t=0), dict(t=9),                                                          # 1 <= t <= N
                       dict(sizes=[7, 0]), dict(sizes=[1 << 24, 1]),                                  # an empty cluster, N above VDB_ANN_MAX_VECTORS
                       dict(sizes=[1 << 23, 1], t=3), dict(dim=1 << 21), dict(dim=0), dict(K=0), dict(K=4097),     # nv_fits, dim, K
                       dict(metric=9), dict(query=None), dict(sizes=None)]
            for over in refused:
                with pytest.raises(api.VdbError) as e:
                    check(_dev_call(hp, index, **over))
                assert e.value.code == -3, over
                assert str(e.value).strip() != "vdb error -3:", over           # each with its own text
            api.sync()
            assert api.profile_end() == {}
        finally:
            hp.free()
            index.free()
    (K0, s0, c0), (_, _, c1), (K2, s2, c2) = counts["1-4-7", 3], counts["1-4-7", 1], counts["wave", 3]
    assert (K0, s0, K2, s2) == (3, [7, 1], 5, [65, 1]) and c0 == c1 == c2 and c0["k_annp_gather"] == 1 and c0["k_mk_tree_trace"] == 3, counts


VALUE_QS, VALUE_NS = (1, 3), (1, 2, 63, 64, 65, 130)


@pytest.fixture(scope="module")
def tables(O):
    """per metric: 3 quantized queries, 130 vectors (the longer databases hold exact ties) and the model's 3 x 130 distances, computed
    once; a case over Q queries and n vectors is the table's corner [:Q, :n]"""
    from test_ann_assign_cpu import METRICS, pool
    queries, vectors = pool(21, max(VALUE_QS), max(VALUE_NS))
    qq, qv = O.quantize(queries, P), O.quantize(vectors, P)
    return {m: (qq, qv, AS.distance_table(O, m, qq, qv, P, L)) for m in METRICS}


@pytest.mark.parametrize("metric", ("euclidean", "cosine", "manhattan", "hamming"))
def test_round_winners_as_values_are_the_models(api, tables, metric):
    qq, qv, table = tables[metric]
    tied = 0
    for Q in VALUE_QS:
        for n in VALUE_NS:
            for p in sorted({1, min(n, 2), min(n, 5)}):
                want_idx, want_dist = PM.rounds_fold(table[:Q, :n], p, P)
                idx, dist = api.nearest_topk_values(metric, qq[:Q], qv[:n], p, P, L)
                assert np.array_equal(idx, want_idx), (Q, n, p, idx, want_idx)
                assert np.array_equal(dist, want_dist), (Q, n, p)
                tied += sum(sum(np.array_equal(table[j, i], want_dist[j, 0]) for i in range(n)) > 1 for j in range(Q))
            one_idx, one_dist = api.nearest_values(metric, qq[:Q], qv[:n], P, L)
            assert np.array_equal(idx[:, 0], one_idx) and np.array_equal(dist[:, 0], one_dist)
    assert tied > 0                                          # the repeats of the longer databases tie: the last of a round's winners was in question


def test_tie_case_probe_many_and_the_refused_query(api, O):
    """two centroids tied nearest leave in round 0, which states the later one, and round 1 states the third: probe_many gives [1, 2];
    over the first two centroids alone the second round has nothing left and states centroid 1 again, which the hot path refuses"""
    from halo2_vectordb_amd.pipeline import AnnIndex, AnnProbeQueryHotPath
    cent, query = np.asarray(TIE_CENTROIDS, dtype=np.float64), np.asarray(TIE_QUERY, dtype=np.float64)
    db = np.random.default_rng(40).integers(0, 219, size=(6, DIM)).astype(np.float64)
    qc, qq = O.quantize(cent, P), O.quantize(query, P)
    a = TM.topk_model(O, "euclidean", qq[None], qc, 2, P, L, inputs=False)
    assert a["indicator_bits"][0].tolist() == [[1, 1, 0], [0, 0, 1]]
    idx, _ = api.nearest_topk_values("euclidean", qq[None], qc, 2, P, L)
    assert idx.tolist() == [[1, 2]]
    index = AnnIndex(6, DIM, 3, db, [0, 1, 2, 0, 1, 2], cent, P=P, L=L)
    two = AnnIndex(6, DIM, 2, db, [0, 1, 0, 1, 0, 1], cent[:2], P=P, L=L)
    try:
        assert index.probe_many(query, 2).tolist() == [1, 2]
        assert index.probe_many(query, 1)[0] == index.probe(query) == 1
        assert two.probe_many(query, 2).tolist() == [1, 1]
        with pytest.raises(ValueError):
            AnnProbeQueryHotPath(two, query, probes=2, topk=1, k=13, P=P, L=L, tau=TAU)
        c = PM.case(O, "wave")
        wave = AnnIndex(c["n"], DIM, c["K"], c["f"]["db"], c["ids"], c["f"]["cent"], P=P, L=L)
        try:
            assert wave.probe_many(c["f"]["query"], 1)[0] == wave.probe(c["f"]["query"]) == c["rounds"][0]
            assert wave.probe_many(c["f"]["query"], 2).tolist() == c["rounds"]
        finally:
            wave.free()
    finally:
        index.free()
        two.free()
