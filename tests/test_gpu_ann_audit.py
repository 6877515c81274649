"""The audit of one cluster's routing on the GPU (pipeline.AnnAuditHotPath; vdb_wit_ann_audit*): the streams are tests/ann_audit_model.py's bit
for bit (tests/test_ann_audit_cpu.py holds that model against the host-built map first); host and device forms, the launch list, refused
arguments, rank windows cut inside the blocks, the kernels' bytes against the map, the device-placed map, the proof, a misrouted member
on the device, an update followed by an audit of the index it leaves, and the alteration sweep."""
import ctypes

import numpy as np
import pytest

import ann_audit_model as AA
import topk_model as TM
from test_ann_audit_cpu import CASES, DIM, L, P, case
from test_gpu_batch_query import _dev
from test_gpu_rounds import TAU
from test_gpu_sweep import _check_window, _windowed

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def api():
    from halo2_vectordb_amd import api as a
    a.init(0)
    return a


def _index(K, n_c, c, metric="euclidean", seed=60, foreign=None):
    """the resident index of a case: cluster c holds the recipe's members, every other cluster one row, its own centroid; `foreign`: the
    slot of cluster c that holds a row next to centroid 0 instead -> (AnnIndex, f64 members)"""
    from halo2_vectordb_amd.pipeline import AnnIndex
    cent, mem = AA.data(seed, K, n_c, c)
    if foreign is not None:
        mem[foreign] = np.clip(cent[0] + np.random.default_rng(7).integers(-3, 4, DIM), 0, 218)
    rows = np.concatenate([mem if j == c else cent[j:j + 1] for j in range(K)])
    ids = np.concatenate([np.full(n_c if j == c else 1, j) for j in range(K)])
    return AnnIndex(rows.shape[0], DIM, K, rows, ids, cent, P=P, L=L, metric=metric), mem


def _hot_path(K, n_c, c, metric="euclidean", k=13, **kw):
    from halo2_vectordb_amd.pipeline import AnnAuditHotPath
    foreign = kw.pop("foreign", None)
    index, _ = _index(K, n_c, c, metric, foreign=foreign)
    return index, AnnAuditHotPath(index, c, k=k, P=P, L=L, metric=metric, tau=TAU, **kw)


@pytest.mark.parametrize("metric,K,n_c,c", CASES)
def test_host_witness_is_the_models(api, O, metric, K, n_c, c):
    m, cent, mem, roots, index_root = case(O, metric, K, n_c, c)
    got = api.wit_ann_audit(metric, cent, mem, roots, c, P, L, selectors=True)
    assert got["n_in"] == m["n_in"] == K + 2 and got["stream"].shape == m["advice"].shape
    bad = np.flatnonzero((got["stream"] != m["advice"]).any(axis=1))
    assert bad.size == 0, f"first differing advice cells {bad[:5]} of {got['stream'].shape[0]} (blocks {m['regions']}, per member {m['per_member']})"
    assert np.array_equal(got["lookup"], m["lookup"]) and np.array_equal(got["selectors"], m["selectors"])
    # the flag bytes beyond the gate bit: outside the distance and qmin blocks (of whose constants the oracle keeps none) the model's;
    # every member's K distance blocks are those of vdb_wit_distance emitted alone
    gen = m["generator"]
    assert np.array_equal(got["flags"][~gen], m["flags"][~gen])
    r = m["regions"]
    for i in (0, n_c - 1):
        alone = api.wit_distance(metric, cent, np.repeat(mem[i:i + 1], K, axis=0), P, L, selectors=True)
        lo = r["routed"] + i * m["per_member"]
        assert np.array_equal(got["flags"][lo:lo + m["chain_off"]], alone["flags"]) and np.array_equal(got["stream"][lo:lo + m["chain_off"]], alone["stream"])
    assert np.array_equal(got["routed"], m["routed"]) and got["routed"].all()
    assert np.array_equal(got["public"], m["public"]) and np.array_equal(got["public"][0], index_root)


@pytest.mark.parametrize("K,n_c,c", [(3, 5, 2), (5, 70, 3)])
def test_device_form_on_a_resident_index_is_the_host_form(api, O, K, n_c, c):
    m, cent, mem, roots, index_root = case(O, "euclidean", K, n_c, c)
    index, hp = _hot_path(K, n_c, c)
    try:
        assert np.array_equal(index.roots()[:K + 1], roots) and np.array_equal(index.members(c), mem)
        hp.setup()
        assert hp.resident and (hp.n_cells, hp.n_in, hp.n_lookup) == (m["advice"].shape[0], K + 2, m["lookup"].shape[0])
        d_flags = hp.keygen_flags()
        host = api.wit_ann_audit("euclidean", cent, mem, roots, c, P, L, selectors=True)
        assert np.array_equal(d_flags.download((hp.n_cells,), dtype=np.uint8), host["flags"])
        d_flags.free()
        hp._witness()
        api.sync()
        assert np.array_equal(hp.d_stream.download((hp.n_cells, 4)), host["stream"]) and np.array_equal(hp.d_lookup.download((hp.n_lookup, 4)), host["lookup"])
        root, c_fr, routed = hp.results()
        assert np.array_equal(root, index_root) and TM.to_ints(c_fr[None]) == [c] and routed.tolist() == [1] * n_c
    finally:
        hp.free()
        index.free()


def test_launch_list_depends_on_neither_K_nor_the_cluster_size_and_refused_arguments_launch_nothing(api, O):
    from halo2_vectordb_amd import circuit_sym as CS
    from halo2_vectordb_amd._lib import check
    counts = {}
    for K, n_c, c in ((2, 2, 1), (5, 70, 3)):
        index, hp = _hot_path(K, n_c, c)
        try:
            hp.setup()
            hp._witness()
            api.sync()
            api.profile_begin(deferred=True)
            hp._witness()
            api.sync()
            counts[K] = {kern: int(v["launches"]) for kern, v in api.profile_end().items()}
            lib = hp.lib
            d_out = api.DeviceBuffer(1 << 16)
            check(lib.vdb_memset_dev(d_out.ptr, 0xA5, ctypes.c_size_t(1 << 16)))
            api.sync()
            api.profile_begin(deferred=True)

            def call(K_=K, c_=c, n_c_=n_c, dim=DIM, lc=None, lm=None):
                return lib.vdb_wit_ann_audit_dev(hp.metric, P, L, hp.p_cent, hp.p_members, index.d_roots.ptr, lc, lm, K_, c_, n_c_, dim, d_out.ptr,
                                                 d_out.at(1 << 14), None, d_out.at(1 << 15), d_out.at(3 << 14))
            big = 1 << 24
            # the frame's refusals, the audit's own, the instance limits, the cell limit (a circuit whose instance counts pass: held
            # against the layout first), one resident tree without the other
            huge = dict(n_c_=1 << 16, dim=256)
            lay = CS.ann_audit_layout("euclidean", K, huge["n_c_"], huge["dim"], P, L)
            assert lay["total"] > 1 << 34 and huge["n_c_"] * K <= big and huge["n_c_"] * huge["dim"] <= big
            sized = [dict(K_=0), dict(K_=4097), dict(n_c_=big + 1), dict(n_c_=0), dict(dim=0), dict(dim=(1 << 20) + 1), dict(n_c_=big // K + 1),
                     dict(n_c_=big // 8 + 1, dim=8), huge]
            for kw in sized:                                        # the size call first: it shares the layout and writes nothing
                cells = ctypes.c_uint64()
                assert lib.vdb_wit_ann_audit_size(hp.metric, P, L, kw.get("K_", K), kw.get("n_c_", n_c), kw.get("dim", DIM), ctypes.byref(cells), None, None) == -3, kw
            for kw in sized + [dict(c_=K), dict(lc=index.levels_ptr(K)), dict(lm=index.levels_ptr(c))]:
                with pytest.raises(api.VdbError) as e:
                    check(call(**kw))
                assert e.value.code == -3, kw
            api.sync()
            assert api.profile_end() == {}
            assert (d_out.download((1 << 16,), dtype=np.uint8) == 0xA5).all()
            d_out.free()
        finally:
            hp.free()
            index.free()
    assert counts[2] == counts[5] and counts[2]["k_anna_pick"] == 1 and counts[2]["k_nv_qmin"] == 1 and counts[2]["k_inv_fixup"] == 1, counts
    assert counts[2]["k_mk_leaf_trace"] == 3 and counts[2]["k_mk_tree_trace"] == 2 and counts[2]["k_mku_inputs"] == 1, counts
    assert "k_annu_new_roots" not in counts[2] and "k_nv_is_equal" not in counts[2], counts


def test_launch_count_is_the_same_at_K_one(api, O):
    """the qmin chain is launched at K = 1 too, where it has no lane"""
    index, hp = _hot_path(1, 1, 0)
    try:
        hp.setup()
        hp._witness()
        api.sync()
        api.profile_begin(deferred=True)
        hp._witness()
        api.sync()
        got = {kern: int(v["launches"]) for kern, v in api.profile_end().items()}
        assert got["k_nv_qmin"] == 1 and got["k_anna_pick"] == 1, got
    finally:
        hp.free()
        index.free()


def test_two_windowed_calls_write_the_bytes_of_one(api, O):
    from halo2_vectordb_amd._lib import check
    lib = api.init()
    K, n_c, c = 3, 5, 2
    m, cent, mem, roots, _ = case(O, "euclidean", K, n_c, c)
    want, lk, r = m["advice"], m["lookup"], m["regions"]
    cells, per, per_l = want.shape[0], m["per_member"], m["per_member_l"]
    from halo2_vectordb_amd import circuit_sym as CS
    lay = CS.ann_audit_layout("euclidean", K, n_c, DIM, P, L)
    d_lk = lay["units"]["db"].n_lk
    up = []
    try:
        d_cent, d_mem, d_roots = _dev(api, up, cent), _dev(api, up, mem), _dev(api, up, roots)
        d_routed, d_pub = api.DeviceBuffer(32), api.DeviceBuffer(64)
        up += [d_routed, d_pub]
        run = lambda d_adv, d_lkb: check(lib.vdb_wit_ann_audit_dev(0, P, L, d_cent.ptr, d_mem.ptr, d_roots.ptr, None, None, K, c, n_c, DIM, d_adv.ptr, d_lkb.ptr,
                                                                  None, d_routed.ptr, d_pub.ptr))
        m1 = r["routed"] + per                                  # member 1's sub-block
        # inside the header; inside an indicator; between member 1's last distance and its chain (the lookup cut between the distance
        # runs and the qmin runs); inside a pick block; inside MC; inside the assigned members
        cuts = [(2, 0), (r["indicator"] + 8 + 5, 0), (m1 + m["chain_off"], per_l + K * d_lk), (m1 + m["pick_off"] + 5, 2 * per_l),
                (r["merkle_c"] + 1000, len(lk)), (r["members"] + 3, 0)]
        # the seams of the cluster frame the audits share: where the head ends, between the centroids and the members (inside the one
        # launch that assigns both), where MC and MM start, one cell into MM
        cuts += [(r["centroids"], 0), (r["members"], 0), (r["merkle_c"], len(lk)), (r["merkle_m"], len(lk)), (r["merkle_m"] + 1, len(lk))]
        for cut, lcut in cuts:
            halves = []
            for window in ((0, cut, 0, lcut), (cut, cells, lcut, len(lk))):
                g_adv, g_lk = _windowed(api, lib, check, want, lk, window, run)
                _check_window(want, lk, g_adv, g_lk, window, (cut, window))
                assert np.array_equal(d_pub.download((2, 4)), m["public"]), (cut, window)
                assert d_routed.download((n_c,), dtype=np.uint8).tolist() == [1] * n_c, (cut, window)
                halves.append((g_adv, g_lk))
            assert np.array_equal(np.concatenate([halves[0][0][:cut], halves[1][0][cut:]]), want), cut
            assert np.array_equal(np.concatenate([halves[0][1][:lcut], halves[1][1][lcut:]]), lk), cut
    finally:
        for b in up:
            b.free()


def test_kernels_witness_and_flags_satisfy_the_map(api, O):
    from halo2_vectordb_amd import circuit_sym as CS
    from test_merkle_update_cpu import fetchers
    K, n_c, c = 3, 5, 2
    m, cent, mem, roots, _ = case(O, "euclidean", K, n_c, c)
    got = api.wit_ann_audit("euclidean", cent, mem, roots, c, P, L, selectors=True)
    ff, fv, vals = fetchers(dict(advice=got["stream"], flags=got["flags"]))
    cm, public, info = CS.build_ann_audit("euclidean", K, n_c, DIM, P, L, ff, fv)
    rep = cm.check_witness(vals, TM.to_ints(got["lookup"]), got["flags"])
    assert not any(rep.values()), rep
    assert [vals[x] for x in public] == TM.to_ints(got["public"])
    assert [int(cm.copy_of[x]) for x in info["own"]] == info["m"] and cm.copy_of[info["members_root"]] == info["picked"]


@pytest.mark.parametrize("K,n_c,c", [(1, 1, 0), (3, 5, 0), (3, 5, 2)])
def test_device_placed_map_is_the_host_builders(api, O, K, n_c, c):
    from halo2_vectordb_amd.rounds import ProverRounds
    index, hp = _hot_path(K, n_c, c)
    maps = {}
    try:
        hp.setup()
        for on_dev in (True, False):
            pr = ProverRounds(hp)
            pr.map_on_device = on_dev
            d_flags = hp.keygen_flags()
            cm = pr.circuit_map(d_flags)
            d_flags.free()
            maps[on_dev] = (np.array(cm.copy_of), np.array(cm.const_idx), np.asarray(cm.gate).copy(), [int(v) for v in cm.consts], np.array(cm.lookup_src),
                            np.array(cm.asserted), pr.public_cells)
            if on_dev:
                cm.free()
        d, h = maps[True], maps[False]
        assert d[6] == h[6] and len(h[6]) == 2
        for i in (0, 2, 4, 5):
            assert np.array_equal(d[i], h[i]), i
        val = lambda x: np.where(x[1] >= 0, np.asarray(x[3] + [0], dtype=object)[np.maximum(x[1], -1)], -1)
        assert np.array_equal(val(d), val(h))
    finally:
        hp.free()
        index.free()


def test_proof_is_accepted_and_bound_to_the_index_root_and_the_cluster(api, O):
    from halo2_vectordb_amd import verifier
    from halo2_vectordb_amd.rounds import ProverRounds
    K, n_c, c = 3, 5, 2
    m, _, _, _, index_root = case(O, "euclidean", K, n_c, c)
    index, hp = _hot_path(K, n_c, c, k=13)                     # the smallest k that holds the 2^12-entry table: several columns
    pr = None
    try:
        pr = ProverRounds(hp.setup()).keygen()
        assert hp.n_adv_cols >= 3, hp.n_adv_cols
        assert pr.keygen_report.violations() == 0, pr.keygen_report.as_dict()
        out = pr.prove(None, seed=29)
        want = TM.to_ints(m["public"])
        assert out["instances"] == want and want == [TM.to_ints(index_root[None])[0], c]
        vk = verifier.VerifyingKey.from_prover(pr, out["opened"])
        assert verifier.verify(out["proof"], want, vk)
        for i in range(2):
            wrong = list(want)
            wrong[i] = (wrong[i] + 1) % O.R_MOD
            assert not verifier.verify(out["proof"], wrong, vk), i
    finally:
        if pr is not None:
            pr.free()
        hp.free()
        index.free()


def test_a_misrouted_member_is_flagged_and_fails_the_mock_report(api, O):
    """a failing Mock report, not a fault: the call succeeds on an index with one foreign row in cluster c"""
    from halo2_vectordb_amd import circuit_sym as CS
    from halo2_vectordb_amd.rounds import ProverRounds
    K, n_c, c, bad = 3, 5, 2, 3
    index, hp = _hot_path(K, n_c, c, foreign=bad)
    pr = None
    try:
        pr = ProverRounds(hp.setup()).keygen()
        assert hp.results()[2].tolist() == [1, 1, 1, 0, 1]
        rep = pr.keygen_report
        lay = CS.ann_audit_layout("euclidean", K, n_c, DIM, P, L)
        own_bad = lay["routed"] + (bad + 1) * lay["per_member"] - 1
        assert rep.violations() == 1 and rep.copies_unequal == 1 and rep.first_copy == own_bad, rep.as_dict()
    finally:
        if pr is not None:
            pr.free()
        hp.free()
        index.free()


def test_an_update_into_the_assigned_cluster_then_an_audit_of_the_index_it_leaves(api, O):
    from halo2_vectordb_amd import verifier
    from halo2_vectordb_amd.pipeline import AnnAuditHotPath, AnnUpdateHotPath
    from halo2_vectordb_amd.rounds import ProverRounds
    K, n_c, c = 3, 5, 2
    index, mem = _index(K, n_c, c)
    made, pr = [index], None
    try:
        cent, _ = AA.data(60, K, n_c, c)
        row = np.clip(cent[c] + np.asarray([1, -2, 2, -1]), 0, 218).astype(np.float64)
        assert index.assign(row[None]).tolist() == [c]
        au = AnnUpdateHotPath(index, c, ([n_c], row[None]), grow=None, k=13, tau=TAU).setup()
        made.append(au)
        au._witness()
        api.sync()
        ix2 = index.updated(au)
        made.append(ix2)
        hp = AnnAuditHotPath(ix2, c, k=13, P=P, L=L, tau=TAU).setup()
        made.append(hp)
        assert hp.n == n_c + 1
        pr = ProverRounds(hp).keygen()
        assert pr.keygen_report.violations() == 0, pr.keygen_report.as_dict()
        root, c_fr, routed = hp.results()
        assert np.array_equal(root, au.results()[5]) and routed.tolist() == [1] * (n_c + 1)
        out = pr.prove(None, seed=31)
        assert out["instances"] == TM.to_ints(np.stack([root, c_fr]))
        assert verifier.verify(out["proof"], out["instances"], verifier.VerifyingKey.from_prover(pr, out["opened"]))
    finally:
        if pr is not None:
            pr.free()
        for x in reversed(made):
            x.free()


def test_single_cell_alteration_sweep(api, O):
    """tests/alteration_model.py's method by the device sweep of tests/test_gpu_alteration.py at (K 2, n_c 2, c 1): the map as the device
    placed it and the bytes the kernels wrote; a cell may stay free only by a rule of alteration_model.explain"""
    from test_gpu_alteration import device_sweep
    index, hp = _hot_path(2, 2, 1)
    try:
        device_sweep(api, O, f"ann audit euclidean K 2 n_c 2 c 1 dim {DIM}", hp.setup())       # frees the hot path
    finally:
        index.free()
