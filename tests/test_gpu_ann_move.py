"""Moves proved against the committed index root on the GPU (pipeline.AnnMoveHotPath, AnnIndex.moved; vdb_wit_ann_move*,
vdb_ann_index_move_dev).  The streams are tests/ann_move_model.py's bit for bit (tests/test_ann_move_cpu.py holds that model against the
index, delete and update models first); host and device forms, rank windows cut at a carried cell of E_b, inside S, between F_a and B_b
and inside F_b, the launch list, refused arguments, the moved index against a fresh build over its own rows with every row's database
slot kept, a batch beyond one workgroup, the whole proof, changed instances, cells tampered in HBM, the binding of both trees to their
roots, a chain there and back, the other hot paths on the moved index, and the alteration and splice sweeps on the device map."""
import ctypes

import numpy as np
import pytest

import ann_delete_model as AD
import ann_model as AN
import ann_move_model as AV
import merkle_ops_model as MO
import merkle_update_model as MU
import topk_model as TM
from test_gpu_ann_delete import _resident
from test_gpu_batch_query import _dev
from test_gpu_rounds import TAU
from test_gpu_sweep import _check_window, _windowed

pytestmark = pytest.mark.gpu
P, L, DIM = 48, 12, 3


@pytest.fixture(scope="module")
def api():
    from halo2_vectordb_amd import api as a
    a.init(0)
    return a


def _rows(seed, n, dim):
    return np.random.default_rng(seed).integers(0, 219, size=(n, dim)).astype(np.float64)


_MODELS = {}


def _case(O, name, seed=70, slots=None, sizes=None, ab=None):
    """-> dict(f64 rows, quantized rows, the index model before the batch, the two trees before the batch (device layout, b's grown), the
    model and the trees after the batch); computed once per case and left unchanged"""
    key = (name, None if slots is None else tuple(slots), sizes, ab)
    if key not in _MODELS:
        sizes0, a, b, slots0 = AV.SHAPES[name]
        sizes, slots, (a, b) = sizes0 if sizes is None else sizes, slots0 if slots is None else slots, (a, b) if ab is None else ab
        ids = AD.ids_of(sizes)
        K = len(sizes)
        f = dict(db=_rows(seed, len(ids), DIM), cent=_rows(seed + 1, K, DIM))
        db, cent = O.quantize(f["db"], P), O.quantize(f["cent"], P)
        ix = AN.index_model(O, db, ids, cent)
        d_a, sh, d_b, g = AV.shape_of(sizes[a], sizes[b], len(slots))
        tree_a = MU.build_tree(O, AN.select_cluster(db, ids, a)[0])
        tree_b0 = MU.build_tree(O, AN.select_cluster(db, ids, b)[0])
        tree_b = MO.grow_tree(O, tree_b0, g)
        before = (MU.flat_levels(tree_a), MU.flat_levels(tree_b), MU.flat_levels(tree_b0))
        m = AV.move_model(O, ix["roots"][:K + 1], a, b, tree_a, tree_b, slots, plan_k=13)
        _MODELS[key] = dict(f=f, db=db, cent=cent, ids=ids, K=K, dim=DIM, a=a, b=b, slots=list(slots), ix=ix, before_a=before[0], before_b=before[1],
                            ungrown_b=before[2], m=m, tree_a=tree_a, tree_b=tree_b, n_a=int(sizes[a]), n_b=int(sizes[b]), shape=(d_a, sh, d_b, g))
    return _MODELS[key]


def _move_dev(api, s, levels_a=None, levels_b=None, profile=False):
    """vdb_wit_ann_move_dev into poisoned buffers -> (stream, flags, public, a's levels after, b's[, launches per kernel of a second run])"""
    from halo2_vectordb_amd._lib import check
    lib = api.init()
    m, K = len(s["slots"]), s["K"]
    u64 = ctypes.c_uint64
    cells, g = u64(), ctypes.c_uint()
    check(lib.vdb_wit_ann_move_size(K, s["n_a"], s["n_b"], m, ctypes.byref(cells), None, None, None, None, None, ctypes.byref(g)))
    cells, idx = cells.value, np.ascontiguousarray(s["slots"], dtype=np.uint64)
    levels_a, levels_b = s["before_a"] if levels_a is None else levels_a, s["before_b"] if levels_b is None else levels_b
    up = []
    try:
        d_la, d_lb, d_roots = _dev(api, up, levels_a), _dev(api, up, levels_b), _dev(api, up, s["ix"]["roots"][:K + 1])
        d_adv, d_sel, d_pub = api.DeviceBuffer(cells * 32), api.DeviceBuffer(cells), api.DeviceBuffer((6 * m + 4) * 32)
        up += [d_adv, d_sel, d_pub]
        check(lib.vdb_memset_dev(d_adv.ptr, 0xA5, ctypes.c_size_t(cells * 32)))
        check(lib.vdb_memset_dev(d_sel.ptr, 0xFF, ctypes.c_size_t(cells)))
        run = lambda: check(lib.vdb_wit_ann_move_dev(d_la.ptr, d_lb.ptr, d_roots.ptr, K, s["a"], s["b"], s["n_a"], s["n_b"], g.value, api._p(idx), m, d_adv.ptr,
                                                     d_sel.ptr, d_pub.ptr))
        run()
        api.sync()
        out = [d_adv.download((cells, 4)), d_sel.download((cells,), dtype=np.uint8), d_pub.download((6 * m + 4, 4)), d_la.download(levels_a.shape),
               d_lb.download(levels_b.shape)]
        if profile:
            d_la.upload(levels_a)
            d_lb.upload(levels_b)
            api.profile_begin(deferred=True)
            run()
            api.sync()
            out.append({name: int(v["launches"]) for name, v in api.profile_end().items()})
        return out
    finally:
        for b in up:
            b.free()


# ---------------------------------------------------------------------------------------------------------------- streams and trees
@pytest.mark.parametrize("name", sorted(AV.SHAPES))
def test_entry_points_write_the_models_stream_and_leave_the_models_trees(api, O, name):
    s = _case(O, name)
    m, K = s["m"], s["K"]
    stream, flags, pub, la, lb = _move_dev(api, s)
    assert stream.shape == m["advice"].shape
    bad = np.flatnonzero((stream != m["advice"]).any(axis=1))
    assert bad.size == 0, f"first differing advice cells {bad[:5]} of {stream.shape[0]} (blocks {m['regions']})"
    assert np.array_equal(flags & 1, m["selectors"]) and not (flags & ~np.uint8(3)).any()
    # the flag bytes: outside the hash blocks the model's (a selection's leading zero is not flagged by the generator, as in the query
    # circuit); inside E', S and E_b the gate bits above, the single cells below, and one flag pattern for every node hash
    r, u, ub = m["regions"], m["delete"], m["append"]
    outside = np.ones(flags.shape[0], dtype=bool)
    outside[r["update"]:r["mid"]] = False
    outside[r["update_b"]:r["new_roots"]] = False
    diff = np.flatnonzero((flags != m["flags"]) & outside)
    assert diff.size == 0 and not flags[:K + 3].any(), (diff[:8], r)
    d_a, sh, d_b, g = s["shape"]
    hashes = [r["update"] + lv + off for reg in u["regions"] for lv in reg["levels"] for off in (20, 20 + 4506 + 16)]
    hashes += [r["shrink"] + 2 + h * 4506 for h in range(d_a - 1 + sh)] if sh else []
    hashes += [r["update_b"] + lv + off for reg in ub["regions"] for lv in reg["levels"] for off in (20, 20 + 4506 + 16)]
    hashes += [r["update_b"] + x for x in ub["growth"]["z"] + ub["growth"]["r"]] if g else []
    assert all(np.array_equal(flags[h:h + 4506], flags[hashes[0]:hashes[0] + 4506]) for h in hashes)
    assert len(hashes) >= len(s["slots"]) * (4 * d_a + 2 * d_b)
    carried = [r["update"] + x for x in u["carried"]] + [r["update_b"] + x for x in ub["carried"]]
    assert not flags[carried].any(), "a carried leaf is a plain witness cell"
    assert (flags[[r["update"] + x for x in u["constants"]] + [r["update_b"] + x for x in ub["constants"]]] == 2).all()
    if sh:
        assert flags[r["shrink"]] == 0 and flags[r["shrink"] + 1] == 2
    assert np.array_equal(pub, m["public"]) and pub.shape[0] == 6 * len(s["slots"]) + 4
    assert np.array_equal(la, MU.flat_levels(s["tree_a"])) and np.array_equal(lb, MU.flat_levels(s["tree_b"]))
    host = api.wit_ann_move(s["before_a"], s["before_b"], s["ix"]["roots"][:K + 1], s["a"], s["b"], s["n_a"], s["n_b"], s["slots"], selectors=True)
    assert np.array_equal(host["stream"], stream) and np.array_equal(host["flags"], flags) and np.array_equal(host["public"], pub)
    assert np.array_equal(host["levels_src"], la) and np.array_equal(host["levels_dst"], lb) and host["input_cells"] == K + 3
    assert (host["delete_base"], host["shrink_base"], host["append_base"], host["shrink"], host["grow"]) == (r["update"], r["shrink"], r["update_b"], sh, g)


def test_two_windowed_calls_write_the_bytes_of_one(api, O):
    from halo2_vectordb_amd._lib import check
    lib = api.init()
    s = _case(O, "repeat")
    m, K = s["m"], s["K"]
    want, pub, r, u, ub = m["advice"], m["public"], m["regions"], m["delete"], m["append"]
    assert (m["s"], m["g"]) == (2, 2)
    cells = want.shape[0]
    lk = np.zeros((0, 4), dtype=np.uint64)
    idx = np.ascontiguousarray(s["slots"], dtype=np.uint64)
    up = []
    try:
        d_roots, d_pub = _dev(api, up, s["ix"]["roots"][:K + 1]), _dev(api, up, np.zeros_like(pub))
        # in front of and behind a carried cell of E_b, inside E_b's growth block and a level of it; inside S: between S_0 and Z_0, inside
        # an S hash; between F_a and B_b, inside B_b, between C_b and E_b; inside F_b; a carried cell of E'; the header; near the end
        for cut in (r["update_b"] + ub["carried"][1], r["update_b"] + ub["carried"][2] + 1, r["update_b"] + ub["growth"]["r"][1] + 40,
                    r["update_b"] + ub["regions"][1]["levels"][2] + 25, r["shrink"] + 1, r["mid"] - 4506 - 7, r["indicator_b"], r["indicator_b"] + 8 + 5,
                    r["update_b"], r["new_roots"] + 11, r["update"] + u["carried"][1], 2, cells - 3):
            halves = []
            for window in ((0, cut, 0, 0), (cut, cells, 0, 0)):
                d_la, d_lb = _dev(api, up, s["before_a"]), _dev(api, up, s["before_b"])      # every call starts from the trees before the batch
                run = lambda d_adv, d_lk: check(lib.vdb_wit_ann_move_dev(d_la.ptr, d_lb.ptr, d_roots.ptr, K, s["a"], s["b"], s["n_a"], s["n_b"], m["g"],
                                                                         api._p(idx), len(idx), d_adv.ptr, None, d_pub.ptr))
                g_adv, _ = _windowed(api, lib, check, want, lk, window, run)
                _check_window(want, lk, g_adv, lk, window, (cut, window))
                assert np.array_equal(d_pub.download(pub.shape), pub), (cut, window)
                assert np.array_equal(d_la.download(s["before_a"].shape), MU.flat_levels(s["tree_a"])), (cut, window)
                assert np.array_equal(d_lb.download(s["before_b"].shape), MU.flat_levels(s["tree_b"])), (cut, window)
                halves.append(g_adv)
            assert np.array_equal(np.concatenate([halves[0][:cut], halves[1][cut:]]), want), cut
    finally:
        for b in up:
            b.free()


def test_launch_list_depends_on_the_depths_and_on_s_and_g_alone_and_refused_arguments_launch_nothing(api, O):
    from halo2_vectordb_amd._lib import check
    lib = api.init()
    counts = {}
    counts["m1"] = _move_dev(api, _case(O, "shrink_grow"), profile=True)[5]                                        # 5 -> 4 | 4 -> 5: d_a 3, d_b 3
    counts["m2"] = _move_dev(api, _case(O, "shrink_grow", slots=[1, 3], sizes=(5, 3, 3)), profile=True)[5]         # 5 -> 3 | 3 -> 5: the same depths
    counts["K2"] = _move_dev(api, _case(O, "shrink_grow", sizes=(5, 4)), profile=True)[5]
    counts["back"] = _move_dev(api, _case(O, "shrink_grow", sizes=(3, 4, 5), ab=(2, 1)), profile=True)[5]          # a > b, the same depths
    counts["flat"] = _move_dev(api, _case(O, "flat"), profile=True)[5]                                             # 4 -> 3 | 3 -> 4: d 2, 2, s = g = 0
    assert counts["m1"] == counts["m2"] == counts["K2"] == counts["back"], counts
    want = dict(k_annmv_header=1, k_annu_indicator=2, k_nv_select=2, k_mk_leaf_states=4, k_mk_leaf_trace=4, k_mku_touchers=2, k_mku_level=6,
                k_mku_grow_trace=1, k_mku_writeback=2, k_mku_inputs=2, k_mku_level_trace=2, k_mku_index=2, k_annd_shrink_trace=1, k_annu_new_roots=2,
                k_annmv_public=1, k_inv_fixup=1)
    assert counts["m1"] == want, counts
    flat = dict(want, k_mku_level=4)
    del flat["k_annd_shrink_trace"], flat["k_mku_grow_trace"]
    assert counts["flat"] == flat, counts
    # refusals (K, a, b, n_a, n_b, grow, slots): no move, too many, emptying a (m = n_a and beyond), a slot at the fill, a slot at the fill
    # at its turn, a = b, a >= K, b >= K, K < 2, K too large, an empty b, a grow that is too small and one that is too large
    s = _case(O, "shrink_grow")
    old = api.ann_index_build(s["db"], s["ids"], s["cent"])
    up = []
    try:
        d_la, d_lb, d_roots = _dev(api, up, s["before_a"]), _dev(api, up, s["before_b"]), _dev(api, up, s["ix"]["roots"][:4])
        d_out = api.DeviceBuffer(1 << 16)
        up.append(d_out)
        check(lib.vdb_memset_dev(d_out.ptr, 0xA5, ctypes.c_size_t(1 << 16)))
        api.sync()
        api.profile_begin(deferred=True)
        for K, a, b, n_a, n_b, grow, idx in ((3, 0, 1, 5, 4, 1, []), (3, 0, 1, 5000, 4, 10, [0] * 2049), (3, 0, 1, 5, 4, 2, [0] * 5), (3, 0, 1, 2, 4, 1, [0] * 3),
                                             (3, 0, 1, 5, 4, 1, [5]), (3, 0, 1, 5, 4, 1, [0, 4]), (3, 0, 0, 5, 5, 1, [1]), (3, 3, 1, 5, 4, 1, [1]),
                                             (3, 0, 3, 5, 4, 1, [1]), (1, 0, 0, 5, 4, 1, [1]), (4097, 0, 1, 5, 4, 1, [1]), (3, 0, 1, 5, 0, 1, [1]),
                                             (3, 0, 1, 5, 4, 0, [1]), (3, 0, 1, 5, 4, 2, [1]), (3, 0, 1, 5, 3, 1, [1])):
            uidx = np.ascontiguousarray(idx + [0], dtype=np.uint64)
            with pytest.raises(api.VdbError) as e:
                check(lib.vdb_wit_ann_move_dev(d_la.ptr, d_lb.ptr, d_roots.ptr, K, a, b, n_a, n_b, grow, api._p(uidx), len(idx), d_out.ptr, None,
                                               d_out.at(1 << 15)))
            assert e.value.code == -3, (K, a, b, n_a, n_b, grow, idx)
        for a, b, slots, grow in ((0, 0, [1], None), (0, 3, [1], None), (0, 1, [5], None), (0, 1, [0, 4], None), (2, 0, [0, 0, 0], None), (0, 1, [], None),
                                  (0, 1, [1], 0), (0, 1, [1], 2)):
            with pytest.raises(api.VdbError) as e:
                api.ann_index_move(old, a, b, MU.flat_levels(s["tree_a"]), MU.flat_levels(s["tree_b"]), slots, grow=grow)
            assert e.value.code == -3, (a, b, slots, grow)
        api.sync()
        assert api.profile_end() == {}
        assert (d_out.download((1 << 16,), dtype=np.uint8) == 0xA5).all()
        assert np.array_equal(d_la.download(s["before_a"].shape), s["before_a"]) and np.array_equal(d_lb.download(s["before_b"].shape), s["before_b"])
    finally:
        for b in up:
            b.free()


# ---------------------------------------------------------------------------------------------------------------- the index after the batch
def _fresh_build_over_own_rows(api, got, K, cent):
    """the result equals ann_index_build over its own grouped rows with nondecreasing ids, entry for entry but the slots, which a fresh
    build numbers 0 .. n - 1"""
    ids2 = np.repeat(np.arange(K), np.diff(got["offsets"].astype(np.int64)))
    want = api.ann_index_build(got["grouped"], ids2, cent)
    for key in ("grouped", "offsets", "roots", "forest"):
        assert np.array_equal(got[key], want[key]), key
    assert np.array_equal(got["segments"], want["segments"]) and np.array_equal(want["slots"], np.arange(len(ids2), dtype=np.uint32))
    return ids2


@pytest.mark.parametrize("name", sorted(AV.SHAPES))
def test_moved_index_is_a_fresh_build_over_its_own_rows_and_every_row_keeps_its_slot(api, O, name):
    s = _case(O, name)
    a, b = s["a"], s["b"]
    old = api.ann_index_build(s["db"], s["ids"], s["cent"])
    got = api.ann_index_move(old, a, b, MU.flat_levels(s["tree_a"]), MU.flat_levels(s["tree_b"]), s["slots"])
    ids2 = _fresh_build_over_own_rows(api, got, s["K"], s["cent"])
    grouped2, want_ids, slots2 = AV.moved_grouping(s["db"], s["ids"], a, b, s["slots"])
    assert np.array_equal(got["grouped"], grouped2) and np.array_equal(ids2, want_ids)
    assert np.array_equal(got["slots"].astype(np.int64), slots2) and sorted(got["slots"].tolist()) == list(range(len(s["ids"])))
    assert np.array_equal(s["db"][got["slots"]], got["grouped"]), "each row keeps its database slot"
    assert np.array_equal(got["roots"][-1], s["m"]["public"][-1]), "the moved index's root is the circuit's public index_root_new"
    sh, g = api.ann_index_move_layout(np.diff(old["offsets"].astype(np.int64)), a, b, s["slots"])[:2]
    assert (sh, g) == (s["m"]["s"], s["m"]["g"])


def test_a_batch_beyond_one_workgroup(api, O):
    """(130, 3) at dim 3, 67 moves: a goes 256 -> 64 leaves (s = 2), b 4 -> 128 (g = 5): more than 64 moves, more than one workgroup of
    rows and of digests.  Values only: the witness call supplies the two trees, no model stream"""
    n_a, n_b, k = 130, 3, 67
    rng = np.random.default_rng(5)
    slots = [int(rng.integers(0, n_a - j)) for j in range(k)]
    slots[3], slots[40] = n_a - 4, 0                                 # a self-carry and slot 0 again
    ids = AD.ids_of((n_a, n_b))
    db, cent = O.quantize(_rows(80, n_a + n_b, DIM), P), O.quantize(_rows(81, 2, DIM), P)
    old = api.ann_index_build(db, ids, cent)
    tree_a = old["forest"][int(old["segments"][0]):int(old["segments"][1])]
    tree_b = api.merkle_tree_grow(old["forest"][int(old["segments"][1]):int(old["segments"][2])], n_b, 5)
    w = api.wit_ann_move(tree_a, tree_b, old["roots"][:3], 0, 1, n_a, n_b, slots)
    assert (w["shrink"], w["grow"]) == (2, 5)
    got = api.ann_index_move(old, 0, 1, w["levels_src"], w["levels_dst"], slots)
    ids2 = _fresh_build_over_own_rows(api, got, 2, cent)
    grouped2, want_ids, slots2 = AV.moved_grouping(db, ids, 0, 1, slots)
    assert np.array_equal(got["grouped"], grouped2) and np.array_equal(ids2, want_ids) and np.array_equal(got["slots"].astype(np.int64), slots2)
    assert np.array_equal(got["roots"][-1], w["public"][-1]) and np.array_equal(old["roots"][-1], w["public"][0])
    # both trees' roots against merkle_tree_build over the members
    mem_a, mem_b = got["grouped"][:n_a - k], got["grouped"][n_a - k:]
    assert np.array_equal(api.merkle_tree_build(mem_a)[-2], got["roots"][1]) and np.array_equal(api.merkle_tree_build(mem_b)[-2], got["roots"][2])
    assert np.array_equal(w["levels_dst"][-2], got["roots"][2]) and np.array_equal(w["levels_src"][2 * (256 - 4)], got["roots"][1])
    pub = w["public"][3:-1].reshape(k, 6, 4)
    assert TM.to_ints(pub[:, 0]) == slots and TM.to_ints(pub[:, 2]) == [n_a - 1 - j for j in range(k)] and TM.to_ints(pub[:, 4]) == [n_b + j for j in range(k)]
    assert not pub[:, 5].any() and np.array_equal(pub[:, 1], w["levels_dst"][n_b:n_b + k]), "what arrived is what left, move by move"


# ---------------------------------------------------------------------------------------------------------------- the proof
@pytest.fixture(scope="module", params=["shrink_grow", "backwards"])
def proved(api, O, request):
    """one AnnMoveHotPath per shape with its keys and its proof, shared by the tests below"""
    from halo2_vectordb_amd.pipeline import AnnIndex, AnnMoveHotPath
    from halo2_vectordb_amd.rounds import ProverRounds
    s = _case(O, request.param)
    index = AnnIndex(len(s["ids"]), s["dim"], s["K"], s["f"]["db"], s["ids"], s["f"]["cent"], P=P, L=13)
    hp = AnnMoveHotPath(index, s["a"], s["b"], s["slots"], k=13, tau=TAU).setup()
    pr = ProverRounds(hp).keygen()
    hp._witness()
    api.sync()
    stream = hp.d_stream.download((hp.n_cells, 4))
    out = pr.prove(None, seed=23)
    yield dict(s=s, index=index, hp=hp, pr=pr, out=out, stream=stream)
    pr.free()
    hp.free()
    index.free()


def test_hot_path_proves_the_models_batch_and_changed_instances_are_rejected(api, O, proved):
    from halo2_vectordb_amd import verifier
    s, hp, pr, out = proved["s"], proved["hp"], proved["pr"], proved["out"]
    m, k = s["m"], len(s["slots"])
    assert hp.n_cells == m["advice"].shape[0] and hp.n_in == s["K"] + 3 and hp.n_lookup == 0 and np.array_equal(hp.bp, m["break_points"])
    assert (hp.depth, hp.shrink, hp.depth_b, hp.grow) == s["shape"] and hp.n_input_rows() == 0
    assert (hp.delete_base, hp.shrink_base, hp.append_base) == (m["regions"]["update"], m["regions"]["shrink"], m["regions"]["update_b"])
    assert pr.keygen_report.violations() == 0, pr.keygen_report.as_dict()
    assert pr.mock_check().violations() == 0
    assert np.array_equal(proved["stream"], m["advice"])
    res = hp.results()
    assert np.array_equal(np.concatenate([res[0][None], res[1][None], res[2][None], np.stack(res[3:9], axis=1).reshape(-1, 4), res[9][None]]), m["public"])
    assert np.array_equal(res[0], proved["index"].roots()[-1])
    mem_a, mem_b, last = AV.simulate(s["n_a"], s["n_b"], s["slots"])
    assert hp.origin == mem_a and hp.moved_from == [i for w, i in mem_b if w == "a"]
    assert TM.to_ints(res[5]) == last and TM.to_ints(res[3]) == s["slots"] and TM.to_ints(res[7]) == [s["n_b"] + j for j in range(k)] and not res[8].any()
    assert np.array_equal(hp.d_levels_a.download((2 * hp.lp, 4)), MU.flat_levels(s["tree_a"]))
    assert np.array_equal(hp.d_levels_b.download((2 * hp.lp_b, 4)), MU.flat_levels(s["tree_b"]))
    want = TM.to_ints(m["public"])
    assert out["instances"] == want and len(want) == 6 * k + 4
    vk = verifier.VerifyingKey.from_prover(pr, out["opened"])
    assert verifier.verify(out["proof"], want, vk)
    for at in range(len(want)):                                  # every public value: both roots, a, b, and the six values of every move
        wrong = list(want)
        wrong[at] = (wrong[at] + 1) % O.R_MOD
        assert not verifier.verify(out["proof"], wrong, vk), at


def test_cells_tampered_in_hbm_fail_the_mock_stage(api, O, proved):
    from halo2_vectordb_amd import circuit_sym as CS
    s, hp, pr = proved["s"], proved["hp"], proved["pr"]
    hp._witness()
    api.sync()
    stream = hp.d_stream.download((hp.n_cells, 4))
    assert np.array_equal(stream, proved["stream"])
    lay = CS.ann_move_layout(s["K"], hp.m, hp.depth, hp.shrink, hp.depth_b, hp.grow)
    u, ub, K = lay["update_layout"], lay["update_b_layout"], s["K"]
    one = O.fr_from_ints([1])
    d_flags = api.DeviceBuffer(hp.n_cells)
    try:
        d_flags.upload(np.asarray(pr.circuit.gate).astype(np.uint8))
        assert pr.mock_check(d_flags).violations() == 0              # the witness as it lies in HBM, not emitted again
        arrived = [lay["update_b"] + ub["block"][j] for j in range(hp.m)]
        removed = [lay["update"] + u["old_leaf"] + 2 * j for j in range(hp.m)]
        mids = [lay["mid"] + 8 * j + 7 for j in range(K)]
        # every carried leaf of E_b, every removed-leaf cell, every mid_j, S_0, b's out_j and another's
        for cell in arrived + removed + mids + [lay["shrink"], lay["new_roots"] + 8 * s["b"] + 7, lay["new_roots"] + 8 * s["a"] + 7]:
            hp.d_stream.upload(O.fr_add(stream[cell:cell + 1], one), offset=cell * 32)
            rep = pr.mock_check(d_flags)
            hp.d_stream.upload(np.ascontiguousarray(stream[cell:cell + 1]), offset=cell * 32)
            assert rep.violations() >= 1, (cell, rep.as_dict())
        assert pr.mock_check(d_flags).violations() == 0
    finally:
        d_flags.free()


def test_tree_of_another_cluster_breaks_its_picked_tie_alone(api, O):
    """ids 0 0 0 1 1 1 2 2 2: a move 0 -> 1 with cluster 2's tree passed as a's, then as b's: the one copy that fails is that tree's
    picked tie (the trees of a shape are interchangeable for every gate)"""
    from halo2_vectordb_amd import circuit_sym as CS
    from halo2_vectordb_amd.pipeline import AnnIndex, AnnMoveHotPath
    from halo2_vectordb_amd.rounds import ProverRounds
    ids = np.repeat(np.arange(3), 3)
    f = dict(db=_rows(96, 9, DIM), cent=_rows(97, 3, DIM))
    index = AnnIndex(9, DIM, 3, f["db"], ids, f["cent"], P=P, L=13)
    lay = CS.ann_move_layout(3, 1, 2, 1, 2, 0)
    try:
        for kw, picked in ((dict(), None), (dict(levels_src=index.levels(2)), lay["sponge_old"] - 1), (dict(levels_dst=index.levels(2)), lay["update_b"] - 1)):
            hp = AnnMoveHotPath(index, 0, 1, [1], k=13, tau=TAU, **kw).setup()
            pr = ProverRounds(hp).keygen()
            try:
                rep = pr.keygen_report
                if picked is None:
                    assert rep.violations() == 0, rep.as_dict()
                else:
                    assert rep.violations() == rep.copies_unequal == 1 and int(pr.circuit.copy_of[rep.first_copy]) == picked, rep.as_dict()
            finally:
                pr.free()
                hp.free()
    finally:
        index.free()


# ---------------------------------------------------------------------------------------------------------------- the resident index
def test_moved_keeps_the_database_and_a_cover_publishes_the_old_database_root(api, O, proved):
    from halo2_vectordb_amd.pipeline import AnnCoverHotPath
    s, hp, index = proved["s"], proved["hp"], proved["index"]
    K, dim = s["K"], s["dim"]
    made = []
    try:
        before = [b.download((b.nbytes,), dtype=np.uint8) for b in (index.d_grouped, index.d_slots, index.d_offsets, index.d_forest, index.d_roots)]
        ix2 = index.moved(hp)
        made.append(ix2)
        got = _resident(ix2, K, dim)
        _fresh_build_over_own_rows(api, got, K, s["cent"])
        grouped2, ids2, slots2 = AV.moved_grouping(s["db"], s["ids"], s["a"], s["b"], s["slots"])
        assert np.array_equal(got["grouped"], grouped2) and np.array_equal(got["slots"].astype(np.int64), slots2)
        assert np.array_equal(ix2.qvec, index.qvec) and ix2.n == index.n
        want_ids = np.zeros(len(ids2), dtype=np.uint32)
        want_ids[slots2] = ids2
        assert np.array_equal(ix2.cluster_ids, want_ids) and np.array_equal(ix2.sizes, np.bincount(ids2))
        lp = 2 * api.merkle_levels(index.n)[0]
        assert np.array_equal(ix2.database_tree().download((lp, 4)), index.database_tree().download((lp, 4))), "no vector of the database changed"
        root_new = hp.results()[9]
        assert np.array_equal(ix2.roots()[-1], root_new)
        cover_old, cover_new = AnnCoverHotPath(index, k=12, L=L, tau=TAU).setup(), AnnCoverHotPath(ix2, k=12, L=L, tau=TAU).setup()
        made += [cover_old, cover_new]
        cover_old._witness()
        cover_new._witness()
        api.sync()
        assert np.array_equal(cover_new.results()[0], cover_old.results()[0]), "the old database_root"
        assert np.array_equal(cover_new.results()[1], root_new) and np.array_equal(cover_old.results()[1], hp.results()[0])
        after = [b.download((b.nbytes,), dtype=np.uint8) for b in (index.d_grouped, index.d_slots, index.d_offsets, index.d_forest, index.d_roots)]
        assert all(np.array_equal(x, y) for x, y in zip(before, after)), "the old index's buffers are only read"
    finally:
        for x in reversed(made):
            x.free()


def test_a_chain_there_and_back_keeps_every_clusters_multiset_of_leaves(api, O):
    from halo2_vectordb_amd.pipeline import AnnIndex, AnnMoveHotPath
    s = _case(O, "backwards")
    K, dim, a, b, k = s["K"], s["dim"], s["a"], s["b"], len(s["slots"])
    made = []
    try:
        ix0 = AnnIndex(len(s["ids"]), dim, K, s["f"]["db"], s["ids"], s["f"]["cent"], P=P, L=13)
        made.append(ix0)
        hp1 = AnnMoveHotPath(ix0, a, b, s["slots"], k=13, tau=TAU).setup()
        made.append(hp1)
        hp1._witness()
        api.sync()
        ix1 = ix0.moved(hp1)
        made.append(ix1)
        # the same members back: they are the last k of b
        back = [s["n_b"] + k - 1 - j for j in range(k)]
        hp2 = AnnMoveHotPath(ix1, b, a, back, k=13, tau=TAU).setup()
        made.append(hp2)
        assert (hp2.shrink, hp2.grow) == (hp1.grow, hp1.shrink)
        hp2._witness()
        api.sync()
        assert np.array_equal(hp2.results()[0], hp1.results()[9]), "the second move starts from the first one's public index_root_new"
        ix2 = ix1.moved(hp2)
        made.append(ix2)
        r0, r2 = _resident(ix0, K, dim), _resident(ix2, K, dim)
        _fresh_build_over_own_rows(api, r2, K, s["cent"])
        assert np.array_equal(ix2.sizes, ix0.sizes) and np.array_equal(ix2.cluster_ids, ix0.cluster_ids)
        for c in range(K):
            leaves = lambda r: sorted(TM.to_ints(r["forest"][int(r["segments"][c]):int(r["segments"][c]) + int(ix0.sizes[c])]))
            assert leaves(r0) == leaves(r2), c
        assert np.array_equal(s["db"][r2["slots"]], r2["grouped"]) and sorted(r2["slots"].tolist()) == list(range(ix0.n))
    finally:
        for x in reversed(made):
            x.free()


def test_the_other_hot_paths_run_on_the_moved_index(api, O, proved):
    """one small call of each: a query, a read, an update, a delete and a routing audit against the moved index and its root"""
    from halo2_vectordb_amd.pipeline import AnnAuditHotPath, AnnDeleteHotPath, AnnQueryHotPath, AnnUpdateHotPath, ReadHotPath
    s, hp = proved["s"], proved["hp"]
    b, dim = s["b"], s["dim"]
    made = []
    try:
        ix2 = proved["index"].moved(hp)
        made.append(ix2)
        root_new = hp.results()[9]
        n_b2 = int(ix2.sizes[b])
        assert n_b2 == s["n_b"] + hp.m
        q = AnnQueryHotPath(ix2, s["f"]["cent"][b] + 0.25, cluster=b, k=13, P=P, L=L, tau=TAU).setup()
        made.append(q)
        q._witness()
        api.sync()
        assert np.array_equal(q.results()[3], root_new)
        members = api.dequantize(ix2.members(b), P)
        rd = ReadHotPath(n=n_b2, dim=dim, m=1, k=13, P=P, tau=TAU, vectors=members, levels=ix2.levels(b), reads=[n_b2 - 1]).setup()
        made.append(rd)
        rd._witness()
        api.sync()
        moved_row = AN.select_cluster(s["db"], s["ids"], s["a"])[0][hp.moved_from[-1]]
        assert np.array_equal(rd.results()[0], ix2.roots()[1 + b]) and np.array_equal(np.asarray(rd.results()[3]).reshape(-1, 4), moved_row)
        au = AnnUpdateHotPath(ix2, b, ([0], _rows(71, 1, dim)), grow=None, k=13, tau=TAU).setup()
        made.append(au)
        au._witness()
        api.sync()
        assert np.array_equal(au.results()[0], root_new)
        ad = AnnDeleteHotPath(ix2, b, [0], k=13, tau=TAU).setup()
        made.append(ad)
        ad._witness()
        api.sync()
        assert np.array_equal(ad.results()[0], root_new) and np.array_equal(ad.results()[5][0], ix2.levels(b).download((2 * ad.lp, 4))[n_b2 - 1])
        aa = AnnAuditHotPath(ix2, b, k=13, P=P, L=L, tau=TAU).setup()
        made.append(aa)
        aa._witness()
        api.sync()
        assert np.array_equal(aa.results()[0], root_new)
    finally:
        for x in reversed(made):
            x.free()


# ---------------------------------------------------------------------------------------------------------------- the sweeps on the device map
def test_single_cell_alteration_sweep(api, O):
    """tests/alteration_model.py's method on the device map and the kernels' bytes at the shape with a shrink and a growth: the one kind
    of cell that stays free is the inverse witness of the is_zero whose operand is zero (tests/test_ann_move_cpu.py pins it to one cell
    per indicator block)"""
    from halo2_vectordb_amd.pipeline import AnnIndex, AnnMoveHotPath
    from test_gpu_alteration import device_sweep
    s = _case(O, "shrink_grow")
    index = AnnIndex(len(s["ids"]), s["dim"], s["K"], s["f"]["db"], s["ids"], s["f"]["cent"], P=P, L=13)
    try:
        hp = AnnMoveHotPath(index, s["a"], s["b"], s["slots"], k=13, tau=TAU).setup()
        device_sweep(api, O, "ann move K 3 0 -> 1 m 1 s 1 g 1", hp)          # frees the hot path
    finally:
        index.free()


def _splice_with_inputs_inside_the_stream(api, O, name, hp, moves):
    """test_gpu_splice.device_splice from its own parts, for a circuit whose assigned witnesses do not all lie at the head of the stream:
    device_splice requires that nothing behind the first n_in cells is loaded with load_witness (but a Hamming distance's two cells),
    and the two update blocks assign theirs (old leaves, bits, siblings, R_0, S_0) where they start.  Those cells are inputs like the
    header's: the sweep is run between two witnesses in which NONE of them differs, which is asserted, so that the one altered input
    is still the only free cell among the changed ones.  Everything else is device_splice's: (1) both streams honest on the device,
    judge's (2), (4), (5), every cut's hybrid passing, the suffix splices against the recount, the dropped tie, (3) a public cell
    reached, and the stream back where it was."""
    import alteration_model as AM
    import splice_model as SM
    from halo2_vectordb_amd.rounds import ProverRounds
    from test_circuit_sym_cpu import to_ints
    from test_gpu_alteration import Checker
    from test_gpu_splice import Device, downloaded_map, dropped_tie, hybrid, streams, suffix_splices
    from test_splice_cpu import judge
    pr = ProverRounds(hp).keygen()
    chk = None
    try:
        assert pr.keygen_report.violations() == 0, pr.keygen_report.as_dict()
        cm, public, n, L_ = downloaded_map(pr), [int(c) for c in pr.instance_cells], hp.n_cells, hp.L
        loaded = np.asarray(SM.loaded_witnesses(cm, hp.n_in), dtype=np.int64)
        assert len(loaded) >= 1 and loaded.min() >= hp.delete_base, "the update blocks' assigned witnesses"
        rows = hp.vectors_f64.copy()
        honest = streams(api, hp)
        chk = Checker(api, O, hp.d_stream, hp.d_lookup, cm, L_, public, [0] * len(public))
        dev = Device(O, chk, hp.d_stream, hp.d_lookup, honest[0], honest[1], public)
        assert AM.violations(dev.report()) == 0
        reached = False
        checker_for = lambda m: Checker(api, O, hp.d_stream, hp.d_lookup, m, L_, public, [0] * len(public))
        for first, (what, i, j, new) in enumerate(moves(rows)):
            w = rows.copy()
            w[i, j] = new
            hp.set_vectors(w)
            other = streams(api, hp)
            hp.set_vectors(rows)
            dev.now = [other[0].copy(), other[1].copy()]
            assert AM.violations(dev.report()) == 0, (name, what)
            dev.show(*honest)
            D, DL = SM.changed(honest[0], other[0], honest[1], other[1])
            assert not np.isin(loaded, D).any(), "no assigned witness inside the stream differs between the two"
            need = SM.needed(cm, D, DL, public)
            W, W2 = (SM.sparse(n, need, to_ints(O, s_[0][need])) for s_ in (honest, other))
            LK, LK2 = (SM.sparse(0, DL, []) for _ in range(2))
            got = judge(f"{name}, {what}", cm, hp.n_in, W, W2, LK, LK2, D, DL, i * rows.shape[1] + j, public, L_, [])
            reached |= got["public"]
            for c in got["found"]:
                base, alt = ((honest, other), (other, honest))[c["direction"]]
                dev.show(*hybrid(base, alt, (c["cells"], c["lookups"])))
                rep = dev.report()
                assert AM.violations(rep) == 0, (name, what, SM.describe(cm, c), rep)
            dev.show(*honest)
            if first == 0:
                suffix_splices(name, cm, dev, honest, other, W, W2, LK, LK2, D, DL, got, public, L_)
                dropped_tie(name, cm, dev, checker_for, hp.n_in, honest, other, W, W2, LK, LK2, D, DL, i * rows.shape[1] + j, public, L_)
        assert reached, f"{name}: no perturbation reaches a public cell"
        assert np.array_equal(hp.d_stream.download((n, 4)), honest[0]) and AM.violations(dev.report()) == 0
    finally:
        if chk is not None:
            chk.free()
        pr.free()
        hp.free()


def test_splice_sweep_between_two_honest_witnesses(api, O):
    """tests/splice_model.py's method between two honest witnesses of the shape shrink_grow.  The circuit has no input row: what is
    varied is ONE header cell, the root of the cluster that takes no part in the move (two indexes that differ in a row of cluster 2),
    which reaches both public index roots through C_a, D, F_a, C_b, F_b and G.  The sweep's one input is stated to it as a row of the
    K + 3 header cells whose place 3 + 2 selects the index.  test_gpu_splice.device_splice itself refuses a circuit with assigned
    witnesses behind its head (as its docstring says of the ANN update and delete): the sweep runs from its parts, see above."""
    from halo2_vectordb_amd.pipeline import AnnIndex, AnnMoveHotPath
    s = _case(O, "shrink_grow")
    K, other = s["K"], 2
    assert other not in (s["a"], s["b"])
    db2 = s["f"]["db"].copy()
    db2[int(np.flatnonzero(s["ids"] == other)[0]), 1] += 1.0
    variants = [AnnIndex(len(s["ids"]), s["dim"], K, rows, s["ids"], s["f"]["cent"], P=P, L=13) for rows in (s["f"]["db"], db2)]

    class Spliced(AnnMoveHotPath):
        def set_vectors(self, w):
            self.index = variants[int(w[0, 3 + other])]

    try:
        hp = Spliced(variants[0], s["a"], s["b"], s["slots"], k=13, tau=TAU).setup()
        hp.vectors_f64 = np.zeros((1, K + 3))
        _splice_with_inputs_inside_the_stream(api, O, "ann move K 3 0 -> 1 m 1 s 1 g 1", hp,
                                              lambda r: [("the root of the cluster that stays", 0, 3 + other, 1.0)])   # frees hp
    finally:
        for ix in variants:
            ix.free()
