"""Inserts and replacements proved against the committed root (pipeline.UpdateHotPath; vdb_merkle_tree_build_dev, vdb_wit_merkle_update*)
on the GPU.  The streams are tests/merkle_update_model.py's, bit for bit — advice, gate-start flags, size, break points, public values
(tests/test_merkle_update_cpu.py holds that model against the oracle first) — and the resident tree after a batch is the tree built from
the updated database; host and device forms, rank windows, the launch count, refused arguments, the Mock stage, the whole proof, changed
instances, tampered witnesses and a second batch chained to the first."""
import ctypes

import numpy as np
import pytest

import merkle_update_model as MU
import topk_model as TM
from examples_common import load
from test_gpu_batch_query import _dev
from test_gpu_rounds import FIXED, TAU, _meta, _verify
from test_gpu_sharded import _run
from test_gpu_sweep import _check_window, _windowed

pytestmark = pytest.mark.gpu
P = 48


@pytest.fixture(scope="module")
def api():
    from halo2_vectordb_amd import api as a
    a.init(0)
    return a


def _rows(seed, n, dim):
    return np.random.default_rng(seed).integers(0, 219, size=(n, dim)).astype(np.float64)


def _size(api, n, dim, m):
    from halo2_vectordb_amd._lib import check
    cells, n_in = ctypes.c_uint64(), ctypes.c_uint64()
    check(api.init().vdb_wit_merkle_update_size(n, dim, m, ctypes.byref(cells), ctypes.byref(n_in)))
    return cells.value, n_in.value


def _tree_dev(api, db):
    """vdb_merkle_tree_build_dev -> (2 lp, 4)"""
    return api.merkle_tree_build(db)


def _dev_call(api, levels, n, new, idx):
    """vdb_wit_merkle_update_dev into poisoned buffers -> (stream, flags, public, levels after)"""
    from halo2_vectordb_amd._lib import check
    lib = api.init()
    m, dim = new.shape[0], new.shape[1]
    cells, _ = _size(api, n, dim, m)
    idx = np.ascontiguousarray(idx, dtype=np.uint64)
    up = []
    try:
        d_lv, d_new = _dev(api, up, levels), _dev(api, up, new)
        d_adv, d_sel, d_pub = api.DeviceBuffer(cells * 32), api.DeviceBuffer(cells), api.DeviceBuffer((3 * m + 2) * 32)
        up += [d_adv, d_sel, d_pub]
        check(lib.vdb_memset_dev(d_adv.ptr, 0xA5, ctypes.c_size_t(cells * 32)))
        check(lib.vdb_memset_dev(d_sel.ptr, 0xFF, ctypes.c_size_t(cells)))
        check(lib.vdb_wit_merkle_update_dev(d_lv.ptr, n, dim, d_new.ptr, api._p(idx), m, d_adv.ptr, d_sel.ptr, d_pub.ptr))
        api.sync()
        return d_adv.download((cells, 4)), d_sel.download((cells,), dtype=np.uint8), d_pub.download((3 * m + 2, 4)), d_lv.download(levels.shape)
    finally:
        for b in up:
            b.free()


def _apply(db, n_lp, idx, new):
    """the database after the batch: replacements in place, inserts appended (an insert takes the first free slot)"""
    cur = [db[i] for i in range(db.shape[0])]
    for j, i in enumerate(idx):
        if i < len(cur):
            cur[i] = new[j]
        else:
            assert i == len(cur) < n_lp
            cur.append(new[j])
    return np.stack(cur)


# (n, dim, indices): depth 1, 3 and 10; dim 4, 5 and 128; m 1, 2 and 64; the first and last leaf; n a power of two and not; repeated
# slots; sibling pairs; inserts at n and n + 1
CASES = {
    "depth1_m1_last": (2, 4, [1]),
    "depth1_m2_both": (2, 5, [0, 1]),
    "depth3_pow2_first_last_repeat": (8, 4, [0, 7, 0, 7, 3]),
    "depth3_siblings_and_inserts": (6, 5, [4, 5, 6, 7, 6, 2, 3]),
    "depth10_m2_inserts": (600, 4, [600, 601]),
    "depth10_m64": (1000, 5, None),
    "dim128_m2": (5, 128, [4, 5]),
}


def _case(name):
    n, dim, idx = CASES[name]
    if idx is None:                                       # 64 updates: random slots with repeats, sibling pairs, then inserts at n, n + 1, ...
        rng = np.random.default_rng(64)
        idx = list(rng.integers(0, n, size=40)) + [10, 11, 10, 0, n - 1, 998, 999, 998] + list(range(n, n + 16))
        idx = [int(i) for i in idx]
        assert len(idx) == 64
    return n, dim, idx


@pytest.mark.parametrize("name", sorted(CASES))
def test_entry_points_write_the_models_stream_and_leave_the_updated_tree(api, O, name):
    n, dim, idx = _case(name)
    db, new = O.quantize(_rows(n, n, dim), P), O.quantize(_rows(n + 1, len(idx), dim), P)
    levels0 = _tree_dev(api, db)
    tree = MU.build_tree(O, db)
    assert np.array_equal(levels0, MU.flat_levels(tree)), "vdb_merkle_tree_build_dev"
    assert np.array_equal(levels0[2 * len(tree[0]) - 2], O.poseidon_merkle_root(db))
    m = MU.update_model(O, tree, idx, new)
    cells, n_in = _size(api, n, dim, len(idx))
    assert cells == m["advice"].shape[0] and n_in == m["n_in"]
    stream, flags, pub, levels1 = _dev_call(api, levels0, n, new, idx)
    bad = np.flatnonzero((stream != m["advice"]).any(axis=1))
    assert bad.size == 0, f"first differing advice cells {bad[:5]} of {cells}"
    assert np.array_equal(flags & 1, m["selectors"]) and not (flags & ~np.uint8(3)).any()
    assert np.array_equal(pub, m["public"])
    after = _apply(db, len(tree[0]), idx, new)
    assert np.array_equal(levels1, MU.flat_levels(tree)), "the tree after the batch is the sequential one"
    assert np.array_equal(levels1, _tree_dev(api, after)), "... and vdb_merkle_tree_build_dev of the updated database"
    assert np.array_equal(pub[-1], O.poseidon_merkle_root(after))
    # the host-buffer form writes the same bytes
    host = api.wit_merkle_update(levels0, n, new, idx, selectors=True)
    assert np.array_equal(host["stream"], stream) and np.array_equal(host["flags"], flags) and np.array_equal(host["public"], pub)
    assert np.array_equal(host["levels"], levels1) and host["input_cells"] == n_in


def test_reference_shaped_inputs(api, O):
    """data/query.in's database (20 x 3) takes data/euclid.in's two vectors: a replacement and an insert"""
    db = O.quantize(np.asarray(load("query")["database"], dtype=np.float64), P)
    e = load("euclid")
    new = O.quantize(np.asarray([e["a"], e["b"]], dtype=np.float64), P)
    n, idx = db.shape[0], [7, 20]
    levels0 = _tree_dev(api, db)
    tree = MU.build_tree(O, db)
    m = MU.update_model(O, tree, idx, new)
    stream, flags, pub, levels1 = _dev_call(api, levels0, n, new, idx)
    assert np.array_equal(stream, m["advice"]) and np.array_equal(flags & 1, m["selectors"]) and np.array_equal(pub, m["public"])
    assert np.array_equal(pub[2 + 3], MU.ZERO) and np.array_equal(pub[-1], O.poseidon_merkle_root(_apply(db, 32, idx, new)))
    assert np.array_equal(levels1, MU.flat_levels(tree))


def test_two_windowed_calls_write_the_bytes_of_one(api, O):
    from halo2_vectordb_amd import circuit_sym as CS
    from halo2_vectordb_amd._lib import check
    lib = api.init()
    n, dim, idx = 6, 5, [4, 5, 6, 4, 1]
    db, new = O.quantize(_rows(1, n, dim), P), O.quantize(_rows(2, len(idx), dim), P)
    levels0 = _tree_dev(api, db)
    want, _flags, pub, levels1 = _dev_call(api, levels0, n, new, idx)
    cells = want.shape[0]
    lk = np.zeros((0, 4), dtype=np.uint64)
    lay_in = _size(api, n, dim, len(idx))[1]
    lay = CS.merkle_update_layout(len(idx), dim, 3)
    level1 = lay["levels_at"][1] + lay["level_cells"]                  # update 1, level 1
    # ... and inside a level's first select block, between the two permutations of its old hash, inside its second select block
    in_level = (level1 + 7, level1 + 20 + CS.perm_cells(2), level1 + 20 + lay["node_cells"] + 5)
    assert lay["n_in"] == lay_in and lay["total"] == cells
    up = []
    try:
        d_new, d_pub = _dev(api, up, new), _dev(api, up, np.zeros_like(pub))
        uidx = np.ascontiguousarray(idx, dtype=np.uint64)
        for cut in (lay_in - 3, lay_in + 2256 + 7, cells // 2, cells - 2) + in_level:
            halves = []
            for window in ((0, cut, 0, 0), (cut, cells, 0, 0)):
                d_lv = _dev(api, up, levels0)                       # every call starts from the tree before the batch
                run = lambda d_adv, d_lk: check(lib.vdb_wit_merkle_update_dev(d_lv.ptr, n, dim, d_new.ptr, api._p(uidx), len(idx), d_adv.ptr, None, d_pub.ptr))
                g_adv, _ = _windowed(api, lib, check, want, lk, window, run)
                _check_window(want, lk, g_adv, lk, window, (cut, window))
                assert np.array_equal(d_pub.download(pub.shape), pub) and np.array_equal(d_lv.download(levels0.shape), levels1), (cut, window)
                halves.append(g_adv)
            assert np.array_equal(np.concatenate([halves[0][:cut], halves[1][cut:]]), want), cut
    finally:
        for b in up:
            b.free()


def test_launch_count_does_not_depend_on_the_number_of_updates(api, O):
    from halo2_vectordb_amd._lib import check
    lib = api.init()
    n, dim = 1000, 4
    db = O.quantize(_rows(3, n, dim), P)
    levels0 = _tree_dev(api, db)
    counts = {}
    for m in (1, 64):
        new = O.quantize(_rows(4, m, dim), P)
        idx = np.ascontiguousarray(np.random.default_rng(m).integers(0, n, size=m), dtype=np.uint64)
        cells, _ = _size(api, n, dim, m)
        up = []
        try:
            d_lv, d_new = _dev(api, up, levels0), _dev(api, up, new)
            bufs = [api.DeviceBuffer(cells * 32), api.DeviceBuffer((3 * m + 2) * 32)]
            up += bufs
            run = lambda: check(lib.vdb_wit_merkle_update_dev(d_lv.ptr, n, dim, d_new.ptr, api._p(idx), m, bufs[0].ptr, None, bufs[1].ptr))
            run()
            api.sync()
            api.profile_begin(deferred=True)
            run()
            api.sync()
            prof = api.profile_end()
            counts[m] = {name: int(v["launches"]) for name, v in prof.items()}
        finally:
            for b in up:
                b.free()
    assert counts[1] == counts[64], counts
    assert counts[1] == dict(k_mku_touchers=1, k_mk_leaf_states=1, k_mku_level=10, k_mku_writeback=1, k_mku_inputs=1, k_mk_leaf_trace=1,
                             k_mku_level_trace=1, k_mku_index=1), counts[1]


def test_refused_arguments_return_the_error_code_and_launch_nothing(api, O):
    from halo2_vectordb_amd._lib import check
    lib = api.init()
    cells, n_in = ctypes.c_uint64(), ctypes.c_uint64()
    for n, dim, m in ((8, 4, 0), (1, 4, 1), (0, 4, 1), (8, 0, 1), (8, 4, 4097), ((1 << 30) + 1, 4, 1), (8, (1 << 20) + 1, 1), (8, 1 << 20, 4096)):
        with pytest.raises(api.VdbError) as e:
            check(lib.vdb_wit_merkle_update_size(n, dim, m, ctypes.byref(cells), ctypes.byref(n_in)))
        assert e.value.code == -3, (n, dim, m)                            # VDB_ERR_ARG
    db, new = O.quantize(_rows(5, 6, 4), P), O.quantize(_rows(6, 2, 4), P)
    levels0 = _tree_dev(api, db)
    up = []
    try:
        d_lv, d_new = _dev(api, up, levels0), _dev(api, up, new)
        d_out = api.DeviceBuffer(1 << 16)
        up.append(d_out)
        check(lib.vdb_memset_dev(d_out.ptr, 0xA5, ctypes.c_size_t(1 << 16)))
        api.sync()
        api.profile_begin(deferred=True)
        for n, idx, m in ((6, [1, 8], 2), (6, [1 << 40, 0], 2), (6, [0, 1], 0), (1, [0, 0], 2)):
            uidx = np.ascontiguousarray(idx, dtype=np.uint64)
            with pytest.raises(api.VdbError) as e:
                check(lib.vdb_wit_merkle_update_dev(d_lv.ptr, n, 4, d_new.ptr, api._p(uidx), m, d_out.ptr, None, d_out.at(1 << 15)))
            assert e.value.code == -3, (n, idx, m)
        api.sync()
        assert api.profile_end() == {}
        assert (d_out.download((1 << 16,), dtype=np.uint8) == 0xA5).all() and np.array_equal(d_lv.download(levels0.shape), levels0)
    finally:
        for b in up:
            b.free()


def _hot_path(n, dim, idx, seed, k=13, **kw):
    from halo2_vectordb_amd.pipeline import UpdateHotPath
    return UpdateHotPath(n, dim, len(idx), k, 8, P=P, tau=TAU, vectors=_rows(seed, n, dim), updates=(idx, _rows(seed + 1, len(idx), dim)), **kw)


def test_hot_path_streams_break_points_and_results_are_the_models(api, O):
    n, dim, idx = 6, 4, [4, 5, 6, 4, 1, 7]
    hp = _hot_path(n, dim, idx, 11, k=12).setup()
    try:
        d_flags = hp.keygen_flags()
        flags = d_flags.download((hp.n_cells,), dtype=np.uint8)
        d_flags.free()
        hp._witness()
        api.sync()
        db = O.quantize(_rows(11, n, dim), P)
        tree = MU.build_tree(O, db)
        m = MU.update_model(O, tree, idx, hp.qvec, plan_k=12)
        assert np.array_equal(hp.qvec, O.quantize(_rows(12, len(idx), dim), P))
        assert hp.n_cells == m["advice"].shape[0] and hp.n_in == m["n_in"] and hp.n_lookup == 0
        assert np.array_equal(hp.d_stream.download((hp.n_cells, 4)), m["advice"]) and np.array_equal(flags & 1, m["selectors"])
        assert np.array_equal(hp.bp, m["break_points"]) and len(hp.bp) >= 3
        old_root, indices, old_leaves, new_leaves, new_root = hp.results()
        assert np.array_equal(np.concatenate([old_root[None], np.stack([indices, old_leaves, new_leaves], axis=1).reshape(-1, 4), new_root[None]]), m["public"])
        assert TM.to_ints(indices) == idx and np.array_equal(old_leaves[2], MU.ZERO) and not np.array_equal(old_leaves[3], MU.ZERO)
        assert np.array_equal(hp.d_levels.download((16, 4)), MU.flat_levels(tree)), "the updated tree stays on the device"
        assert np.array_equal(hp.d_levels0.download((16, 4)), MU.flat_levels(MU.build_tree(O, db)))
    finally:
        hp.free()


def test_proof_is_accepted_states_the_models_instances_and_chains(api, O):
    from halo2_vectordb_amd import verifier
    from halo2_vectordb_amd.pipeline import UpdateHotPath
    from halo2_vectordb_amd.rounds import ProverRounds, quotient_identity_holds
    from oracle import pairing as PR
    n, dim, idx = 6, 4, [4, 5, 6, 4]
    hp = _hot_path(n, dim, idx, 21).setup()
    pr = ProverRounds(hp).keygen()
    hp2 = pr2 = None
    try:
        assert pr.keygen_report.violations() == 0, pr.keygen_report.as_dict()
        out = pr.prove(None, seed=17)
        tree = MU.build_tree(O, O.quantize(_rows(21, n, dim), P))
        m = MU.update_model(O, tree, idx, hp.qvec)
        want = TM.to_ints(m["public"])
        assert out["instances"] == want and len(want) == 3 * len(idx) + 2
        assert quotient_identity_holds(pr, out["challenges"], out["evals"], out["instances"])
        vk = verifier.VerifyingKey.from_prover(pr, out["opened"])
        assert verifier.verify(out["proof"], want, vk)
        yvk = dict(meta=_meta(pr), opened=out["opened"], fixed={name: pr.fixed[name].commits for name in FIXED}, tau_h=PR.pt_mul(PR.G2, TAU))
        assert _verify(O, api, out["proof"], {**yvk, "instances": want})
        wrong_root = list(want)
        wrong_root[-1] = (wrong_root[-1] + 1) % O.R_MOD
        assert not verifier.verify(out["proof"], wrong_root, vk)
        wrong_leaf = list(want)                              # an insert claimed where a vector was replaced: old_leaf of update 3 set to 0
        assert wrong_leaf[1 + 3 * 3 + 1] != 0
        wrong_leaf[1 + 3 * 3 + 1] = 0
        assert not verifier.verify(out["proof"], wrong_leaf, vk)
        # a second batch from the resident tree the first left: its old root is the first's new root
        idx2 = [0, 7]
        hp2 = UpdateHotPath(n + 1, dim, len(idx2), 13, 8, P=P, tau=TAU, levels=hp.d_levels, updates=(idx2, _rows(23, len(idx2), dim))).setup()
        pr2 = ProverRounds(hp2).keygen()
        assert pr2.keygen_report.violations() == 0
        out2 = pr2.prove(None, seed=18)
        m2 = MU.update_model(O, tree, idx2, hp2.qvec)
        assert out2["instances"] == TM.to_ints(m2["public"]) and out2["instances"][0] == want[-1]
        assert verifier.verify(out2["proof"], out2["instances"], verifier.VerifyingKey.from_prover(pr2, out2["opened"]))
    finally:
        for x in (pr2, hp2, pr, hp):
            if x is not None:
                x.free()


def test_tampered_sibling_and_tampered_chain_root_are_noticed(api, O):
    """the witness as it lies in HBM with one assigned sibling altered, and with the top of update 1's old path (the cell tied to the
    root update 0 left) altered: the Mock stage reports violations for each"""
    from halo2_vectordb_amd import circuit_sym as CS
    from halo2_vectordb_amd.rounds import ProverRounds
    n, dim, idx = 6, 4, [2, 5, 2]
    hp = _hot_path(n, dim, idx, 31, k=12).setup()
    pr = ProverRounds(hp).keygen()
    try:
        assert pr.keygen_report.violations() == 0
        assert pr.mock_check().violations() == 0
        stream = hp.d_stream.download((hp.n_cells, 4))
        lay = CS.merkle_update_layout(len(idx), dim, 3)
        cm = pr.circuit
        tied = [c for c in range(lay["n_in"] + lay["per_update"], lay["n_in"] + 2 * lay["per_update"])
                if lay["n_in"] <= cm.copy_of[c] < lay["n_in"] + lay["per_update"]]
        assert len(tied) == 1 and np.array_equal(stream[tied[0]], stream[cm.copy_of[tied[0]]])
        assert tied[0] < lay["n_in"] + 2 * lay["per_update"] - lay["ip_cells"] - 16 - lay["node_cells"]      # inside the last level's old hash
        one = O.fr_from_ints([1])
        d_flags = api.DeviceBuffer(hp.n_cells)
        try:
            d_flags.upload(np.asarray(cm.gate).astype(np.uint8))
            assert pr.mock_check(d_flags).violations() == 0          # the witness as it lies in HBM, not emitted again
            for cell in (lay["sibs"] + 1 * 3 + 1, lay["sibs"], tied[0]):
                hp.d_stream.upload(O.fr_add(stream[cell:cell + 1], one), offset=cell * 32)
                rep = pr.mock_check(d_flags)
                hp.d_stream.upload(np.ascontiguousarray(stream[cell:cell + 1]), offset=cell * 32)
                assert rep.violations() >= 1, (cell, rep.as_dict())
        finally:
            d_flags.free()
    finally:
        pr.free()
        hp.free()


def test_two_sharded_ranks_write_the_one_rank_proof(tmp_path):
    """col_shard: every rank runs the whole value pass and stores the cells of its own columns"""
    one = _run(1, "merkle_update", str(tmp_path / "p1.bin"), 0)
    assert one["every_rank_wrote_the_same_bytes"] and one["quotient_identity_at_x_holds"] and one["mock_prover_violations"] == 0
    rep = _run(2, "merkle_update", str(tmp_path / "p2.bin"), 29581)
    assert rep["world"] == 2 and rep["every_rank_wrote_the_same_bytes"] and rep["quotient_identity_at_x_holds"]
    assert open(tmp_path / "p2.bin", "rb").read() == open(tmp_path / "p1.bin", "rb").read()
    assert rep["sha256"] == one["sha256"] and rep["n_instances"] == one["n_instances"] == 3 * 4 + 2
