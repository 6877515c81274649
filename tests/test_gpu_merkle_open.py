"""Reads proved against the committed root (pipeline.ReadHotPath; vdb_wit_merkle_open*) on the GPU.  The streams are
tests/merkle_open_model.py's, bit for bit — advice, gate-start flags, size, break points, public values (tests/test_merkle_open_cpu.py
holds that model against the oracle first) — in both modes; the tree is left as it was; host and device forms, rank windows, the launch
counts, refused arguments, the Mock stage, the whole proof, changed instances, a read after a write, a stale tree, tampered witnesses
and the sharded proof."""
import ctypes

import numpy as np
import pytest

import merkle_open_model as MO
import merkle_update_model as MU
import topk_model as TM
from test_gpu_batch_query import _dev
from test_gpu_rounds import FIXED, TAU, _meta, _verify
from test_gpu_sharded import _run
from test_gpu_sweep import _check_window, _windowed

pytestmark = pytest.mark.gpu
P = 48
LEAF_LAUNCHES = dict(k_mko_inputs=1, k_mko_level_trace=1, k_mko_index=1)
VECTOR_LAUNCHES = dict(LEAF_LAUNCHES, k_mk_leaf_states=1, k_mk_leaf_trace=1)


@pytest.fixture(scope="module")
def api():
    from halo2_vectordb_amd import api as a
    a.init(0)
    return a


def _rows(seed, n, dim):
    return np.random.default_rng(seed).integers(0, 219, size=(n, dim)).astype(np.float64)


def _size(api, n, dim, m, with_vectors):
    from halo2_vectordb_amd._lib import check
    cells, n_in = ctypes.c_uint64(), ctypes.c_uint64()
    check(api.init().vdb_wit_merkle_open_size(n, dim, m, int(with_vectors), ctypes.byref(cells), ctypes.byref(n_in)))
    return cells.value, n_in.value


def _n_pub(m, dim, with_vectors):
    return 1 + 2 * m + (m * dim if with_vectors else 0)


def _dev_call(api, levels, n, dim, vectors, idx):
    """vdb_wit_merkle_open_dev into poisoned buffers -> (stream, flags, public, levels after)"""
    from halo2_vectordb_amd._lib import check
    lib = api.init()
    m = len(idx)
    cells, _ = _size(api, n, dim, m, vectors is not None)
    n_pub = _n_pub(m, dim, vectors is not None)
    idx = np.ascontiguousarray(idx, dtype=np.uint64)
    up = []
    try:
        d_lv = _dev(api, up, levels)
        d_vec = _dev(api, up, vectors) if vectors is not None else None
        d_adv, d_sel, d_pub = api.DeviceBuffer(cells * 32), api.DeviceBuffer(cells), api.DeviceBuffer(n_pub * 32)
        up += [d_adv, d_sel, d_pub]
        check(lib.vdb_memset_dev(d_adv.ptr, 0xA5, ctypes.c_size_t(cells * 32)))
        check(lib.vdb_memset_dev(d_sel.ptr, 0xFF, ctypes.c_size_t(cells)))
        check(lib.vdb_wit_merkle_open_dev(d_lv.ptr, n, dim, d_vec.ptr if d_vec else None, api._p(idx), m, d_adv.ptr, d_sel.ptr, d_pub.ptr))
        api.sync()
        return d_adv.download((cells, 4)), d_sel.download((cells,), dtype=np.uint8), d_pub.download((n_pub, 4)), d_lv.download(levels.shape)
    finally:
        for b in up:
            b.free()


def _seeded_65(n):
    """65 slots with repeats: one more read than a wavefront, 650 (read, level) lanes at depth 10"""
    idx = [int(i) for i in np.random.default_rng(65).integers(0, n, size=60)] + [0, n - 1, 10, 11, 10]
    assert len(idx) == 65
    return idx


# name: (n, dim, reads in leaf mode, reads in vector mode)
CASES = {
    "depth1": (2, 4, [1], [1]),
    "depth1_odd_dim": (2, 5, [0, 1], [0, 1]),
    "depth3_repeat_first_last": (8, 4, [0, 7, 0, 3], [0, 7, 0, 3]),
    "depth3_padding_slots": (6, 5, [4, 5, 6, 7], [4, 5, 1]),
    "depth10_m65": (1000, 4, _seeded_65(1000), _seeded_65(1000)),
    "dim128": (5, 128, [4, 0], [4, 0]),
}
_trees = {}


def _tree(api, O, name):
    """the case's database, its model tree (left unchanged by every reader) and the device form of it, computed once"""
    if name not in _trees:
        n, dim = CASES[name][:2]
        db = O.quantize(_rows(n, n, dim), P)
        tree = MU.build_tree(O, db)
        levels = api.merkle_tree_build(db)
        assert np.array_equal(levels, MU.flat_levels(tree)), "vdb_merkle_tree_build_dev"
        _trees[name] = (db, tree, levels)
    return _trees[name]


@pytest.mark.parametrize("with_vectors", [True, False], ids=["vector", "leaf"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_entry_points_write_the_models_stream_and_leave_the_tree(api, O, name, with_vectors):
    n, dim, leaf_reads, vector_reads = CASES[name]
    idx = vector_reads if with_vectors else leaf_reads
    db, tree, levels = _tree(api, O, name)
    vectors = np.ascontiguousarray(db[idx]) if with_vectors else None
    m = MO.open_model(O, tree, idx, vectors)
    cells, n_in = _size(api, n, dim, len(idx), with_vectors)
    assert cells == m["advice"].shape[0] and n_in == m["n_in"]
    stream, flags, pub, levels1 = _dev_call(api, levels, n, dim, vectors, idx)
    bad = np.flatnonzero((stream != m["advice"]).any(axis=1))
    assert bad.size == 0, f"first differing advice cells {bad[:5]} of {cells}"
    assert np.array_equal(flags & 1, m["selectors"]) and not (flags & ~np.uint8(3)).any()
    assert np.array_equal(pub, m["public"]) and np.array_equal(pub[0], O.poseidon_merkle_root(db))
    assert np.array_equal(levels1, levels), "a read leaves the tree as it is"
    if not with_vectors:
        for j, i in enumerate(idx):
            assert np.array_equal(pub[2 + 2 * j], MU.ZERO) == (i >= n), "a padding slot shows leaf 0"
    # the host-buffer form writes the same bytes
    host = api.wit_merkle_open(levels, n, idx, vectors, selectors=True)
    assert np.array_equal(host["stream"], stream) and np.array_equal(host["flags"], flags) and np.array_equal(host["public"], pub)
    assert host["input_cells"] == n_in


@pytest.mark.parametrize("with_vectors", [True, False], ids=["vector", "leaf"])
def test_two_windowed_calls_write_the_bytes_of_one(api, O, with_vectors):
    from halo2_vectordb_amd import circuit_sym as CS
    from halo2_vectordb_amd._lib import check
    lib = api.init()
    name = "depth3_padding_slots"
    n, dim, leaf_reads, vector_reads = CASES[name]
    idx = vector_reads if with_vectors else leaf_reads
    db, _tree_lists, levels = _tree(api, O, name)
    vectors = np.ascontiguousarray(db[idx]) if with_vectors else None
    want, _flags, pub, _ = _dev_call(api, levels, n, dim, vectors, idx)
    cells = want.shape[0]
    lk = np.zeros((0, 4), dtype=np.uint64)
    lay = CS.merkle_open_layout(len(idx), dim, 3, with_vectors)
    level1 = lay["n_in"] + lay["per_read"] + lay["leaf_cells"] + lay["level_cells"]        # read 1, level 1
    # inside the inputs, inside a leaf sponge (vector mode), inside a level's select block, between the two permutations of its hash, inside
    # the second one, two from the end
    cuts = [lay["n_in"] - 3, level1 + 9, level1 + 20 + CS.perm_cells(2), level1 + 20 + 2256 + 1000, cells - 2] + ([lay["n_in"] + 2256 + 7] if with_vectors else [])
    up = []
    try:
        d_lv, d_pub = _dev(api, up, levels), _dev(api, up, np.zeros_like(pub))
        d_vec = _dev(api, up, vectors) if with_vectors else None
        uidx = np.ascontiguousarray(idx, dtype=np.uint64)
        run = lambda d_adv, d_lk: check(lib.vdb_wit_merkle_open_dev(d_lv.ptr, n, dim, d_vec.ptr if d_vec else None, api._p(uidx), len(idx), d_adv.ptr, None, d_pub.ptr))
        for cut in cuts:
            halves = []
            for window in ((0, cut, 0, 0), (cut, cells, 0, 0)):
                g_adv, _ = _windowed(api, lib, check, want, lk, window, run)
                _check_window(want, lk, g_adv, lk, window, (cut, window))
                assert np.array_equal(d_pub.download(pub.shape), pub), (cut, window)
                halves.append(g_adv)
            assert np.array_equal(np.concatenate([halves[0][:cut], halves[1][cut:]]), want), cut
        assert np.array_equal(d_lv.download(levels.shape), levels)
    finally:
        for b in up:
            b.free()


def test_launch_counts_depend_on_neither_reads_nor_depth(api, O):
    from halo2_vectordb_amd._lib import check
    lib = api.init()
    counts = {}
    for name, m in (("depth3_repeat_first_last", 1), ("depth10_m65", 1), ("depth10_m65", 65)):
        n, dim, reads, _ = CASES[name]
        db, _tree_lists, levels = _tree(api, O, name)
        idx = reads[:m]
        for with_vectors in (True, False):
            vectors = np.ascontiguousarray(db[idx]) if with_vectors else None
            cells, _ = _size(api, n, dim, m, with_vectors)
            uidx = np.ascontiguousarray(idx, dtype=np.uint64)
            up = []
            try:
                d_lv = _dev(api, up, levels)
                d_vec = _dev(api, up, vectors) if with_vectors else None
                bufs = [api.DeviceBuffer(cells * 32), api.DeviceBuffer(_n_pub(m, dim, with_vectors) * 32)]
                up += bufs
                run = lambda: check(lib.vdb_wit_merkle_open_dev(d_lv.ptr, n, dim, d_vec.ptr if d_vec else None, api._p(uidx), m, bufs[0].ptr, None, bufs[1].ptr))
                run()
                api.sync()
                api.profile_begin(deferred=True)
                run()
                api.sync()
                prof = api.profile_end()
                counts[(name, m, with_vectors)] = {k: int(v["launches"]) for k, v in prof.items()}
            finally:
                for b in up:
                    b.free()
    for key, got in counts.items():
        assert got == (VECTOR_LAUNCHES if key[2] else LEAF_LAUNCHES), (key, got)


def test_refused_arguments_return_the_error_code_and_launch_nothing(api, O):
    from halo2_vectordb_amd._lib import check
    lib = api.init()
    cells, n_in = ctypes.c_uint64(), ctypes.c_uint64()
    for n, dim, m in ((8, 4, 0), (1, 4, 1), (0, 4, 1), (8, 0, 1), ((1 << 30) + 1, 4, 1), (8, (1 << 20) + 1, 1), (1 << 30, 4, 1 << 27), (1 << 14, 128, 1 << 19)):
        for mode in (0, 1):
            with pytest.raises(api.VdbError) as e:
                check(lib.vdb_wit_merkle_open_size(n, dim, m, mode, ctypes.byref(cells), ctypes.byref(n_in)))
            assert e.value.code == -3, (n, dim, m, mode)                      # VDB_ERR_ARG
    db, _tree_lists, levels = _tree(api, O, "depth3_padding_slots")           # n = 6, dim = 5, lp = 8
    up = []
    try:
        d_lv, d_vec = _dev(api, up, levels), _dev(api, up, np.ascontiguousarray(db[:2]))
        d_out = api.DeviceBuffer(1 << 16)
        up.append(d_out)
        check(lib.vdb_memset_dev(d_out.ptr, 0xA5, ctypes.c_size_t(1 << 16)))
        api.sync()
        api.profile_begin(deferred=True)
        # (n, indices, m, vector mode): an index >= lp, far beyond it, m = 0, depth 0, an index >= n in vector mode
        for n, idx, m, with_vectors in ((6, [1, 8], 2, False), (6, [1 << 40, 0], 2, False), (6, [0, 1], 0, False), (1, [0, 0], 2, False), (6, [1, 8], 2, True),
                                        (6, [0, 6], 2, True), (6, [0, 1], 0, True), (1, [0, 0], 2, True)):
            uidx = np.ascontiguousarray(idx, dtype=np.uint64)
            with pytest.raises(api.VdbError) as e:
                check(lib.vdb_wit_merkle_open_dev(d_lv.ptr, n, 5, d_vec.ptr if with_vectors else None, api._p(uidx), m, d_out.ptr, None, d_out.at(1 << 15)))
            assert e.value.code == -3, (n, idx, m, with_vectors)
        api.sync()
        assert api.profile_end() == {}
        assert (d_out.download((1 << 16,), dtype=np.uint8) == 0xA5).all() and np.array_equal(d_lv.download(levels.shape), levels)
    finally:
        for b in up:
            b.free()
    # the host form refuses before it touches its output arrays
    stream = np.full((64, 4), 7, dtype=np.uint64)
    uidx = np.ascontiguousarray([0, 6], dtype=np.uint64)
    with pytest.raises(api.VdbError) as e:
        check(lib.vdb_wit_merkle_open(api._p(levels), 6, 5, api._p(np.ascontiguousarray(db[:2])), api._p(uidx), 2, api._p(stream), None, api._p(stream)))
    assert e.value.code == -3 and (stream == 7).all()


def _hot_path(n, dim, reads, seed, reveal, k=13, **kw):
    from halo2_vectordb_amd.pipeline import ReadHotPath
    kw.setdefault("vectors", _rows(seed, n, dim))
    return ReadHotPath(n, dim, len(reads), k, 8, P=P, tau=TAU, reads=reads, reveal=reveal, **kw)


def _model_of(O, hp, db_rows, reads):
    db = O.quantize(db_rows, P)
    tree = MU.build_tree(O, db)
    return MO.open_model(O, tree, reads, np.ascontiguousarray(db[reads]) if hp.with_vectors else None, plan_k=hp.k), tree


@pytest.mark.parametrize("reveal,reads", [("vector", [2, 5, 2, 0]), ("leaf", [2, 7, 5])], ids=["vector", "leaf_with_a_padding_slot"])
def test_hot_path_is_the_model_and_its_proof_is_accepted(api, O, reveal, reads):
    from halo2_vectordb_amd import verifier
    from halo2_vectordb_amd.rounds import ProverRounds, quotient_identity_holds
    from oracle import pairing as PR
    n, dim = 6, 4
    hp = _hot_path(n, dim, reads, 11, reveal, k=12).setup()
    pr = None
    try:
        d_flags = hp.keygen_flags()
        flags = d_flags.download((hp.n_cells,), dtype=np.uint8)
        d_flags.free()
        hp._witness()
        api.sync()
        m, tree = _model_of(O, hp, _rows(11, n, dim), reads)
        k = len(reads)
        assert hp.n_cells == m["advice"].shape[0] and hp.n_in == m["n_in"] and hp.n_lookup == 0
        assert np.array_equal(hp.d_stream.download((hp.n_cells, 4)), m["advice"]) and np.array_equal(flags & 1, m["selectors"])
        assert np.array_equal(hp.bp, m["break_points"]) and len(hp.bp) >= 3
        res = hp.results()
        assert np.array_equal(res[0], m["public"][0]) and TM.to_ints(res[1]) == reads and np.array_equal(res[2], m["public"][2:1 + 2 * k:2])
        if reveal == "vector":
            assert len(res) == 4 and np.array_equal(res[3].reshape(-1, 4), m["public"][1 + 2 * k:]) and np.array_equal(res[3], hp.qvec)
        else:
            assert len(res) == 3 and np.array_equal(res[2][1], MU.ZERO) and not np.array_equal(res[2][0], MU.ZERO)
        assert np.array_equal(hp.d_levels.download((16, 4)), MU.flat_levels(tree))
        pr = ProverRounds(hp).keygen()
        assert pr.keygen_report.violations() == 0, pr.keygen_report.as_dict()
        out = pr.prove(None, seed=17)
        want = TM.to_ints(m["public"])
        assert out["instances"] == want and len(want) == 1 + 2 * k + (k * dim if reveal == "vector" else 0)
        assert quotient_identity_holds(pr, out["challenges"], out["evals"], out["instances"])
        vk = verifier.VerifyingKey.from_prover(pr, out["opened"])
        assert verifier.verify(out["proof"], want, vk)
        yvk = dict(meta=_meta(pr), opened=out["opened"], fixed={name: pr.fixed[name].commits for name in FIXED}, tau_h=PR.pt_mul(PR.G2, TAU))
        assert _verify(O, api, out["proof"], {**yvk, "instances": want})
        changed = [0, 1] + ([1 + 2 * k + dim + 1] if reveal == "vector" else [2 + 2])        # the root, idx of read 0, a vector word / the empty slot's leaf
        if reveal == "leaf":
            assert want[2 + 2] == 0
        for at in changed:
            wrong = list(want)
            wrong[at] = (wrong[at] + 1) % O.R_MOD
            assert not verifier.verify(out["proof"], wrong, vk), at
    finally:
        for x in (pr, hp):
            if x is not None:
                x.free()


def test_read_after_write_and_a_stale_tree(api, O):
    """the root a batch of updates states as its new root is the root the next read proves against; the same read against the tree from
    before the batch still writes a stream, whose broken copies the Mock stage reports (a report on a finished stream)"""
    from halo2_vectordb_amd import verifier
    from halo2_vectordb_amd.pipeline import UpdateHotPath
    from halo2_vectordb_amd.rounds import ProverRounds
    n, dim, widx, reads = 6, 4, [4, 6], [6, 4, 0]
    rows, new = _rows(41, n, dim), _rows(42, 2, dim)
    up = UpdateHotPath(n, dim, 2, 13, 8, P=P, tau=TAU, vectors=rows, updates=(widx, new)).setup()
    hp = pr = stale = pr2 = None
    try:
        up._witness()
        api.sync()
        new_root = up.results()[-1]
        after = np.concatenate([rows, new[1:2]])
        after[4] = new[0]
        hp = _hot_path(n + 1, dim, reads, 0, "vector", vectors=after, levels=up.d_levels).setup()
        pr = ProverRounds(hp).keygen()
        assert pr.keygen_report.violations() == 0, pr.keygen_report.as_dict()
        out = pr.prove(None, seed=19)
        root, _idx, _leaves, vectors = hp.results()
        assert np.array_equal(root, new_root) and np.array_equal(root, O.poseidon_merkle_root(O.quantize(after, P)))
        assert np.array_equal(vectors, O.quantize(np.stack([new[1], new[0], rows[0]]), P))
        assert out["instances"][0] == TM.to_ints(new_root[None])[0]
        assert verifier.verify(out["proof"], out["instances"], verifier.VerifyingKey.from_prover(pr, out["opened"]))
        stale = _hot_path(n + 1, dim, reads, 0, "vector", vectors=after, levels=up.d_levels0).setup()
        pr2 = ProverRounds(stale).keygen()
        rep = pr2.keygen_report
        assert rep.violations() >= 1 and rep.as_dict()["copies_unequal"] >= 1, rep.as_dict()
    finally:
        for x in (pr2, stale, pr, hp, up):
            if x is not None:
                x.free()


def test_tampered_sibling_bit_and_tied_top_are_noticed(api, O):
    """the witness as it lies in HBM with one assigned sibling, one assigned bit and the top of read 1 (the cell tied to read 0's top)
    altered alone: the Mock stage reports violations for each"""
    from halo2_vectordb_amd import circuit_sym as CS
    from halo2_vectordb_amd.rounds import ProverRounds
    n, dim, reads = 6, 4, [2, 5, 2]
    hp = _hot_path(n, dim, reads, 31, "vector", k=12).setup()
    pr = ProverRounds(hp).keygen()
    try:
        assert pr.keygen_report.violations() == 0
        stream = hp.d_stream.download((hp.n_cells, 4))
        lay = CS.merkle_open_layout(len(reads), dim, 3, True)
        cm = pr.circuit
        blk = lay["n_in"] + lay["per_read"]
        tied = [c for c in range(blk, blk + lay["per_read"]) if lay["n_in"] <= cm.copy_of[c] < blk]
        assert len(tied) == 1 and np.array_equal(stream[tied[0]], stream[cm.copy_of[tied[0]]])
        one = O.fr_from_ints([1])
        d_flags = api.DeviceBuffer(hp.n_cells)
        try:
            d_flags.upload(np.asarray(cm.gate).astype(np.uint8))
            assert pr.mock_check(d_flags).violations() == 0          # the witness as it lies in HBM, not emitted again
            for cell in (lay["sibs"] + 1 * 3 + 1, lay["bits"] + 2 * 3, tied[0]):
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
    """col_shard: every rank reads the same tree and stores the cells of its own columns"""
    one = _run(1, "merkle_read", str(tmp_path / "p1.bin"), 0)
    assert one["every_rank_wrote_the_same_bytes"] and one["quotient_identity_at_x_holds"] and one["mock_prover_violations"] == 0
    rep = _run(2, "merkle_read", str(tmp_path / "p2.bin"), 29583)
    assert rep["world"] == 2 and rep["every_rank_wrote_the_same_bytes"] and rep["quotient_identity_at_x_holds"]
    assert open(tmp_path / "p2.bin", "rb").read() == open(tmp_path / "p1.bin", "rb").read()
    assert rep["sha256"] == one["sha256"] and rep["n_instances"] == one["n_instances"] == 1 + 2 * 4 + 4 * 4
