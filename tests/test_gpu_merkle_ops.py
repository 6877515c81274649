"""Deletes and tree growth proved against the committed root (pipeline.UpdateHotPath(kinds, grow); vdb_merkle_tree_grow_dev,
vdb_wit_merkle_update_ops*) on the GPU.  The streams are tests/merkle_ops_model.py's, bit for bit — advice, flags, size, public values,
the tree after the batch (tests/test_merkle_ops_cpu.py holds that model against the oracle first); the plain call is the ops call with
no deletes and no growth, bytes and launches; host and device forms, rank windows, the launch count, refused arguments, the Mock stage,
the whole proof, changed instances, tampered cells, and reads and a second batch chained to the grown tree."""
import ctypes

import numpy as np
import pytest

import merkle_ops_model as MO
import merkle_update_model as MU
import topk_model as TM
from test_gpu_batch_query import _dev
from test_gpu_merkle_update import P, TAU, _rows
from test_gpu_sweep import _check_window, _windowed

pytestmark = pytest.mark.gpu
W, D = 0, 1
# n = 5 (d = 3): a slot written then deleted (2, 2), a slot and its sibling (4, 5), an empty slot deleted (7), the last real slot
SHAPE1 = dict(kinds=[W, D, W, D, D, W, D], idx={0: [2, 2, 4, 5, 7, 0, 4], 2: [2, 2, 4, 5, 7, 9, 31]})


@pytest.fixture(scope="module")
def api():
    from halo2_vectordb_amd import api as a
    a.init(0)
    return a


def _size(api, n, dim, kinds, grow):
    from halo2_vectordb_amd._lib import check
    cells, n_in = ctypes.c_uint64(), ctypes.c_uint64()
    k = np.ascontiguousarray(kinds, dtype=np.uint8)
    check(api.init().vdb_wit_merkle_update_ops_size(n, dim, len(kinds), api._p(k), grow, ctypes.byref(cells), ctypes.byref(n_in)))
    return cells.value, n_in.value


def _ops_dev(api, levels, n, dim, new, idx, kinds, grow, profile=False, plain=False):
    """vdb_wit_merkle_update_ops_dev (plain: vdb_wit_merkle_update_dev) into poisoned buffers
    -> (stream, flags, public, levels after[, launches per kernel of a second, profiled run])"""
    from halo2_vectordb_amd._lib import check
    lib = api.init()
    m = len(idx)
    cells, _ = _size(api, n, dim, kinds, grow)
    idx, kinds = np.ascontiguousarray(idx, dtype=np.uint64), np.ascontiguousarray(kinds, dtype=np.uint8)
    up = []
    try:
        d_lv = _dev(api, up, levels)
        d_new = _dev(api, up, new) if new.shape[0] else None
        d_adv, d_sel, d_pub = api.DeviceBuffer(cells * 32), api.DeviceBuffer(cells), api.DeviceBuffer((3 * m + 2) * 32)
        up += [d_adv, d_sel, d_pub]
        check(lib.vdb_memset_dev(d_adv.ptr, 0xA5, ctypes.c_size_t(cells * 32)))
        check(lib.vdb_memset_dev(d_sel.ptr, 0xFF, ctypes.c_size_t(cells)))
        p_new = d_new.ptr if d_new is not None else None
        if plain:
            run = lambda: check(lib.vdb_wit_merkle_update_dev(d_lv.ptr, n, dim, p_new, api._p(idx), m, d_adv.ptr, d_sel.ptr, d_pub.ptr))
        else:
            run = lambda: check(lib.vdb_wit_merkle_update_ops_dev(d_lv.ptr, n, dim, grow, p_new, api._p(idx), api._p(kinds), m, d_adv.ptr, d_sel.ptr, d_pub.ptr))
        run()
        api.sync()
        out = [d_adv.download((cells, 4)), d_sel.download((cells,), dtype=np.uint8), d_pub.download((3 * m + 2, 4)), d_lv.download(levels.shape)]
        if profile:
            d_lv.upload(levels)
            api.profile_begin(deferred=True)
            run()
            api.sync()
            out.append({name: int(v["launches"]) for name, v in api.profile_end().items()})
        return out
    finally:
        for b in up:
            b.free()


def _case(api, O, n, dim, idx, kinds, grow, seed):
    """-> (tree before growth (device layout), grown tree (device layout), new vectors, the model, the model's tree after the batch)"""
    db = O.quantize(_rows(seed, n, dim), P)
    new = O.quantize(_rows(seed + 1, max(kinds.count(W), 1), dim), P)[: kinds.count(W)]
    small = MU.build_tree(O, db)
    tree = MO.grow_tree(O, small, grow)
    grown = MU.flat_levels(tree)
    m = MO.ops_model(O, tree, idx, kinds, new, grow)
    return MU.flat_levels(small), grown, new, m, tree


# ---------------------------------------------------------------------------------------------------------------- streams and tree
@pytest.mark.parametrize("n,dim,grow", [(5, 3, 0), (5, 3, 2), (5, 4, 0), (5, 4, 2), (1, 3, 1)])
def test_entry_points_write_the_models_stream_and_leave_the_models_tree(api, O, n, dim, grow):
    idx, kinds = (SHAPE1["idx"][grow], SHAPE1["kinds"]) if n == 5 else ([1, 0], [W, D])
    small, grown, new, m, tree = _case(api, O, n, dim, idx, kinds, grow, 40 + dim)
    assert np.array_equal(api.merkle_tree_grow(small, n, grow), grown), "vdb_merkle_tree_grow_dev"
    cells, n_in = _size(api, n, dim, kinds, grow)
    assert cells == m["advice"].shape[0] and n_in == m["n_in"]
    stream, flags, pub, levels1 = _ops_dev(api, grown, n, dim, new, idx, kinds, grow)
    bad = np.flatnonzero((stream != m["advice"]).any(axis=1))
    assert bad.size == 0, f"first differing advice cells {bad[:5]} of {cells}"
    assert np.array_equal(flags & 1, m["selectors"]) and not (flags & ~np.uint8(3)).any()
    assert (flags[m["constants"]] == 2).all() and not flags[:n_in].any(), "load_constant cells carry the constant flag, inputs none"
    assert np.array_equal(pub, m["public"])
    assert np.array_equal(levels1, MU.flat_levels(tree)), "the tree after the batch is the sequential one"
    for j, kd in enumerate(kinds):
        assert np.array_equal(pub[3 + 3 * j], MU.ZERO) == bool(kd)
    host = api.wit_merkle_update(grown, n, new, idx, selectors=True, kinds=kinds, grow=grow)
    assert np.array_equal(host["stream"], stream) and np.array_equal(host["flags"], flags) and np.array_equal(host["public"], pub)
    assert np.array_equal(host["levels"], levels1) and host["input_cells"] == n_in


def test_plain_call_is_the_ops_call_without_deletes_or_growth(api, O):
    n, dim, idx = 6, 5, [4, 5, 6, 4, 1]
    kinds = [W] * len(idx)
    small, grown, new, m, tree = _case(api, O, n, dim, idx, kinds, 0, 50)
    assert np.array_equal(small, grown)
    a = _ops_dev(api, small, n, dim, new, idx, kinds, 0, profile=True, plain=True)
    b = _ops_dev(api, small, n, dim, new, idx, kinds, 0, profile=True)
    for x, y in zip(a[:4], b[:4]):
        assert x.tobytes() == y.tobytes()
    assert a[4] == b[4] == dict(k_mku_touchers=1, k_mk_leaf_states=1, k_mku_level=3, k_mku_writeback=1, k_mku_inputs=1, k_mk_leaf_trace=1,
                                k_mku_level_trace=1, k_mku_index=1), (a[4], b[4])
    want = MU.update_model(O, MU.build_tree(O, O.quantize(_rows(50, n, dim), P)), idx, new)
    assert np.array_equal(a[0], want["advice"]) and np.array_equal(a[2], want["public"])


# ---------------------------------------------------------------------------------------------------------------- growth
@pytest.mark.parametrize("grow", [1, 3])
def test_tree_growth_is_the_models_and_leaves_its_input(api, O, grow):
    from halo2_vectordb_amd._lib import check
    lib = api.init()
    n, dim = 5, 3
    db = O.quantize(_rows(60, n, dim), P)
    small = api.merkle_tree_build(db)
    want = MU.flat_levels(MO.grow_tree(O, MU.build_tree(O, db), grow))
    up = []
    try:
        d_small = _dev(api, up, small)
        d_out = api.DeviceBuffer(want.nbytes + 64)
        up.append(d_out)
        check(lib.vdb_memset_dev(d_out.ptr, 0xA5, ctypes.c_size_t(want.nbytes + 64)))
        check(lib.vdb_merkle_tree_grow_dev(d_small.ptr, n, grow, d_out.ptr))
        api.sync()
        got = d_out.download(want.shape)
        bad = np.flatnonzero((got != want).any(axis=1))
        assert bad.size == 0, f"entries {bad[:8]} of {want.shape[0]}"
        assert (d_out.download((64,), dtype=np.uint8, offset=want.nbytes) == 0xA5).all(), "2 lp 2^g entries, not one more"
        assert np.array_equal(d_small.download(small.shape), small), "the input tree is only read"
    finally:
        for b in up:
            b.free()


def test_growing_four_by_one_and_inserting_the_fifth_is_the_tree_of_five(api, O):
    dim = 4
    five = O.quantize(_rows(61, 5, dim), P)
    grown = api.merkle_tree_grow(api.merkle_tree_build(five[:4]), 4, 1)
    out = api.wit_merkle_update(grown, 4, five[4:], [4], grow=1)
    assert np.array_equal(out["levels"], api.merkle_tree_build(five))
    assert np.array_equal(out["public"][0], O.poseidon_merkle_root(five[:4])) and np.array_equal(out["public"][-1], O.poseidon_merkle_root(five))


# ---------------------------------------------------------------------------------------------------------------- launches, windows, refusals
def test_launch_count_depends_on_neither_the_batch_size_nor_the_kinds(api, O):
    n, dim, grow = 5, 3, 1
    db = O.quantize(_rows(62, n, dim), P)
    grown = api.merkle_tree_grow(api.merkle_tree_build(db), n, grow)
    rng = np.random.default_rng(62)
    counts = {}
    for name, m, kind in (("one_write", 1, W), ("64_writes", 64, W), ("64_deletes", 64, D), ("one_delete", 1, D)):
        kinds = [kind] * m
        new = O.quantize(_rows(63, max(kinds.count(W), 1), dim), P)[: kinds.count(W)]
        counts[name] = _ops_dev(api, grown, n, dim, new, rng.integers(0, 16, size=m), kinds, grow, profile=True)[4]
    assert all(c == counts["one_write"] for c in counts.values()), counts
    assert counts["one_write"] == dict(k_mku_touchers=1, k_mk_leaf_states=1, k_mku_level=4, k_mku_grow_trace=1, k_mku_writeback=1, k_mku_inputs=1,
                                       k_mk_leaf_trace=1, k_mku_level_trace=1, k_mku_index=1), counts["one_write"]


def test_two_windowed_calls_write_the_bytes_of_one(api, O):
    from halo2_vectordb_amd._lib import check
    lib = api.init()
    n, dim, grow = 5, 3, 2
    idx, kinds = SHAPE1["idx"][grow], SHAPE1["kinds"]
    _small, grown, new, m, tree = _case(api, O, n, dim, idx, kinds, grow, 64)
    want, pub, levels1 = m["advice"], m["public"], MU.flat_levels(tree)
    cells, n_in = want.shape[0], m["n_in"]
    lk = np.zeros((0, 4), dtype=np.uint64)
    uidx, ukinds = np.ascontiguousarray(idx, dtype=np.uint64), np.ascontiguousarray(kinds, dtype=np.uint8)
    up = []
    try:
        d_new, d_pub = _dev(api, up, new), _dev(api, up, np.zeros_like(pub))
        g = m["growth"]
        # inside the inputs, between R_0 and Z_0, inside an R hash, at a delete's zero cell, near the end
        for cut in (n_in - 3, g["z0"], g["r"][0] + 2256 + 7, m["regions"][1]["new_leaf"], cells - 2):
            halves = []
            for window in ((0, cut, 0, 0), (cut, cells, 0, 0)):
                d_lv = _dev(api, up, grown)                         # every call starts from the tree before the batch
                run = lambda d_adv, d_lk: check(lib.vdb_wit_merkle_update_ops_dev(d_lv.ptr, n, dim, grow, d_new.ptr, api._p(uidx), api._p(ukinds),
                                                                                   len(idx), d_adv.ptr, None, d_pub.ptr))
                g_adv, _ = _windowed(api, lib, check, want, lk, window, run)
                _check_window(want, lk, g_adv, lk, window, (cut, window))
                assert np.array_equal(d_pub.download(pub.shape), pub) and np.array_equal(d_lv.download(grown.shape), levels1), (cut, window)
                halves.append(g_adv)
            assert np.array_equal(np.concatenate([halves[0][:cut], halves[1][cut:]]), want), cut
    finally:
        for b in up:
            b.free()


def test_refused_arguments_return_the_error_code_and_launch_nothing(api, O):
    from halo2_vectordb_amd._lib import check
    lib = api.init()
    db, new = O.quantize(_rows(65, 6, 4), P), O.quantize(_rows(66, 2, 4), P)
    grown = api.merkle_tree_grow(api.merkle_tree_build(db), 6, 1)
    up = []
    try:
        d_lv, d_new = _dev(api, up, grown), _dev(api, up, new)
        d_out = api.DeviceBuffer(1 << 16)
        up.append(d_out)
        check(lib.vdb_memset_dev(d_out.ptr, 0xA5, ctypes.c_size_t(1 << 16)))
        api.sync()
        api.profile_begin(deferred=True)
        # a kind of 2, d + g > 30, d + g == 0, an index >= lp 2^g, no update, too many updates
        for n, grow, idx, kinds in ((6, 1, [1, 2], [0, 2]), (6, 28, [1, 2], [0, 0]), (1, 0, [0, 0], [0, 1]), (6, 1, [1, 16], [0, 1]),
                                    (6, 1, [], []), (6, 1, [1] * 4097, [1] * 4097)):
            uidx, uk = np.ascontiguousarray(idx + [0], dtype=np.uint64), np.ascontiguousarray(kinds + [0], dtype=np.uint8)
            with pytest.raises(api.VdbError) as e:
                check(lib.vdb_wit_merkle_update_ops_dev(d_lv.ptr, n, 4, grow, d_new.ptr, api._p(uidx), api._p(uk), len(idx), d_out.ptr, None,
                                                        d_out.at(1 << 15)))
            assert e.value.code == -3, (n, grow, idx[:4], kinds[:4])
        with pytest.raises(api.VdbError) as e:
            check(lib.vdb_merkle_tree_grow_dev(d_lv.ptr, 6, 28, d_out.ptr))
        assert e.value.code == -3
        api.sync()
        assert api.profile_end() == {}
        assert (d_out.download((1 << 16,), dtype=np.uint8) == 0xA5).all() and np.array_equal(d_lv.download(grown.shape), grown)
    finally:
        for b in up:
            b.free()


# ---------------------------------------------------------------------------------------------------------------- the proof
N, DIM, GROW = 5, 3, 1
IDX, KINDS = [2, 2, 9, 4, 7], [W, D, W, D, D]


@pytest.fixture(scope="module")
def proved(api, O):
    """one UpdateHotPath(kinds, grow) with its keys, its proof and the model of its batch, shared by the tests below"""
    from halo2_vectordb_amd.pipeline import UpdateHotPath
    from halo2_vectordb_amd.rounds import ProverRounds
    hp = UpdateHotPath(N, DIM, len(IDX), 13, 8, P=P, tau=TAU, vectors=_rows(70, N, DIM), updates=(IDX, _rows(71, KINDS.count(W), DIM)), kinds=KINDS,
                       grow=GROW).setup()
    pr = ProverRounds(hp).keygen()
    hp._witness()
    api.sync()
    stream = hp.d_stream.download((hp.n_cells, 4))
    out = pr.prove(None, seed=19)
    tree = MO.grow_tree(O, MU.build_tree(O, O.quantize(_rows(70, N, DIM), P)), GROW)
    m = MO.ops_model(O, tree, IDX, KINDS, hp.qvec, GROW)
    yield dict(hp=hp, pr=pr, out=out, m=m, tree=tree, stream=stream)
    pr.free()
    hp.free()


def test_hot_path_proves_the_models_batch(api, O, proved):
    from halo2_vectordb_amd import verifier
    from halo2_vectordb_amd.rounds import quotient_identity_holds
    hp, pr, out, m = proved["hp"], proved["pr"], proved["out"], proved["m"]
    assert (hp.lp, hp.depth, hp.w, hp.n_lookup) == (16, 4, 2, 0) and hp.n_cells == m["advice"].shape[0] and hp.n_in == m["n_in"]
    assert pr.keygen_report.violations() == 0, pr.keygen_report.as_dict()
    assert pr.mock_check().violations() == 0
    assert np.array_equal(proved["stream"], m["advice"])
    old_root, indices, old_leaves, new_leaves, new_root = hp.results()
    assert np.array_equal(np.concatenate([old_root[None], np.stack([indices, old_leaves, new_leaves], axis=1).reshape(-1, 4), new_root[None]]), m["public"])
    assert np.array_equal(hp.d_levels.download((32, 4)), MU.flat_levels(proved["tree"])), "the updated, grown tree stays on the device"
    assert np.array_equal(old_root, O.poseidon_merkle_root(O.quantize(_rows(70, N, DIM), P))), "the old root is the root before the growth"
    want = TM.to_ints(m["public"])
    assert out["instances"] == want and len(want) == 3 * len(IDX) + 2
    assert quotient_identity_holds(pr, out["challenges"], out["evals"], out["instances"])
    vk = verifier.VerifyingKey.from_prover(pr, out["opened"])
    assert verifier.verify(out["proof"], want, vk)
    nonzero_delete = list(want)                               # a delete claimed to leave something behind
    assert nonzero_delete[1 + 3 * 1 + 2] == 0
    nonzero_delete[1 + 3 * 1 + 2] = 1
    assert not verifier.verify(out["proof"], nonzero_delete, vk)
    wrong_old_root = list(want)
    wrong_old_root[0] = (wrong_old_root[0] + 1) % O.R_MOD
    assert not verifier.verify(out["proof"], wrong_old_root, vk)


def test_tampered_growth_root_and_tampered_delete_zero_are_noticed(api, O, proved):
    hp, pr, m = proved["hp"], proved["pr"], proved["m"]
    hp._witness()
    api.sync()
    stream = hp.d_stream.download((hp.n_cells, 4))
    assert np.array_equal(stream, proved["stream"])
    one = O.fr_from_ints([1])
    d_flags = api.DeviceBuffer(hp.n_cells)
    try:
        d_flags.upload(np.asarray(pr.circuit.gate).astype(np.uint8))
        assert pr.mock_check(d_flags).violations() == 0              # the witness as it lies in HBM, not emitted again
        for cell in (m["growth"]["r0"], m["growth"]["z0"], m["regions"][1]["new_leaf"], m["regions"][4]["new_leaf"]):
            hp.d_stream.upload(O.fr_add(stream[cell:cell + 1], one), offset=cell * 32)
            rep = pr.mock_check(d_flags)
            hp.d_stream.upload(np.ascontiguousarray(stream[cell:cell + 1]), offset=cell * 32)
            assert rep.violations() >= 1, (cell, rep.as_dict())
        assert pr.mock_check(d_flags).violations() == 0
    finally:
        d_flags.free()


def test_reads_and_a_second_batch_chain_to_the_grown_tree(api, O, proved):
    from halo2_vectordb_amd import verifier
    from halo2_vectordb_amd.pipeline import ReadHotPath, UpdateHotPath
    from halo2_vectordb_amd.rounds import ProverRounds
    hp, m, tree = proved["hp"], proved["m"], proved["tree"]
    new_root = TM.to_ints(m["public"])[-1]
    made = []
    try:
        # leaf mode: the deleted slot 2 and the written slot 9 of the 16-leaf tree, against the update's new root
        rd = ReadHotPath(hp.lp, DIM, 2, 13, 8, P=P, tau=TAU, levels=hp.d_levels, reads=[2, 9], reveal="leaf").setup()
        made.append(rd)
        pr = ProverRounds(rd).keygen()
        made.append(pr)
        assert pr.keygen_report.violations() == 0
        out = pr.prove(None, seed=20)
        assert out["instances"][0] == new_root and out["instances"][1:5] == [2, 0, 9, TM.to_ints(tree[0][9][None])[0]]
        assert verifier.verify(out["proof"], out["instances"], verifier.VerifyingKey.from_prover(pr, out["opened"]))
        # vector mode: the vector inserted past the old lp = 8
        rows = np.zeros((hp.lp, DIM))
        rows[9] = _rows(71, KINDS.count(W), DIM)[1]
        rv = ReadHotPath(hp.lp, DIM, 1, 13, 8, P=P, tau=TAU, vectors=rows, levels=hp.d_levels, reads=[9]).setup()
        made.append(rv)
        rv._witness()
        api.sync()
        root, indices, leaves, vectors = rv.results()[:4]
        assert TM.to_ints(root[None])[0] == new_root and np.array_equal(leaves[0], tree[0][9]) and np.array_equal(np.asarray(vectors).reshape(-1, 4), hp.qvec[1])
        # a second batch from the grown tree: its old root is the first's new root
        up2 = UpdateHotPath(hp.lp, DIM, 2, 13, 8, P=P, tau=TAU, levels=hp.d_levels, updates=([9, 15], _rows(72, 1, DIM)), kinds=[D, W]).setup()
        made.append(up2)
        pr2 = ProverRounds(up2).keygen()
        made.append(pr2)
        assert pr2.keygen_report.violations() == 0
        out2 = pr2.prove(None, seed=21)
        m2 = MO.ops_model(O, tree, [9, 15], [D, W], up2.qvec, 0)
        assert out2["instances"] == TM.to_ints(m2["public"]) and out2["instances"][0] == new_root
        assert verifier.verify(out2["proof"], out2["instances"], verifier.VerifyingKey.from_prover(pr2, out2["opened"]))
    finally:
        for x in reversed(made):
            x.free()
