"""The witness side of the committed database beyond its first workgroup (witness.hip: mku_emit's kernels under vdb_wit_merkle_update*_dev
and inside vdb_wit_ann_update_dev / vdb_wit_ann_delete_dev, the index-root frame AnnFrame at K = 300 and under the audit layouts at K = 70,
chain_fold_wave past one prefetch chunk), bit for bit against the CPU models and the oracle; there is no tolerance anywhere.  Every case
first asserts on the host (tests/test_witness_shapes_cpu.py, from witness.hip's launch formulas restated in witness_shapes_model) that its
shape reaches the block, wavefront, LDS trip or chunk it is there for: a shape that stops reaching its case fails.  Deliberately unreached:
the second block of k_annd_public, which needs 64 deletes in one call (8 M cells)."""
import ctypes

import numpy as np
import pytest

import merkle_update_model as MU
import topk_model as TM
import witness_shapes_model as WS
from test_gpu_ann_delete import _delete_dev
from test_gpu_ann_update import _update_dev
from test_gpu_batch_query import _dev
from test_gpu_merkle_ops import _ops_dev
from test_gpu_merkle_update import _apply, _dev_call, _size
from test_gpu_sweep import _check_window, _windowed
from test_gpu_witness import assert_streams
from test_witness_shapes_cpu import (ANN_UPDATES, ANND, KM_L, KMEANS, P, PATH_CASES, ann_case, ann_reaches, kmeans_case, kmeans_reaches, last_block_model,
                                     path_case, path_reaches, rows)

pytestmark = pytest.mark.gpu
NO_LOOKUP = np.zeros((0, 4), dtype=np.uint64)


@pytest.fixture(scope="module")
def api():
    from halo2_vectordb_amd import api as a
    a.init(0)
    return a


def _same_stream(stream, want, what=""):
    assert stream.shape == want.shape
    bad = np.flatnonzero((stream != want).any(axis=1))
    assert bad.size == 0, f"{what}first differing advice cells {bad[:5]} of {stream.shape[0]}"


# ---------------------------------------------------------------------------------------------------------------- A: path updates
@pytest.mark.parametrize("name", sorted(PATH_CASES))
def test_path_updates_past_one_block_are_the_models(api, O, name):
    path_reaches(name)
    s = path_case(O, name)
    m, n, dim, grow, idx, kinds = s["m"], s["n"], s["dim"], s["grow"], s["idx"], s["kinds"]
    assert np.array_equal(api.merkle_tree_build(s["db"]), s["small"]) and np.array_equal(api.merkle_tree_grow(s["small"], n, grow), s["grown"])
    if kinds is None:
        cells, n_in = _size(api, n, dim, len(idx))
        stream, flags, pub, levels1 = _dev_call(api, s["grown"], n, s["new"], idx)
    else:
        from test_gpu_merkle_ops import _size as _ops_size
        cells, n_in = _ops_size(api, n, dim, kinds, grow)
        stream, flags, pub, levels1 = _ops_dev(api, s["grown"], n, dim, s["new"], idx, kinds, grow)
    assert cells == m["advice"].shape[0] and n_in == m["n_in"]
    _same_stream(stream, m["advice"])
    assert np.array_equal(flags & 1, m["selectors"]) and not (flags & ~np.uint8(3)).any() and not flags[:n_in].any()
    assert pub.shape == (3 * len(idx) + 2, 4) and np.array_equal(pub, m["public"])
    assert np.array_equal(levels1, s["after"]), "the tree after the batch is the sequential one"
    if kinds is None:
        after = _apply(s["db"], MU.padded(n)[0], idx, s["new"])
        assert np.array_equal(levels1, api.merkle_tree_build(after)), "... and vdb_merkle_tree_build_dev of the updated database"
    else:
        assert (flags[m["constants"]] == 2).all(), "load_constant cells carry the constant flag"
        for j, kd in enumerate(kinds):
            assert np.array_equal(pub[3 + 3 * j], MU.ZERO) == bool(kd)
    host = api.wit_merkle_update(s["grown"], n, s["new"], idx, selectors=True, kinds=kinds, grow=grow)
    assert np.array_equal(host["stream"], stream) and np.array_equal(host["flags"], flags) and np.array_equal(host["public"], pub)
    assert np.array_equal(host["levels"], levels1) and host["input_cells"] == n_in


def _all_bytes(api, buf, nbytes, byte, lo=0, chunk=1 << 26):
    """every byte of [lo, nbytes) of the device buffer is `byte` (read back a piece at a time)"""
    while lo < nbytes:
        size = min(chunk, nbytes - lo)
        if not (buf.download((size,), dtype=np.uint8, offset=lo) == byte).all():
            return False
        lo += size
    return True


def test_max_batch_values(api, O):
    """4096 updates, the most one call admits: the only shape that fills k_mku_touchers' LDS table to its last entry.  The stream (46 M
    cells) is allocated and poisoned in full, stored through a rank window that holds the last update's block alone, and that block is the
    one-update model's on the tree the values-only walk leaves after the 4095 updates before it; public values and tree are the walk's"""
    from halo2_vectordb_amd._lib import check
    lib = api.init()
    m, n, dim = WS.MAX_UPDATES, 2, 1
    idx = [int(i) for i in np.random.default_rng(m).integers(0, 2, size=m)]
    f = WS.path_update_facts(idx, None, 1, dim)
    assert f["fill_trips"] == 16 and f["touchers_blocks"] == 16 and f["index_blocks"] == 64 and set(idx) == {0, 1}
    db, new = O.quantize(rows(n, n, dim), P), O.quantize(rows(n + 1, m, dim), P)
    block, gates, public, after = last_block_model(O, db, idx, new)
    cells, n_in = _size(api, n, dim, m)
    lo = cells - block.shape[0]
    assert n_in == m * (dim + 3) and (cells - n_in) == m * block.shape[0] and cells > 46_000_000
    levels0 = api.merkle_tree_build(db)
    uidx = np.ascontiguousarray(idx, dtype=np.uint64)
    up = []
    try:
        d_lv, d_new = _dev(api, up, levels0), _dev(api, up, new)
        d_adv, d_sel, d_pub = api.DeviceBuffer(cells * 32), api.DeviceBuffer(cells), api.DeviceBuffer((3 * m + 2) * 32)
        up += [d_adv, d_sel, d_pub]
        check(lib.vdb_memset_dev(d_adv.ptr, 0xA5, ctypes.c_size_t(cells * 32)))
        check(lib.vdb_memset_dev(d_sel.ptr, 0xFF, ctypes.c_size_t(cells)))
        with api.wit_window(adv=(lo, cells), lookup=(0, 0)):
            check(lib.vdb_wit_merkle_update_dev(d_lv.ptr, n, dim, d_new.ptr, api._p(uidx), m, d_adv.ptr, d_sel.ptr, d_pub.ptr))
        api.sync()
        _same_stream(d_adv.download(block.shape, offset=lo * 32), block, "the last update's block: ")
        flags = d_sel.download((cells,), dtype=np.uint8)
        assert np.array_equal(flags[lo:] & 1, gates) and not (flags[lo:] & ~np.uint8(3)).any() and (flags[:lo] == 0xFF).all()
        assert _all_bytes(api, d_adv, lo * 32, 0xA5), "a cell outside the window was stored"
        pub = d_pub.download((3 * m + 2, 4))
        bad = np.flatnonzero((pub != public).any(axis=1))
        assert bad.size == 0, f"first differing public values {bad[:5]} of {3 * m + 2}"
        assert np.array_equal(d_lv.download(levels0.shape), after)
        # one update more is refused before anything is launched
        d_out = api.DeviceBuffer(1 << 16)
        up.append(d_out)
        check(lib.vdb_memset_dev(d_out.ptr, 0xA5, ctypes.c_size_t(1 << 16)))
        d_new1 = _dev(api, up, np.concatenate([new, new[:1]]))
        uidx1 = np.ascontiguousarray(idx + [0], dtype=np.uint64)
        api.sync()
        api.profile_begin(deferred=True)
        with pytest.raises(api.VdbError) as e:
            check(lib.vdb_wit_merkle_update_dev(d_lv.ptr, n, dim, d_new1.ptr, api._p(uidx1), m + 1, d_out.ptr, None, d_out.at(1 << 15)))
        assert e.value.code == -3                                              # VDB_ERR_ARG
        api.sync()
        assert api.profile_end() == {}
        assert (d_out.download((1 << 16,), dtype=np.uint8) == 0xA5).all() and np.array_equal(d_lv.download(levels0.shape), after)
    finally:
        for b in up:
            b.free()


# ---------------------------------------------------------------------------------------------------------------- B: the index-root batches
def _frame_flags_are_the_models(flags, m, K):
    """outside the blocks between D and F the flag bytes are the model's"""
    r = m["regions"]
    outside = np.ones(flags.shape[0], dtype=bool)
    outside[r["update"]:r["new_roots"]] = False
    diff = np.flatnonzero((flags != m["flags"]) & outside)
    assert diff.size == 0 and not flags[:K + 2].any(), (diff[:8], r)
    assert np.array_equal(flags & 1, m["selectors"]) and not (flags & ~np.uint8(3)).any()


def _update_is_the_models(api, s):
    """vdb_wit_ann_update_dev against ann_update_model: stream, flags, public values, tree; the update block's bytes are those of the
    block emitted alone (where the model skipped its flag pass, that is what holds the block's flags); the host form"""
    m, K = s["m"], s["K"]
    stream, flags, pub, levels1 = _update_dev(api, s)
    _same_stream(stream, m["advice"], f"blocks {m['regions']}: ")
    _frame_flags_are_the_models(flags, m, K)
    r = m["regions"]
    alone = api.wit_merkle_update(s["grown"], s["n_c"], s["new"], s["slots"], selectors=True, grow=s["grow"])
    assert np.array_equal(flags[r["update"]:r["new_roots"]], alone["flags"]) and np.array_equal(stream[r["update"]:r["new_roots"]], alone["stream"])
    assert np.array_equal(pub, m["public"]) and pub.shape[0] == 3 * len(s["slots"]) + 3
    assert np.array_equal(levels1, s["after"]) and np.array_equal(levels1, alone["levels"])
    host = api.wit_ann_update(s["grown"], s["ix"]["roots"], s["c"], s["n_c"], s["new"], s["slots"], grow=s["grow"], selectors=True)
    assert np.array_equal(host["stream"], stream) and np.array_equal(host["flags"], flags) and np.array_equal(host["public"], pub)
    assert np.array_equal(host["levels"], levels1) and host["input_cells"] == K + 2 and host["update_base"] == r["update"]
    return stream, flags


def test_index_update_past_64_path_updates(api, O):
    """annu_m85: block 1 of k_annu_public writes index_root_new; mku_emit runs past 64 updates at a base that is not 0"""
    ann_reaches("annu_m85")
    s = ann_case(O, "annu_m85")
    assert s["m"]["regions"]["update"] > 0
    _update_is_the_models(api, s)


def test_index_delete_past_64_path_updates(api, O):
    """annd_m33: 66 path updates, carried leaves and emptied slots alternating into block 1 of k_mku_index; three halvings, so block S"""
    ann_reaches(ANND[0])
    s = ann_case(O, ANND[0])
    m, K = s["m"], s["K"]
    assert m["s"] == 3 and len(m["update"]["carried"]) == len(m["update"]["constants"]) == 33
    stream, flags, pub, levels1 = _delete_dev(api, s)
    _same_stream(stream, m["advice"], f"blocks {m['regions']}: ")
    _frame_flags_are_the_models(flags, m, K)
    # inside E' and S (the model skipped its flag pass there): the gate bits above, the single cells below, and one flag pattern for every
    # node hash, wherever it lies: that of the node hashes of a path update emitted alone
    r, u = m["regions"], m["update"]
    depth = MU.padded(s["n_c"])[1]
    hashes = [r["update"] + lv + off for reg in u["regions"] for lv in reg["levels"] for off in (20, 20 + 4506 + 16)]
    hashes += [r["shrink"] + 2 + h * 4506 for h in range(depth - 1 + m["s"])]
    assert len(hashes) == 2 * depth * 66 + depth - 1 + 3
    alone = api.wit_merkle_update(s["before"], s["n_c"], np.zeros((0, 1, 4), dtype=np.uint64), [0], selectors=True, kinds=[1])
    pattern = alone["flags"][alone["input_cells"] + 1 + 20:][:4506]
    assert (pattern & 2).any() and all(np.array_equal(flags[h:h + 4506], pattern) for h in hashes)
    assert not flags[[r["update"] + x for x in u["carried"]]].any(), "a carried leaf is a plain witness cell"
    assert (flags[[r["update"] + x for x in u["constants"]]] == 2).all()
    assert flags[r["shrink"]] == 0 and flags[r["shrink"] + 1] == 2
    assert np.array_equal(pub, m["public"]) and pub.shape[0] == 4 * 33 + 3
    assert np.array_equal(levels1, s["after"])
    host = api.wit_ann_delete(s["before"], s["ix"]["roots"], s["c"], s["n_c"], s["dim"], s["slots"], selectors=True)
    assert np.array_equal(host["stream"], stream) and np.array_equal(host["flags"], flags) and np.array_equal(host["public"], pub)
    assert np.array_equal(host["levels"], levels1) and host["shrink_base"] == r["shrink"] and host["shrink"] == 3


# ---------------------------------------------------------------------------------------------------------------- C: the frame at K = 300
@pytest.mark.parametrize("name", ["K300_c0", "K300_c299"])
def test_frame_at_300_clusters_is_the_models_whole_stream(api, O, name):
    ann_reaches(name)
    s = ann_case(O, name)
    stream, flags = _update_is_the_models(api, s)
    if name == "K300_c0":                                     # -1/259 from the table, -1/260 through the inverse list
        b = s["m"]["regions"]["indicator"]
        for j in (WS.SMALL_INV - 1, WS.SMALL_INV):
            cells, gates, z = TM.is_equal(0, j)
            at = b + WS.indicator_off(j)
            assert z == 0 and np.array_equal(stream[at:at + 12], TM.to_limbs(cells)) and np.array_equal(flags[at:at + 12] & 1, np.asarray(gates, dtype=np.uint8))
            assert TM.to_ints(stream[b + WS.indicator_inverse(j)][None])[0] == pow(-j % TM.R, -1, TM.R)


def test_frame_at_300_clusters_under_rank_windows(api, O):
    """two calls per cut write the bytes of one: at the first inverse cell that goes through the inverse list, so that it opens the
    second window; one cell in front of it; at the edge between blocks 0 and 1 of k_annu_new_roots"""
    from halo2_vectordb_amd._lib import check
    lib = api.init()
    s = ann_case(O, "K300_c0")
    m, K = s["m"], s["K"]
    want, pub, r = m["advice"], m["public"], m["regions"]
    cells = want.shape[0]
    deferred = r["indicator"] + WS.indicator_inverse(WS.SMALL_INV)
    assert r["indicator"] == K + 2 and deferred < r["select"] and r["new_roots"] + 8 * 64 < r["sponge_new"]
    idx = np.ascontiguousarray(s["slots"], dtype=np.uint64)
    up = []
    try:
        d_new, d_roots, d_pub = _dev(api, up, s["new"]), _dev(api, up, s["ix"]["roots"]), _dev(api, up, np.zeros_like(pub))
        for cut in (deferred, deferred - 1, r["new_roots"] + 8 * 64):
            halves = []
            for window in ((0, cut, 0, 0), (cut, cells, 0, 0)):
                d_lv = _dev(api, up, s["grown"])                    # every call starts from the tree before the batch
                run = lambda d_adv, d_lk: check(lib.vdb_wit_ann_update_dev(d_lv.ptr, d_roots.ptr, K, s["c"], s["n_c"], s["dim"], s["grow"], d_new.ptr,
                                                                           api._p(idx), len(idx), d_adv.ptr, None, d_pub.ptr))
                g_adv, _ = _windowed(api, lib, check, want, NO_LOOKUP, window, run)
                _check_window(want, NO_LOOKUP, g_adv, NO_LOOKUP, window, (cut, window))
                assert np.array_equal(d_pub.download(pub.shape), pub), (cut, window)
                assert np.array_equal(d_lv.download(s["grown"].shape), s["after"]), (cut, window)
                halves.append(g_adv)
            assert np.array_equal(np.concatenate([halves[0][:cut], halves[1][cut:]]), want), cut
    finally:
        for b in up:
            b.free()


AUDIT_SEED = 60           # test_ann_audit_cpu.case's assertions hold for it at K = 70: the K distances of every member pairwise distinct


def test_frame_under_the_audit_layout_at_70_clusters(api, O):
    from test_ann_audit_cpu import L, case
    metric, K, n_c, c = "euclidean", 70, 3, 69
    f = WS.frame_facts(K, c, 2)
    assert f["indicator_blocks"] == 2 and f["c_block"] == 1 and f["sponge_perms"] == 36
    m, cent, mem, roots, index_root = case(O, metric, K, n_c, c, seed=AUDIT_SEED)
    got = api.wit_ann_audit(metric, cent, mem, roots, c, P, L, selectors=True)
    assert got["n_in"] == m["n_in"] == K + 2
    _same_stream(got["stream"], m["advice"], f"blocks {m['regions']}, per member {m['per_member']}: ")
    assert np.array_equal(got["lookup"], m["lookup"]) and np.array_equal(got["selectors"], m["selectors"])
    gen = m["generator"]
    assert np.array_equal(got["flags"][~gen], m["flags"][~gen])
    assert np.array_equal(got["routed"], m["routed"]) and got["routed"].all()
    assert np.array_equal(got["public"], m["public"]) and np.array_equal(got["public"][0], index_root)


def test_frame_under_the_mean_layout_at_70_clusters(api, O):
    from test_ann_mean_cpu import L, case
    K, n_c, dim, c = 70, 3, 2, 0
    f = WS.frame_facts(K, c, 2)
    assert f["indicator_blocks"] == 2 and f["c_block"] == 0 and f["sponge_perms"] == 36
    m, cent, mem, roots, index_root = case(O, K, n_c, dim, c)
    got = api.wit_ann_mean(cent, mem, roots, c, P, L, selectors=True)
    assert got["n_in"] == m["n_in"] == K + 2
    _same_stream(got["stream"], m["advice"], f"blocks {m['regions']}: ")
    assert np.array_equal(got["lookup"], m["lookup"]) and np.array_equal(got["selectors"], m["selectors"])
    gen = m["generator"]
    assert np.array_equal(got["flags"][~gen], m["flags"][~gen])
    assert np.array_equal(got["mean_ok"], m["mean_ok"]) and got["mean_ok"].all()
    assert np.array_equal(got["public"], m["public"]) and np.array_equal(got["public"][0], index_root)


# ---------------------------------------------------------------------------------------------------------------- D: chain_fold_wave
@pytest.mark.parametrize("name", sorted(KMEANS))
def test_kmeans_chains_past_one_chunk_are_the_oracles(api, O, name):
    kmeans_reaches(name)
    n, dim, K, I = KMEANS[name]
    qv, c, cent, ind = kmeans_case(O, name)
    got = api.wit_kmeans("manhattan", qv, K, I, P=P, L=KM_L, selectors=True)
    assert np.array_equal(got["centroids"], cent) and np.array_equal(got["indicators"], ind)
    assert_streams(got, c)


def test_kmeans_size_chain_under_rank_windows(api, O):
    """N577 cut one cell into the cluster-size chain, at a lane's eighth step (the edge of its first chunk) and inside lane 31's steps:
    every lane's test of its own cells against the window decides differently on the two sides of a cut"""
    from halo2_vectordb_amd._lib import check
    lib = api.init()
    n, dim, K, I = KMEANS["N577"]
    f = kmeans_reaches("N577")
    qv, c, cent, ind = kmeans_case(O, "N577")
    adv, lk = c.advice(), c.lookup()
    cells = adv.shape[0]
    at = WS.sizes_chain(adv, c.selectors(), n, K, P)
    step = lambda v: at + (v - 1) * 4 * K                          # the cells of step v of cluster 0's chain
    lo5, lo31 = f["lanes"][5][0], f["lanes"][31][0]
    assert (lo5, lo31) == (50, 310) and f["chunks"][5] == [8, 2] and f["lanes"][31][1] == 320
    cuts = (at + 1, step(lo5 + WS.KM_PF), step(lo31 + 4) + 2)
    assert all(at < cut < at + 4 * (n - 1) * K for cut in cuts)
    up = []
    try:
        d_vec, d_cent, d_ind = _dev(api, up, qv), api.DeviceBuffer(cent.nbytes), api.DeviceBuffer(ind.nbytes)
        up += [d_cent, d_ind]
        run = lambda d_adv, d_lk: check(lib.vdb_wit_kmeans_dev(api.METRICS["manhattan"], P, KM_L, d_vec.ptr, n, dim, K, I, 0, d_adv.ptr, d_lk.ptr, None,
                                                               d_cent.ptr, d_ind.ptr))
        for cut in cuts:
            halves = []
            for window in ((0, cut, 0, len(lk)), (cut, cells, 0, len(lk))):
                g_adv, g_lk = _windowed(api, lib, check, adv, lk, window, run)
                _check_window(adv, lk, g_adv, g_lk, window, (cut, window))
                assert np.array_equal(d_cent.download(cent.shape), cent) and np.array_equal(d_ind.download(ind.shape), ind), (cut, window)   # every rank computes every value
                halves.append(g_adv)
            assert np.array_equal(np.concatenate([halves[0][:cut], halves[1][cut:]]), adv), cut
    finally:
        for b in up:
            b.free()
