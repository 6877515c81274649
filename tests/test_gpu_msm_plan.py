"""The MSM driver against its plan, at the smallest shapes where each of its paths exists: the points are the oracle's, and the launches
of k_msm_sort, k_msm_scatter2 and k_msm_combine are what tests/msm_plan_model.py plans for the job — the model that
tests/test_msm_plan_cpu.py holds to the planner's header.

  k = 6, c = 8, 3 columns of 64                            one batch, direct scatter
  k = 9, c = 13, 3 columns of 2^9 - 37, a cap of one byte  three batches of one column, two-phase scatter
  k = 3, c = 7, one column of 1 and of 3 scalars           the entries end off a 16-byte boundary, `raw` starts on the next one: the
                                                           result alone"""
import numpy as np
import pytest

import msm_plan_model as M
from test_gpu_msm import witness_like

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def api():
    from halo2_vectordb_amd import api as a
    a.init(0)
    return a


def setup(api, O, k, c, seed):
    g, gl = O.srs_from_tau(k, 0xC0117A7 + k)
    srs = api.Srs(k, g, gl, window_bits=c)
    rc, _, shape = M.window(k, c)
    assert rc == M.OK and srs.info() == (k, shape.c, shape.W)
    return srs, gl, shape, np.random.default_rng(seed)


def columns(O, rng, n_cols, n):
    """dense, witness-like and alternating columns"""
    cols = np.stack([O.random_fr(rng, n), witness_like(O, rng, n), O.random_fr(rng, n)][:n_cols])
    if n_cols > 2:
        cols[2, ::2] = witness_like(O, rng, n)[::2]
    return cols


def run(api, srs, cols, P=None):
    """the MSM of `cols`; with a plan, its launches held to it"""
    n_cols, n = cols.shape[:2]
    buf = api.DeviceBuffer(cols.nbytes)
    try:
        buf.upload(cols)
        api.profile_begin(deferred=True)
        try:
            got = api.msm_batch_dev(srs, buf.ptr, n_cols, n)
        finally:
            prof = api.profile_end()
    finally:
        buf.free()
    if P is None:
        return got
    launches = {name: prof.get(name, {"launches": 0})["launches"] for name in ("k_msm_sort", "k_msm_scatter2", "k_msm_combine")}
    assert launches == {"k_msm_sort": P.n_batches, "k_msm_scatter2": P.n_batches if P.fine_bits else 0,
                        "k_msm_combine": P.combine_passes * P.n_batches}, (launches, P.n_batches, P.fine_bits, P.combine_passes)
    return got


def test_one_batch_direct_scatter(api, O):
    srs, gl, shape, rng = setup(api, O, 6, 8, 1)
    try:
        cols = columns(O, rng, 3, 64)
        P = M.plan(shape, 3, 64)
        assert (P.n_batches, P.nb, P.fine_bits, P.lcap, P.combine_passes) == (1, 3, 0, 32, 7)
        assert np.array_equal(run(api, srs, cols, P), O.msm_batch(cols, gl, threads=4))
    finally:
        srs.free()


def test_three_batches_two_phase_scatter(api, O):
    from halo2_vectordb_amd._lib import check
    lib, n = api.init(), (1 << 9) - 37
    srs, gl, shape, rng = setup(api, O, 9, 13, 2)
    try:
        cols = columns(O, rng, 3, n)
        P = M.plan(shape, 3, n, M.Mem(16 * M.GIB, 0, 1))        # the work space released and capped at one byte: one column a batch
        assert (P.n_batches, P.nb, P.fine_bits) == (3, 1, 4) and P.combine_passes == 9
        check(lib.vdb_scratch_release())
        check(lib.vdb_msm_set_scratch_cap(1))
        try:
            got = run(api, srs, cols, P)
        finally:
            check(lib.vdb_msm_set_scratch_cap(0))
            check(lib.vdb_scratch_release())
        assert np.array_equal(got, O.msm_batch(cols, gl[:n], threads=4))
    finally:
        srs.free()


def test_entries_that_end_off_a_16_byte_boundary(api, O):
    srs, gl, shape, rng = setup(api, O, 3, 7, 3)
    try:
        for n in (1, 3):
            cols = columns(O, rng, 1, n)
            P = M.plan(shape, 1, n)
            assert P.region_bytes("entries") % 16 and P.off["raw"] % 16 == 0
            assert np.array_equal(run(api, srs, cols), O.msm_batch(cols, gl[:n], threads=1))
    finally:
        srs.free()
