"""The NTT driver against its plan, at the smallest sizes where each of its paths exists, two columns each: the output is the oracle's,
and the number of k_ntt_pass launches is L x chunks of tests/ntt_plan_model.py for the job the entry point asks for — the model that
tests/test_ntt_plan_cpu.py holds to the planner's header.  (The SA instantiations need 2^16 .. 2^18: tests/test_gpu_ntt_shoup_all.py.)

  2^4 forward                                   a single pass
  2^11 forward, lagrange_to_coeff               passes of 6 + 5 stages; 1 / n on the inter-pass twiddles
  2^13 forward                                  passes of 7 + 6
  coeff_to_extended 2^11 -> 2^13                zero padding: pass 0 starts at stage 2
  extended_to_coeff, k = 11, ext 2              the factors zeta^-(e mod 3) at the write-out
  coeff_to_cosets, k = 11, 3 slots, with and without a scalar      virtual columns
  lagrange_to_coeff_src, k = 11                 columns read through their descriptors"""
import ctypes

import numpy as np
import pytest

import ntt_plan_model as M

pytestmark = pytest.mark.gpu

N_COLS = 2
REV2 = (0, 2, 1, 3)          # slot t of the extended domain taken coset by coset = points 4 r + REV2[t] of the natural order


@pytest.fixture(scope="module")
def api():
    from halo2_vectordb_amd import api as a
    a.init(0)
    return a


@pytest.fixture(scope="module")
def ref(O):
    """inputs and the oracle's outputs, computed once and shared; nothing changes them"""
    rng = np.random.default_rng(20261020)
    r = {"s": O.random_fr(rng, 1)[0]}
    for k in (4, 11, 13):
        r["cols", k] = O.random_fr(rng, N_COLS << k).reshape(N_COLS, 1 << k, 4)
        r["fwd", k] = O.ntt_batch(r["cols", k], O.root_of_unity(k), threads=2)
    r["coeff"], r["ext"] = O.lde_batch(r["cols", 11], ext=2, threads=2)
    scaled = O.fr_mul(r["coeff"].reshape(-1, 4), np.tile(r["s"], (N_COLS << 11, 1))).reshape(N_COLS, 1 << 11, 4)
    r["ext_scaled"] = O.lde_batch(O.ntt_batch(scaled, O.root_of_unity(11), threads=2), ext=2, threads=2)[1]
    return r


def launches(api, job, run):
    """runs `run` and holds its k_ntt_pass launches to the model's plan of `job`"""
    P = M.plan(job)
    assert P.rc == M.OK
    api.profile_begin(deferred=True)
    try:
        out = run()
    finally:
        prof = api.profile_end()
    assert prof["k_ntt_pass"]["launches"] == P.L * P.chunks(job.n_cols), (job, prof)
    return out, P


@pytest.mark.parametrize("k,sizes", [(4, [4]), (11, [6, 5]), (13, [7, 6])])
def test_forward(api, O, ref, k, sizes):
    got, P = launches(api, M.Job(k, n_cols=N_COLS, in_place=True), lambda: api.ntt_batch(ref["cols", k], O.root_of_unity(k)))
    assert [p["S"] for p in P.passes] == sizes and not P.needs_scaled_twiddles
    assert np.array_equal(got, ref["fwd", k])


def test_lagrange_to_coeff(api, ref):
    got, P = launches(api, M.Job(11, n_cols=N_COLS, in_place=True, scale_ninv=True), lambda: api.lagrange_to_coeff(ref["cols", 11]))
    assert P.L == 2 and P.needs_scaled_twiddles and not P.passes[1]["scale"]
    assert np.array_equal(got, ref["coeff"])


def test_coeff_to_extended_and_back(api, ref):
    job = M.Job(13, in_len=1 << 11, n_cols=N_COLS, coset_in=True)
    got, P = launches(api, job, lambda: api.coeff_to_extended(ref["coeff"], 2))
    assert [(p["S"], p["s0"]) for p in P.passes] == [(7, 2), (6, 0)] and P.passes[0]["coset"] == 1
    assert np.array_equal(got, ref["ext"])
    job = M.Job(13, n_cols=N_COLS, in_place=True, scale_ninv=True, coset_out=True)
    got, P = launches(api, job, lambda: api.extended_to_coeff(ref["ext"], 11, 2))
    assert P.passes[1]["coset_out"] and not P.passes[0]["coset_out"]
    assert np.array_equal(got[:, : 1 << 11], ref["coeff"]) and not got[:, 1 << 11:].any()


@pytest.mark.parametrize("scaled", [False, True])
def test_coeff_to_cosets(api, ref, scaled):
    from halo2_vectordb_amd._lib import check
    lib, k, n_slots = api.init(), 11, 3
    d_c, d_s = api.DeviceBuffer(ref["coeff"].nbytes), api.DeviceBuffer(N_COLS * n_slots * 32 << k)
    try:
        d_c.upload(ref["coeff"])
        job = M.Job(k, n_cols=N_COLS * n_slots, vslots=n_slots, has_in_tabs=True)
        run = lambda: check(lib.vdb_coeff_to_cosets_dev(d_c.ptr, d_s.ptr, ctypes.c_size_t(N_COLS), k, n_slots, api._p(ref["s"]) if scaled else None))
        _, P = launches(api, job, run)
        assert P.passes[0]["coset"] == 3 and P.passes[0]["kernel"] == "VS" and P.chunk_cols(job.n_cols) == N_COLS * n_slots
        got = d_s.download((N_COLS, n_slots, 1 << k, 4))
    finally:
        d_c.free()
        d_s.free()
    ext = ref["ext_scaled"] if scaled else ref["ext"]
    assert np.array_equal(got, np.stack([ext[:, REV2[t]::4] for t in range(n_slots)], axis=1))


def test_lagrange_to_coeff_src(api, O, ref):
    from halo2_vectordb_amd._lib import check
    lib, k, n_blind = api.init(), 11, 6
    n = 1 << k
    cols = ref["cols", 11]
    # column 0: n - n_blind cells of the stream and its blinding rows; column 1: 65 cells, no blinds, zero elsewhere
    lens = (n - n_blind, 65)
    want_in = np.zeros_like(cols)
    want_in[0, : lens[0]], want_in[0, n - n_blind:] = cols[0, : lens[0]], cols[1, :n_blind]
    want_in[1, : lens[1]] = cols[1, 7: 7 + lens[1]]
    d_stream, d_blind, d_src, d_out = (api.DeviceBuffer(cols.nbytes), api.DeviceBuffer(n_blind * 32), api.DeviceBuffer(64),
                                       api.DeviceBuffer(cols.nbytes))
    try:
        d_stream.upload(cols)
        d_blind.upload(cols[1, :n_blind])
        d_src.upload(np.array([d_stream.ptr.value, lens[0], d_blind.ptr.value, d_stream.ptr.value + (n + 7) * 32, lens[1], 0], dtype=np.uint64))
        job = M.Job(k, n_cols=N_COLS, scale_ninv=True, has_srcs=True)
        _, P = launches(api, job, lambda: check(lib.vdb_lagrange_to_coeff_src_dev(d_src.ptr, d_out.ptr, ctypes.c_size_t(N_COLS), k, n_blind)))
        assert P.L == 2
        got = d_out.download(cols.shape)
    finally:
        for b in (d_stream, d_blind, d_src, d_out):
            b.free()
    assert np.array_equal(got, O.lde_batch(want_in, ext=0, threads=2)[0])
