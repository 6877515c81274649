"""vdb_fr_from_wide_dev (k_from_wide, core.hip), the source of every blinding scalar: 64-byte little-endian records reduced mod r on the
device against `int.from_bytes(rec, "little") % r` — in Montgomery form, and in canonical form through vdb_fr_to_canonical.  The kernel
calls to_mont on raw 256-bit halves, so mont_mul's first operand ranges up to 2^256 - 1; the records are the from_wide cases of
tests/ec_model.py (the halves at 0, 1, r - 1, r, r + 1, 2 r, 2^255, 2^256 - 1 in all pairs, the 512-bit multiples of r and their
neighbours, random ones), which tests/test_gpu_ec.py also runs through the probe."""
import ctypes
import random

import numpy as np
import pytest

import ec_model as E

pytestmark = pytest.mark.gpu

R = E.R
SENTINEL = 0xA5A5A5A5A5A5A5A5


@pytest.fixture(scope="module")
def api():
    from halo2_vectordb_amd import api as a
    a.init(0)
    return a


def limbs4(vals):
    return np.array([[(v >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)] for v in vals], dtype=np.uint64).reshape(-1, 4)


def from_wide(api, raw, n):
    """the n scalars the device makes of the 64 n bytes `raw`, and the record behind them, which no lane may touch"""
    assert len(raw) == 64 * n
    lib = api.init()
    wide, out = api.DeviceBuffer(max(64 * n, 64)), api.DeviceBuffer(32 * (n + 1))
    try:
        if n:
            wide.upload(np.frombuffer(raw, dtype=np.uint8))
        out.upload(np.full((n + 1, 4), SENTINEL, dtype=np.uint64))
        api.check(lib.vdb_fr_from_wide_dev(wide.ptr, ctypes.c_size_t(n), out.ptr))
        api.sync()
        got = out.download((n + 1, 4))
    finally:
        wide.free()
        out.free()
    assert (got[n] == SENTINEL).all()
    return got[:n]


def check_records(api, raw, n):
    got = from_wide(api, raw, n)
    vals = [int.from_bytes(raw[64 * i: 64 * i + 64], "little") % R for i in range(n)]
    assert np.array_equal(got, limbs4([v * E.U256 % R for v in vals]))
    if n:
        assert np.array_equal(api.fr_to_canonical(got), limbs4(vals))
    return vals


def test_from_wide_at_the_edges_of_both_halves(api):
    cases = E.from_wide_values(random.Random(20261018))
    tags = {t.split("/")[0] for t, _, _ in cases}
    assert tags == {"edge", "multiple", "random"} and sum(t == "edge" for t, _, _ in cases) == 64
    raw = b"".join((lo | hi << 256).to_bytes(64, "little") for _, lo, hi in cases)
    vals = check_records(api, raw, len(cases))
    # the multiples of r do reduce to -1, 0, 1
    assert {v for (t, _, _), v in zip(cases, vals) if t.startswith("multiple")} == {R - 1, 0, 1}
    print("cases:", len(cases))


@pytest.mark.parametrize("n", [0, 1, 257])
def test_from_wide_lane_counts(api, n):
    """no record, one, and 257: one lane in a second block; the record behind the last one stays untouched"""
    check_records(api, np.random.default_rng(n).bytes(64 * n), n)
    print("cases:", n)


def test_chacha20_stream_reduces_to_fr_random(api):
    """the ChaCha20 keystream of srs.py through the device: scalar i is halo2curves' Fr::random of draw i (srs.fr_random in Python
    integers); the first is the scalar of the deterministic SRS"""
    from halo2_vectordb_amd import srs
    n = 300
    raw = srs.ChaCha20Rng().fill_bytes(64 * n)
    vals = check_records(api, raw, n)
    rng = srs.ChaCha20Rng()
    assert vals == [srs.fr_random(rng) for _ in range(n)] and vals[0] == srs.gen_srs_tau()
    print("cases:", n)


@pytest.mark.parametrize("seed", [0, 5, 20261018])
def test_random_scalars_dev_is_its_seeded_stream_reduced(api, seed):
    """api.random_scalars_dev(seed=S): the 64 n bytes its docstring names (numpy's default_rng(S).bytes), reduced in Python integers"""
    n = 257
    out = api.DeviceBuffer(32 * n)
    try:
        api.random_scalars_dev(out.ptr, n, seed=seed)
        got = out.download((n, 4))
    finally:
        out.free()
    raw = np.random.default_rng(seed).bytes(64 * n)
    want = [int.from_bytes(raw[64 * i: 64 * i + 64], "little") % R for i in range(n)]
    assert np.array_equal(got, limbs4([v * E.U256 % R for v in want]))
    print("cases:", n)
