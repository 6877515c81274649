"""VDB_NTT_SHOUP_ALL: the specialised 256- / 512-point NTT instantiations with every product by a constant a Shoup product (stage
twiddles, omega_4, the inter-pass twiddles, the coset factors) against the same instantiations with Montgomery products (=0), on inputs
that stress the limb and value bounds — all r - 1, all zero, r - 1 alternating with zero, random — and against the oracle.  The knob is
read once per process: each arm runs in a child process of its own.  Bytes must be identical."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = 0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001

# every SA instantiation: 2^16 (8 + 8: lagrange_to_coeff, forward), 2^17 (9 + 8), 2^18 (9 + 9: forward, the zero-padded coset
# extension from 2^16, extended_to_coeff)
SCRIPT = r"""
import sys
import numpy as np
from halo2_vectordb_amd import api
from oracle import oracle as O
api.init(0)
R = 0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001
def pattern(name, n, seed):
    top = np.array([(R - 1) >> (64 * i) & (2**64 - 1) for i in range(4)], dtype=np.uint64)
    a = np.zeros((n, 4), dtype=np.uint64)
    if name == "max":
        a[:] = top
    elif name == "alt":
        a[::2] = top
    elif name == "rand":
        a = O.random_fr(np.random.default_rng(seed), n).reshape(n, 4)
    return a
out = {}
for name in ("max", "zero", "alt", "rand"):
    for k in (16, 17, 18):
        cols = np.stack([pattern(name, 1 << k, k), pattern("rand", 1 << k, 100 + k)])
        out[f"fwd_{name}_{k}"] = api.ntt_batch(cols, O.root_of_unity(k))
        out[f"l2c_{name}_{k}"] = api.lagrange_to_coeff(cols)
    cols = np.stack([pattern(name, 1 << 16, 7), pattern("rand", 1 << 16, 8)])
    out[f"ext_{name}"] = api.coeff_to_extended(cols, 2)
    out[f"e2c_{name}"] = api.extended_to_coeff(np.stack([pattern(name, 1 << 18, 9)]), 16, 2)
    out[f"lde_{name}"] = api.coeff_to_extended(out[f"l2c_{name}_16"], 2)
    out[f"rt_{name}"] = api.extended_to_coeff(out[f"lde_{name}"], 16, 2)
np.savez(sys.argv[1], **out)
print("ok")
"""


def _arm(tmp_path, on):
    path = str(tmp_path / f"arm{on}.npz")
    env = dict(os.environ, VDB_NTT_SHOUP_ALL=str(on), PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-c", SCRIPT, path], env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout + r.stderr
    return dict(np.load(path))


def test_shoup_all_on_off_identical_and_equal_to_oracle(tmp_path):
    from oracle import oracle as O
    off, on = _arm(tmp_path, 0), _arm(tmp_path, 1)
    assert sorted(off) == sorted(on)
    for key in off:
        assert off[key].tobytes() == on[key].tobytes(), key
    # the oracle on the same inputs (the child's patterns rebuilt here)
    top = np.array([(R - 1) >> (64 * i) & (2**64 - 1) for i in range(4)], dtype=np.uint64)

    def pattern(name, n, seed):
        a = np.zeros((n, 4), dtype=np.uint64)
        if name == "max":
            a[:] = top
        elif name == "alt":
            a[::2] = top
        elif name == "rand":
            a = O.random_fr(np.random.default_rng(seed), n).reshape(n, 4)
        return a

    for name in ("max", "zero", "alt", "rand"):
        for k in (16, 18):
            cols = np.stack([pattern(name, 1 << k, k), pattern("rand", 1 << k, 100 + k)])
            assert np.array_equal(on[f"fwd_{name}_{k}"], O.ntt_batch(cols, O.root_of_unity(k), threads=4)), (name, k)
        cols = np.stack([pattern(name, 1 << 16, 16), pattern("rand", 1 << 16, 116)])
        want_c, want_e = O.lde_batch(cols, ext=2, threads=4)
        assert np.array_equal(on[f"l2c_{name}_16"], want_c), name
        assert np.array_equal(on[f"lde_{name}"], want_e), name
        # extended_to_coeff of the extension: the coefficients again, zero above 2^16
        assert np.array_equal(on[f"rt_{name}"][:, : 1 << 16], want_c) and not on[f"rt_{name}"][:, 1 << 16:].any(), name
