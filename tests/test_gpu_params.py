"""SRS from a halo2 params file on the device (halo2_vectordb_amd/srs.py, csrc/srs.hip): g_to_lagrange against k_srs_setup's direct
L_i(tau) G and the oracle, its exceptional inputs against a Python-integer DFT over G1, the point checks of the RawBytes reader, the
downsize of a larger file, ParamsKZG.check, and proofs made from a params file — bit-equal to the tau path's and verified with the
params file's G2 points through the library, the key files and the command line."""
import io
import json
import random
from contextlib import redirect_stdout

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

R = 0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001
Q = 0x30644E72E131A029B85045B68181585D97816A916871CA8D3C208C16D87CFD47
TAU = 0x1D4C2B3A59687F0E1D2C3B4A5968778695A4B3C2D1E0F
FIXED = ("sel", "sigma", "cst", "table")


@pytest.fixture(scope="module")
def api():
    from halo2_vectordb_amd import api as a
    a.init(0)
    return a


def _mont(tau):
    from halo2_vectordb_amd.srs import tau_mont_limbs
    return tau_mont_limbs(tau)


@pytest.mark.parametrize("k", list(range(1, 19)))
def test_lagrange_from_monomial_equals_the_direct_setup(api, O, k):
    from halo2_vectordb_amd.srs import lagrange_from_monomial
    tau = random.Random(1000 + k).randrange(2, R)
    g, gl = api.srs_setup_unsafe(k, _mont(tau))
    got = lagrange_from_monomial(g)
    assert got.tobytes() == gl.tobytes()
    if k <= 10:
        og, ogl = O.srs_from_tau(k, tau)
        assert np.array_equal(og, g) and np.array_equal(ogl, got)


# ---------------------------------------------------------------- exceptional inputs against a Python DFT over G1
def _omega(api, k):
    w = api.root_of_unity(k)
    return sum(int(w[i]) << (64 * i) for i in range(4)) * pow(1 << 256, -1, R) % R


def _dft_g1(pts, omega):
    """n^-1 sum_j omega^-ij P_j with oracle/pairing.py's affine group law (None = the identity)"""
    from oracle import pairing as PR
    n = len(pts)
    wi, n_inv = pow(omega, -1, R), pow(n, -1, R)
    out = []
    for i in range(n):
        acc = None
        for j, p in enumerate(pts):
            if p is not None:
                acc = PR.pt_add(acc, PR.pt_mul(p, pow(wi, i * j, R)))
        out.append(None if acc is None else PR.pt_mul(acc, n_inv))
    return out


def _to_words(O, pts):
    return np.stack([np.zeros(8, dtype=np.uint64) if p is None else O.fq_from_ints([p[0], p[1]]).reshape(8) for p in pts])


def _exceptional_cases(k):
    from oracle import pairing as PR
    rnd = random.Random(k)
    n = 1 << k
    rand = lambda: PR.pt_mul(PR.G1, rnd.randrange(1, R))
    P = rand()
    base = [rand() for _ in range(n)]
    yield "identity entries", [None if j % 3 == 0 else base[j] for j in range(n)]
    yield "all identity", [None] * n
    yield "all equal", [P] * n
    yield "P / -P across halves", [base[j] if j < n // 2 else PR.pt_neg(base[j - n // 2]) for j in range(n)]
    yield "P / -P neighbours", [base[j] if j % 2 == 0 else PR.pt_neg(base[j - 1]) for j in range(n)]
    yield "P / P across halves", [base[j % (n // 2)] for j in range(n)]
    yield "one point", [P if j == n - 1 else None for j in range(n)]


@pytest.mark.parametrize("k", [1, 2, 3, 4])
def test_lagrange_from_monomial_exceptional_inputs(api, O, k):
    from halo2_vectordb_amd.srs import lagrange_from_monomial
    omega = _omega(api, k)
    for name, pts in _exceptional_cases(k):
        got = lagrange_from_monomial(_to_words(O, pts))
        assert np.array_equal(got, _to_words(O, _dft_g1(pts, omega))), name


def test_downsize_abi_on_a_longer_g(api, O):
    """vdb_srs_downsize takes the first 2^k points of a longer host array"""
    import ctypes
    from halo2_vectordb_amd import _lib
    g, _ = api.srs_setup_unsafe(9, _mont(TAU))
    _, gl7 = api.srs_setup_unsafe(7, _mont(TAU))
    out = np.zeros((128, 8), dtype=np.uint64)
    assert _lib.load().vdb_srs_downsize(ctypes.c_uint32(7), g.ctypes.data, out.ctypes.data) == 0
    assert np.array_equal(out, gl7)


# ---------------------------------------------------------------- point validation
def test_point_validation(api):
    from halo2_vectordb_amd.srs import g1_check
    g, _ = api.srs_setup_unsafe(17, _mont(TAU))
    n = len(g)
    assert g1_check(g) == (0, n)
    q_words = np.array([(Q >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)], dtype=np.uint64)
    x_big, y_big, off, ident = g.copy(), g.copy(), g.copy(), g.copy()
    x_big[5, :4] = q_words                                # x = q: not below q
    y_big[70_001, 4:] = np.uint64(0xFFFFFFFFFFFFFFFF)     # y far above q
    y_big[n - 1, 4:] = q_words
    off[3, 0] ^= np.uint64(1)                             # still below q, off the curve
    off[99_999, 4] ^= np.uint64(2)
    ident[0] = 0
    ident[n - 1] = 0
    assert g1_check(x_big) == (1, 5)
    assert g1_check(y_big) == (2, 70_001)
    assert g1_check(off) == (2, 3)
    assert g1_check(ident) == (0, n)
    assert g1_check(np.zeros((0, 8), dtype=np.uint64)) == (0, 0)


def test_read_names_a_bad_point(api, tmp_path):
    from halo2_vectordb_amd.srs import ParamsKZG
    p = ParamsKZG.setup_unsafe(6, TAU)
    p.g[9, 0] ^= np.uint64(1)
    p.write(tmp_path / "bad_g.srs")
    with pytest.raises(ValueError, match=r"g\[9\]"):
        ParamsKZG.read(tmp_path / "bad_g.srs")
    with pytest.raises(ValueError, match=r"g\[9\]"):
        ParamsKZG.read(tmp_path / "bad_g.srs", k=5)
    assert ParamsKZG.read(tmp_path / "bad_g.srs", k=3).k == 3         # the bad point lies beyond what is read
    p = ParamsKZG.setup_unsafe(6, TAU)
    p.g_lagrange[40, 6] ^= np.uint64(4)
    p.write(tmp_path / "bad_gl.srs")
    with pytest.raises(ValueError, match=r"g_lagrange\[40\]"):
        ParamsKZG.read(tmp_path / "bad_gl.srs")
    assert np.array_equal(ParamsKZG.read(tmp_path / "bad_gl.srs", k=5).g_lagrange, ParamsKZG.setup_unsafe(5, TAU).g_lagrange)


# ---------------------------------------------------------------- downsize
def test_downsize_of_a_larger_file(api, tmp_path):
    from halo2_vectordb_amd.srs import ParamsKZG
    path = tmp_path / "kzg_bn254_15.srs"
    ParamsKZG.setup_unsafe(15, TAU).write(path)
    got, want = ParamsKZG.read(path, k=12), ParamsKZG.setup_unsafe(12, TAU)
    assert got.k == 12
    for name in ("g", "g_lagrange", "g2", "s_g2"):
        assert getattr(got, name).tobytes() == getattr(want, name).tobytes(), name
    full = ParamsKZG.read(path)
    assert full.k == 15 and np.array_equal(full.g[: 1 << 12], want.g)


# ---------------------------------------------------------------- check()
def test_check(api, O):
    from halo2_vectordb_amd.srs import ParamsKZG
    p = ParamsKZG.setup_unsafe(10, TAU)
    assert p.check(seed=3)
    bumped = ParamsKZG(p.k, p.g.copy(), p.g_lagrange, p.g2, p.s_g2)
    x, y = O.fq_to_ints(p.g[5].reshape(2, 4))
    from oracle import pairing as PR
    s = PR.pt_add((x, y), PR.G1)
    bumped.g[5] = O.fq_from_ints([s[0], s[1]]).reshape(8)              # g[5] + G: still on the curve
    assert not bumped.check(seed=3)
    swapped = ParamsKZG(p.k, p.g, p.g_lagrange.copy(), p.g2, p.s_g2)
    swapped.g_lagrange[[17, 300]] = swapped.g_lagrange[[300, 17]]
    assert not swapped.check(seed=3)
    other = ParamsKZG.setup_unsafe(10, TAU + 1)
    assert not ParamsKZG(p.k, p.g, p.g_lagrange, p.g2, other.s_g2).check(seed=3)
    assert not ParamsKZG(p.k, p.g, p.g_lagrange, other.s_g2, p.s_g2).check(seed=3)


# ---------------------------------------------------------------- proofs from a params file
def _cli(*args):
    from halo2_vectordb_amd import verify as cli
    buf = io.StringIO()
    with redirect_stdout(buf):
        rc = cli.main([str(a) for a in args])
    return rc, json.loads(buf.getvalue())


def _meta(path):
    with np.load(path) as doc:
        return json.loads(bytes(doc["meta"]).decode()), sorted(doc.files)


def _prove(hp, seed, tmp_path, tag):
    from halo2_vectordb_amd.io import write_snark
    from halo2_vectordb_amd.rounds import ProverRounds
    hp.setup()
    pr = ProverRounds(hp).keygen()
    try:
        assert pr.keygen_report.violations() == 0
        out = pr.prove(None, seed=seed)
        snark = str(tmp_path / (tag + ".snark"))
        write_snark(snark, out["proof"], out["instances"])
        pr.save_verifying_key(snark + ".vk.npz", opened=out["opened"])
        pr.save_verifying_key_raw(snark + ".vk")
        return dict(proof=out["proof"], fixed={name: pr.fixed[name].commits.copy() for name in FIXED}, snark=snark)
    finally:
        pr.free()
        hp.free()


@pytest.mark.parametrize("circuit", ["kmeans", "query"])
def test_proof_from_a_params_file(api, tmp_path, circuit):
    from halo2_vectordb_amd.pipeline import KmeansHotPath, QueryHotPath
    from halo2_vectordb_amd.srs import ParamsKZG
    from halo2_vectordb_amd.verifier import Verifier
    make = {"kmeans": lambda **kw: KmeansHotPath(n=8, dim=4, K=2, I=1, k=12, L=11, metric="cosine", **kw),
            "query": lambda **kw: QueryHotPath(n=6, dim=4, k=12, L=11, metric="cosine", **kw)}[circuit]
    seed = 31 if circuit == "kmeans" else 17
    srs_path, other_path = tmp_path / "kzg_bn254_13.srs", tmp_path / "other_13.srs"
    ParamsKZG.setup_unsafe(13, TAU).write(srs_path)
    ParamsKZG.setup_unsafe(13, TAU + 5).write(other_path)
    with pytest.raises(ValueError):
        make(tau=TAU, params=srs_path)
    hp = make(params=ParamsKZG.read(srs_path))
    a = _prove(hp, seed, tmp_path, "params")
    assert hp.tau is None and hp.tau_g2 is not None
    b = _prove(make(tau=TAU), seed, tmp_path, "tau")
    assert a["proof"] == b["proof"]
    for name in FIXED:
        assert np.array_equal(a["fixed"][name], b["fixed"][name]), name
    sa, sb = a["snark"], b["snark"]
    with open(sa + ".vk", "rb") as fa, open(sb + ".vk", "rb") as fb:
        assert fa.read() == fb.read()
    (ma, files_a), (mb, files_b) = _meta(sa + ".vk.npz"), _meta(sb + ".vk.npz")
    assert files_a == files_b
    assert set(ma) - set(mb) == {"tau_g2", "g2"} and set(mb) - set(ma) == {"tau"}
    assert {key: v for key, v in ma.items() if key not in ("tau_g2", "g2")} == {key: v for key, v in mb.items() if key != "tau"}
    # verified with the params file's G2 side, from either key file
    assert Verifier.from_files(sa, sa + ".vk.npz").verify()
    assert Verifier.from_files(sa, sa + ".vk.npz", params=srs_path).verify()
    assert Verifier.from_files(sa, sa + ".vk", params=srs_path).verify()
    assert Verifier.from_files(sa, sa + ".vk", params=ParamsKZG.read(srs_path, k=1)).verify()
    assert Verifier.from_files(sb, sb + ".vk", params=srs_path).verify()
    assert _cli(sa, sa + ".vk", "--params", srs_path)[0] == 0
    assert _cli(sa, sa + ".vk.npz", "--params", srs_path)[0] == 0
    # another SRS's G2 side rejects it
    assert not Verifier.from_files(sa, sa + ".vk", params=other_path).verify()
    assert _cli(sa, sa + ".vk", "--params", other_path)[0] == 1
    assert _cli(sa, sa + ".vk.npz", "--params", other_path)[0] == 1
    from halo2_vectordb_amd import verify as cli
    assert cli.main([sa, sa + ".vk", "--params"]) == 2 and cli.main([sa, sa + ".vk", hex(TAU), "--params", str(srs_path)]) == 2
