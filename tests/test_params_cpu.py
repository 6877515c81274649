"""halo2 params files without a GPU (halo2_vectordb_amd/srs.py): the RawBytes layout pinned by a file assembled here with struct.pack from
the oracle's SRS and G2 points, the file size, the reader's refusals, and the host check of G2 points (vdb_g2_check) against points
built with oracle/pairing.py."""
import struct

import numpy as np
import pytest

TAU = 0x2A5F0C91D3E7B4461F08
K = 2


def _fq_limbs(v):
    from oracle import pairing as PR
    m = (v << 256) % PR.Q
    return [(m >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)]


def _g2_words(p):
    if p is None:
        return [0] * 16
    return _fq_limbs(p[0].c[0]) + _fq_limbs(p[0].c[1]) + _fq_limbs(p[1].c[0]) + _fq_limbs(p[1].c[1])


@pytest.fixture(scope="module")
def params_file(tmp_path_factory, O):
    """a k = 2 params file in halo2's RawBytes layout, byte by byte: u32 LE k | g | g_lagrange | g2 | s_g2"""
    from oracle import pairing as PR
    g, gl = O.srs_from_tau(K, TAU)
    g2, s_g2 = _g2_words(PR.G2), _g2_words(PR.pt_mul(PR.G2, TAU))
    blob = struct.pack("<I", K)
    for pts in (g, gl):
        for p in pts:
            blob += struct.pack("<8Q", *[int(w) for w in p])
    blob += struct.pack("<16Q", *g2) + struct.pack("<16Q", *s_g2)
    path = tmp_path_factory.mktemp("params") / "kzg_bn254_2.srs"
    path.write_bytes(blob)
    return path, blob, g, gl, np.array(g2, dtype=np.uint64), np.array(s_g2, dtype=np.uint64)


def test_layout_is_read_back_exactly(params_file):
    from halo2_vectordb_amd import srs
    path, _blob, g, gl, g2, s_g2 = params_file
    file_k, rg, rgl, rg2, rs_g2 = srs.read_params_raw(path)
    assert file_k == K
    assert np.array_equal(rg, g) and np.array_equal(rgl, gl)
    assert np.array_equal(rg2, g2) and np.array_equal(rs_g2, s_g2)
    # below the file's k: the prefix of g only, no Lagrange bases (those are recomputed), the same G2 points
    file_k, rg, rgl, rg2, rs_g2 = srs.read_params_raw(path, k=1)
    assert file_k == K and rgl is None
    assert np.array_equal(rg, g[:2]) and np.array_equal(rg2, g2) and np.array_equal(rs_g2, s_g2)


def test_writer_produces_the_same_bytes(params_file, tmp_path):
    from halo2_vectordb_amd import srs
    _path, blob, g, gl, g2, s_g2 = params_file
    out = tmp_path / "written.srs"
    srs.write_params_raw(out, K, g, gl, g2, s_g2)
    assert out.read_bytes() == blob


@pytest.mark.parametrize("k", [1, 2, 5, 12])
def test_file_size(k):
    from halo2_vectordb_amd import srs
    assert srs.params_file_size(k) == 4 + 2 ** (k + 1) * 64 + 256


def test_params_file_size_matches_the_layout(params_file):
    from halo2_vectordb_amd import srs
    path, blob, *_ = params_file
    assert len(blob) == path.stat().st_size == srs.params_file_size(K) == 772


def test_refusals(params_file, tmp_path):
    from halo2_vectordb_amd.srs import ParamsKZG, read_params_g2
    path, blob, *_ = params_file
    cases = {"short": blob[:600], "header": blob[:3], "empty": b"", "long": blob + b"\0", "k_zero": struct.pack("<I", 0) + blob[4:],
             "k_huge": struct.pack("<I", 1 << 30) + blob[4:]}
    for name, data in cases.items():
        p = tmp_path / (name + ".srs")
        p.write_bytes(data)
        with pytest.raises(ValueError):
            ParamsKZG.read(p)
        with pytest.raises(ValueError):
            read_params_g2(p)
    with pytest.raises(ValueError, match="truncated"):
        ParamsKZG.read(tmp_path / "short.srs")
    with pytest.raises(ValueError, match="wrong length"):
        ParamsKZG.read(tmp_path / "long.srs")
    with pytest.raises(ValueError, match="params file's k"):
        ParamsKZG.read(path, k=K + 1)
    with pytest.raises(ValueError):
        ParamsKZG.read(path, k=0)


def test_read_params_g2_checks_the_points(params_file, tmp_path):
    from halo2_vectordb_amd.srs import read_params_g2
    path, blob, _g, _gl, g2, s_g2 = params_file
    rg2, rs_g2 = read_params_g2(path)
    assert np.array_equal(rg2, g2) and np.array_equal(rs_g2, s_g2)
    bad = bytearray(blob)
    bad[-128] ^= 1                                    # s_g2's x.c0: off the twist
    p = tmp_path / "bad_s_g2.srs"
    p.write_bytes(bytes(bad))
    with pytest.raises(ValueError, match="s_g2"):
        read_params_g2(p)


def _fq_sqrt(v):
    from oracle import pairing as PR
    r = pow(v % PR.Q, (PR.Q + 1) // 4, PR.Q)
    return r if r * r % PR.Q == v % PR.Q else None


def _fq2_sqrt(a0, a1):
    """a square root in Fq2 = Fq[u] / (u^2 + 1) (q = 3 mod 4), or None"""
    from oracle import pairing as PR
    Q = PR.Q
    alpha = _fq_sqrt(a0 * a0 + a1 * a1)
    if alpha is None:
        return None
    for al in (alpha, Q - alpha):
        x0 = _fq_sqrt((a0 + al) * pow(2, -1, Q))
        if x0:
            return x0, a1 * pow(2 * x0, -1, Q) % Q
    return None


def _twist_point_outside_g2():
    """a point of the twist y^2 = x^3 + 3 / (9 + u) that r does not annihilate (the twist's group has a cofactor of ~2^254)"""
    from oracle import pairing as PR
    for c in range(1, 200):
        x = PR.fq2(c, 1)
        rhs = x * x * x + PR.B2
        root = _fq2_sqrt(rhs.c[0] % PR.Q, rhs.c[1] % PR.Q)
        if root is None:
            continue
        p = (x, PR.fq2(*root))
        assert PR.on_twist(p)
        if PR.pt_mul(p, PR.R) is not None:
            return p
    raise AssertionError("no twist point found")


def test_g2_check_on_the_host():
    from oracle import pairing as PR
    from halo2_vectordb_amd.srs import g2_check
    gen = np.array(_g2_words(PR.G2), dtype=np.uint64)
    tau_g2 = np.array(_g2_words(PR.pt_mul(PR.G2, TAU)), dtype=np.uint64)
    assert g2_check([gen, tau_g2, np.zeros(16, dtype=np.uint64)]) == [True, True, True]
    off = gen.copy()
    off[8] ^= np.uint64(1)                            # y.c0 changed: off the twist
    outside = np.array(_g2_words(_twist_point_outside_g2()), dtype=np.uint64)
    big = gen.copy()
    big[4:8] = np.uint64(0xFFFFFFFFFFFFFFFF)          # x.c1 not below q
    assert g2_check([off, outside, big]) == [False, False, False]


def test_g2_check_abi():
    import ctypes
    from halo2_vectordb_amd import _lib
    from oracle import pairing as PR
    lib = _lib.load()
    pts = np.array([_g2_words(PR.G2), _g2_words(PR.pt_mul(PR.G2, 7)), _g2_words(_twist_point_outside_g2())], dtype=np.uint64)
    ok = ctypes.c_int(-1)
    assert lib.vdb_g2_check(pts.ctypes.data, ctypes.c_size_t(2), ctypes.byref(ok)) == 0 and ok.value == 1
    assert lib.vdb_g2_check(pts.ctypes.data, ctypes.c_size_t(3), ctypes.byref(ok)) == 0 and ok.value == 0
    assert lib.vdb_g2_check(None, ctypes.c_size_t(0), ctypes.byref(ok)) == 0 and ok.value == 1
    assert lib.vdb_g2_check(None, ctypes.c_size_t(1), ctypes.byref(ok)) == -3


def test_device_entry_points_need_a_gpu():
    import ctypes
    from halo2_vectordb_amd import _lib
    lib = _lib.load()
    if lib.vdb_device_count() > 0:
        pytest.skip("GPU present")
    buf = (ctypes.c_uint64 * 16)()
    a, b = ctypes.c_uint64(), ctypes.c_uint64()
    assert lib.vdb_g1_check_dev(buf, ctypes.c_size_t(1), ctypes.byref(a), ctypes.byref(b)) in (-1, -6)
    assert lib.vdb_g1_lagrange_from_monomial_dev(ctypes.c_uint32(1), buf, buf) in (-1, -6)
    assert lib.vdb_srs_downsize(ctypes.c_uint32(1), buf, buf) in (-1, -6)
