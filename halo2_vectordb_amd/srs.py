"""The SRS: the reference's "unsafe" universal setup, reproduced deterministically, and halo2's params files.

`gen_srs(k)` (/root/reference/src/scaffold/mod.rs:260, halo2-base `utils::fs::gen_srs`) creates
`ParamsKZG::<Bn256>::setup(k, ChaCha20Rng::from_seed(Default::default()))` when no params file exists; `setup` draws
ONE scalar, `s = Fr::random(rng)`, and derives g[i] = [s^i] G1, g_lagrange, [s] G2 from it.  With the all-zero seed
that scalar is a constant:

    Fr::random(rng) = Fr::from_u512([rng.next_u64(); 8])   = (first 64 keystream bytes, little-endian) mod r

[UPSTREAM-RECALL for the call chain — parity unpinned: the reference ships no params file to compare with; the RNG
itself is pinned by the RFC 7539 zero-key keystream vectors in tests/test_io_cpu.py.]  The powers are then computed on
the GPU by vdb_srs_setup_unsafe.

When params/kzg_bn254_{k}.srs exists, `gen_srs` reads it instead (ParamsKZG::read, SerdeFormat::RawBytes): that is how a deployment
brings a ceremony-derived SRS, typically one large file cut down with ParamsKZG::downsize(k).  ParamsKZG below reads, checks,
downsizes and writes such files; the downsize (g_to_lagrange, an inverse DFT over G1) runs on the GPU.
"""
import ctypes
import os
import struct

import numpy as np

from .protocol import R_MOD, fr_from_int


def _rotl(v, c):
    return ((v << c) & 0xFFFFFFFF) | (v >> (32 - c))


def _quarter(s, a, b, c, d):
    s[a] = (s[a] + s[b]) & 0xFFFFFFFF; s[d] = _rotl(s[d] ^ s[a], 16)
    s[c] = (s[c] + s[d]) & 0xFFFFFFFF; s[b] = _rotl(s[b] ^ s[c], 12)
    s[a] = (s[a] + s[b]) & 0xFFFFFFFF; s[d] = _rotl(s[d] ^ s[a], 8)
    s[c] = (s[c] + s[d]) & 0xFFFFFFFF; s[b] = _rotl(s[b] ^ s[c], 7)


def chacha20_block(key32, counter, stream=0):
    """One 64-byte ChaCha20 block in rand_chacha's layout: 64-bit block counter (words 12-13), 64-bit stream id
    (words 14-15); identical to RFC 7539 for stream 0 and counters below 2^32."""
    st = [0x61707865, 0x3320646E, 0x79622D32, 0x6B206574] + list(struct.unpack("<8I", key32))
    st += [counter & 0xFFFFFFFF, (counter >> 32) & 0xFFFFFFFF, stream & 0xFFFFFFFF, (stream >> 32) & 0xFFFFFFFF]
    w = st[:]
    for _ in range(10):
        _quarter(w, 0, 4, 8, 12); _quarter(w, 1, 5, 9, 13); _quarter(w, 2, 6, 10, 14); _quarter(w, 3, 7, 11, 15)
        _quarter(w, 0, 5, 10, 15); _quarter(w, 1, 6, 11, 12); _quarter(w, 2, 7, 8, 13); _quarter(w, 3, 4, 9, 14)
    return struct.pack("<16I", *[(a + b) & 0xFFFFFFFF for a, b in zip(w, st)])


class ChaCha20Rng:
    """rand_chacha::ChaCha20Rng::from_seed(seed): sequential keystream, next_u64 = two little-endian u32 words."""

    def __init__(self, seed=bytes(32)):
        self.key, self.counter, self.buf = bytes(seed), 0, b""

    def fill_bytes(self, n):
        while len(self.buf) < n:
            self.buf += chacha20_block(self.key, self.counter)
            self.counter += 1
        out, self.buf = self.buf[:n], self.buf[n:]
        return out

    def next_u64(self):
        return int.from_bytes(self.fill_bytes(8), "little")


def fr_random(rng):
    """halo2curves `Fr::random`: from_u512 of eight next_u64 limbs (little-endian), reduced mod r."""
    limbs = [rng.next_u64() for _ in range(8)]
    return sum(l << (64 * i) for i, l in enumerate(limbs)) % R_MOD


def gen_srs_tau(seed=bytes(32)):
    """The toxic-waste scalar of `gen_srs` (canonical integer)."""
    return fr_random(ChaCha20Rng(seed))


def tau_mont_limbs(tau):
    """canonical integer -> Montgomery form as 4 x u64 (the layout vdb_srs_setup_unsafe takes)"""
    return fr_from_int(tau)


# ---------------------------------------------------------------- halo2's params file (ParamsKZG::{read, write}, SerdeFormat::RawBytes)
# [UPSTREAM-RECALL] layout, parity unpinned (the reference ships no params file to compare with):
#   u32 LITTLE-endian k | g[2^k] | g_lagrange[2^k] | g2 | s_g2
# a G1 point is x then y, each the four little-endian 64-bit limbs of its Montgomery form (the words of this build's (n, 8) uint64
# arrays, identity (0, 0)); a G2 point is x.c0, x.c1, y.c0, y.c1 likewise (the vdb_g2 layout: 16 uint64).
MAX_PARAMS_K = 28          # Fr's two-adicity: no evaluation domain is larger


def params_file_size(k):
    return 4 + (2 << k) * 64 + 2 * 128


def _read_words(f, n_words):
    b = f.read(8 * n_words)
    if len(b) != 8 * n_words:
        raise ValueError("truncated params file")
    return np.frombuffer(b, dtype="<u8").astype(np.uint64)


def read_params_raw(path, k=None):
    """The arrays of a params file as they lie on disk, no point checked: (file_k, g, g_lagrange, g2, s_g2) with g the first 2^k
    monomial points ((2^k, 8) uint64), g_lagrange the file's (2^k, 8) when k is the file's k and None otherwise (only the prefix of
    g is read: the rest of a large file is skipped), g2 and s_g2 (16,) uint64.  ValueError on a truncated file, a length that does
    not fit the header, or k above the file's."""
    size = os.path.getsize(path)
    with open(path, "rb") as f:
        head = f.read(4)
        if len(head) != 4:
            raise ValueError("truncated params file: no header")
        file_k = int.from_bytes(head, "little")
        if not 1 <= file_k <= MAX_PARAMS_K:
            raise ValueError(f"params file: implausible k = {file_k}")
        want = params_file_size(file_k)
        if size < want:
            raise ValueError(f"truncated params file: {size} bytes where k = {file_k} takes {want}")
        if size != want:
            raise ValueError(f"params file has the wrong length: {size} bytes where k = {file_k} takes {want}")
        k = file_k if k is None else int(k)
        if not 1 <= k <= file_k:
            raise ValueError(f"k = {k} is not within 1 .. {file_k}, the params file's k")
        n = 1 << k
        g = _read_words(f, 8 * n).reshape(n, 8)
        gl = None
        if k == file_k:
            gl = _read_words(f, 8 * n).reshape(n, 8)
        f.seek(4 + (2 << file_k) * 64)
        g2, s_g2 = _read_words(f, 16), _read_words(f, 16)
    return file_k, g, gl, g2, s_g2


def write_params_raw(path, k, g, g_lagrange, g2, s_g2):
    n = 1 << k
    with open(path, "wb") as f:
        f.write(struct.pack("<I", k))
        for arr, shape in ((g, (n, 8)), (g_lagrange, (n, 8)), (g2, (16,)), (s_g2, (16,))):
            arr = np.ascontiguousarray(arr, dtype="<u8")
            if arr.shape != shape:
                raise ValueError(f"params: an array of shape {arr.shape} where {shape} belongs")
            f.write(arr.tobytes())


def g2_check(points):
    """vdb_g2_check of each (16,) uint64 point (host): a list of booleans"""
    from . import _lib
    out = []
    for p in points:
        p = np.ascontiguousarray(p, dtype=np.uint64).reshape(16)
        ok = ctypes.c_int(0)
        _lib.check(_lib.load().vdb_g2_check(p.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(1), ctypes.byref(ok)))
        out.append(bool(ok.value))
    return out


def read_params_g2(path):
    """(g2, s_g2) of a params file, both checked to be G2 points: all a verifier needs of it.  ValueError otherwise."""
    _, _, _, g2, s_g2 = read_params_raw(path, k=1)
    _check_g2(g2, s_g2)
    return g2, s_g2


def _check_g2(g2, s_g2):
    for name, ok in zip(("g2", "s_g2"), g2_check([g2, s_g2])):
        if not ok:
            raise ValueError(f"params file: {name} is not a point of G2")


def g1_check(points):
    """vdb_g1_check_dev over (n, 8) host points: (number of invalid points, index of the first; n when none)"""
    from . import _lib
    from .api import DeviceBuffer
    points = np.ascontiguousarray(points, dtype=np.uint64).reshape(-1, 8)
    n_bad, first = ctypes.c_uint64(), ctypes.c_uint64()
    d = DeviceBuffer(max(points.nbytes, 64))
    try:
        if len(points):
            d.upload(points)
        _lib.check(_lib.init().vdb_g1_check_dev(d.ptr, ctypes.c_size_t(len(points)), ctypes.byref(n_bad), ctypes.byref(first)))
    finally:
        d.free()
    return n_bad.value, first.value


def _raise_bad(name, n_bad, first):
    if n_bad:
        raise ValueError(f"params file: {name}[{first}] is not a point of G1 (coordinate not below q, or off the curve); {n_bad} such points")


def lagrange_from_monomial(g):
    """halo2's g_to_lagrange on the device (vdb_g1_lagrange_from_monomial_dev): (2^k, 8) monomial points -> (2^k, 8) Lagrange points"""
    from . import _lib
    from .api import DeviceBuffer
    g = np.ascontiguousarray(g, dtype=np.uint64).reshape(-1, 8)
    n = len(g)
    k = n.bit_length() - 1
    if n < 2 or n != 1 << k:
        raise ValueError("g_to_lagrange needs 2^k points, k >= 1")
    d = DeviceBuffer(g.nbytes)
    try:
        d.upload(g)
        _lib.check(_lib.init().vdb_g1_lagrange_from_monomial_dev(ctypes.c_uint32(k), d.ptr, d.ptr))
        return d.download((n, 8))
    finally:
        d.free()


def _g1_generator():
    q = 0x30644E72E131A029B85045B68181585D97816A916871CA8D3C208C16D87CFD47
    return np.array([((v << 256) % q >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for v in (1, 2) for i in range(4)], dtype=np.uint64)


class ParamsKZG:
    """halo2's ParamsKZG<Bn256>: k, the monomial bases g[i] = [tau^i] G1, the Lagrange bases g_lagrange[i] = [L_i(tau)] G1 ((2^k, 8)
    uint64 Montgomery affine each), g2 = G2's generator and s_g2 = [tau] G2 ((16,) uint64 each).  The prover takes g and g_lagrange
    (pipeline.KmeansHotPath(params=...)), the verifier g2 and s_g2 (verifier.VerifyingKey.read(params=...))."""

    def __init__(self, k, g, g_lagrange, g2, s_g2):
        self.k = int(k)
        n = 1 << self.k
        self.g = np.ascontiguousarray(g, dtype=np.uint64).reshape(n, 8)
        self.g_lagrange = np.ascontiguousarray(g_lagrange, dtype=np.uint64).reshape(n, 8)
        self.g2 = np.ascontiguousarray(g2, dtype=np.uint64).reshape(16)
        self.s_g2 = np.ascontiguousarray(s_g2, dtype=np.uint64).reshape(16)

    @classmethod
    def read(cls, path, k=None):
        """ParamsKZG::read (RawBytes) of a params file, followed by ParamsKZG::downsize(k) when k is below the file's: then only the
        first 2^k monomial points are read and g_lagrange is computed from them on the device.  Every point that is used is checked
        as halo2's reader checks it (on the device for G1; g2 and s_g2 on the host, where their subgroup is checked too).
        ValueError on a truncated file, a wrong length, k above the file's, or a bad point (named with its index)."""
        file_k, g, gl, g2, s_g2 = read_params_raw(path, k)
        k = file_k if k is None else int(k)
        _check_g2(g2, s_g2)
        _raise_bad("g", *g1_check(g))
        if gl is None:
            gl = lagrange_from_monomial(g)
        else:
            _raise_bad("g_lagrange", *g1_check(gl))
        return cls(k, g, gl, g2, s_g2)

    @classmethod
    def setup_unsafe(cls, k, tau=None):
        """ParamsKZG::setup with a known scalar — the file halo2-base's gen_srs writes when none exists (tau = None: its fixed-seed
        scalar, gen_srs_tau).  Test and benchmark setups only: whoever knows tau can forge openings."""
        from . import api
        from .verifier import _g2_generator_times
        tau = gen_srs_tau() if tau is None else int(tau) % R_MOD
        g, gl = api.srs_setup_unsafe(k, tau_mont_limbs(tau))
        return cls(k, g, gl, _g2_generator_times(1), _g2_generator_times(tau))

    def write(self, path):
        """ParamsKZG::write (RawBytes): the file read() reads"""
        write_params_raw(path, self.k, self.g, self.g_lagrange, self.g2, self.s_g2)

    def downsize(self, k):
        """ParamsKZG::downsize(k): the first 2^k monomial points and their Lagrange bases (computed on the device); G2 unchanged"""
        k = int(k)
        if k == self.k:
            return self
        if not 1 <= k < self.k:
            raise ValueError(f"cannot downsize params of k = {self.k} to k = {k}")
        g = self.g[: 1 << k]
        return ParamsKZG(k, g, lagrange_from_monomial(g), self.g2, self.s_g2)

    def check(self, seed=0):
        """Is this an SRS at all?  halo2 does not ask (this is an opt-in addition for files from elsewhere).  True when g[0] and g2
        are the generators, the powers chain holds — e(sum r_i g[i+1], g2) = e(sum r_i g[i], s_g2) — and g_lagrange belongs to g:
        sum r_i g_lagrange[i] = sum c_j g[j] with c = iNTT(r); r random from `seed` (two MSMs each, one pairing)."""
        from . import api
        from .verifier import _g2_generator_times, _neg_point, msm_points, pairing_check
        if not np.array_equal(self.g[0], _g1_generator()) or not np.array_equal(self.g2, _g2_generator_times(1)):
            return False
        n = 1 << self.k
        rng = np.random.default_rng(seed)

        def scalars(m):   # below 2^253 < r: valid Montgomery words of random field elements
            r = rng.integers(0, 2**64, size=(m, 4), dtype=np.uint64)
            r[:, 3] &= np.uint64((1 << 61) - 1)
            return r

        r = scalars(n - 1)
        a, b = msm_points(self.g[1:], r), msm_points(self.g[:-1], r)
        if not pairing_check(np.stack([a, _neg_point(b)]), np.stack([self.g2, self.s_g2])):
            return False
        r = scalars(n)
        c = api.lagrange_to_coeff(r[None])[0]
        return bool(np.array_equal(msm_points(self.g_lagrange, r), msm_points(self.g, c)))
