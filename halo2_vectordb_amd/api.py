"""numpy-facing wrappers over the C ABI (include/vdb.h).  Thin plumbing only: every function
marshals numpy buffers into one `vdb_*` call.  Field elements are uint64 arrays (..., 4):
little-endian limbs, Montgomery form (halo2curves layout).  G1 points are (..., 8): x then y.
"""
import contextlib
import ctypes

import numpy as np

from . import _lib
from ._lib import VdbError, check  # noqa: F401

NTT_INVERSE_SCALE = 1


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _sz(n):
    return ctypes.c_size_t(int(n))


def _fr(a):
    a = np.ascontiguousarray(a, dtype=np.uint64)
    assert a.shape[-1] == 4
    return a


def init(device=None):
    return _lib.init(device)


def shutdown():
    _lib.load().vdb_shutdown()
    _lib._inited = None


def device_count():
    return _lib.load().vdb_device_count()


def init_devices(n):
    """Bind GPUs 0 .. n-1 in this process (vdb_init_devices); this thread works on device 0 until set_device."""
    return _lib.init_devices(n)


def set_device(device):
    check(_lib.load().vdb_set_device(int(device)))


def current_device():
    return _lib.load().vdb_current_device()


def devices_bound():
    return _lib.load().vdb_devices_bound()


# ---------------------------------------------------------------- field helpers
def _binop(name, a, b):
    L = _lib.init()
    a, b = _fr(a), _fr(b)
    o = np.empty_like(a)
    check(getattr(L, name)(_p(a), _p(b), _p(o), _sz(a.size // 4)))
    return o


def fr_mul(a, b):
    return _binop("vdb_fr_mul", a, b)


def fr_add(a, b):
    return _binop("vdb_fr_add", a, b)


def fr_sub(a, b):
    return _binop("vdb_fr_sub", a, b)


def _unop(name, a):
    L = _lib.init()
    a = _fr(a)
    o = np.empty_like(a)
    check(getattr(L, name)(_p(a), _p(o), _sz(a.size // 4)))
    return o


def fr_from_canonical(a):
    return _unop("vdb_fr_from_canonical", a)


def fr_to_canonical(a):
    return _unop("vdb_fr_to_canonical", a)


def fr_batch_invert(a):
    return _unop("vdb_fr_batch_invert", a)


def bench_fr_mul(threads=256 * 256 * 8, iters=2000):
    L = _lib.init()
    out = ctypes.c_double(0)
    check(L.vdb_bench_fr_mul(_sz(threads), _sz(iters), ctypes.byref(out)))
    return out.value


def root_of_unity(k):
    o = np.zeros(4, dtype=np.uint64)
    check(_lib.load().vdb_fr_root_of_unity(ctypes.c_uint32(k), _p(o)))
    return o


# ---------------------------------------------------------------- NTT
def _col_ptrs(cols):
    ptrs = (ctypes.c_void_p * len(cols))(*[c.ctypes.data for c in cols])
    return ptrs


def ntt_batch(cols, omega, flags=0):
    """cols: (n_cols, n, 4); returns transformed copy (host-pointer entry point)."""
    L = _lib.init()
    cols = np.array(cols, dtype=np.uint64, copy=True)
    n_cols, n = cols.shape[0], cols.shape[1]
    views = [cols[i] for i in range(n_cols)]
    omega = _fr(omega)
    check(L.vdb_ntt_batch(_col_ptrs(views), _sz(n_cols), ctypes.c_uint32(n.bit_length() - 1), _p(omega), ctypes.c_int(flags)))
    return cols


def lagrange_to_coeff(cols):
    L = _lib.init()
    cols = np.array(cols, dtype=np.uint64, copy=True)
    n_cols, n = cols.shape[0], cols.shape[1]
    views = [cols[i] for i in range(n_cols)]
    check(L.vdb_lagrange_to_coeff(_col_ptrs(views), _sz(n_cols), ctypes.c_uint32(n.bit_length() - 1)))
    return cols


def coeff_to_extended(cols, ext_k=2):
    L = _lib.init()
    cols = _fr(cols)
    n_cols, n = cols.shape[0], cols.shape[1]
    out = np.zeros((n_cols, n << ext_k, 4), dtype=np.uint64)
    check(L.vdb_coeff_to_extended(_col_ptrs([cols[i] for i in range(n_cols)]), _col_ptrs([out[i] for i in range(n_cols)]),
                                  _sz(n_cols), ctypes.c_uint32(n.bit_length() - 1), ctypes.c_uint32(ext_k)))
    return out


# ---------------------------------------------------------------- SRS / MSM
class Srs:
    """Device-resident KZG bases + fixed-base window tables (vdb_srs_load)."""

    def __init__(self, k, g=None, g_lagrange=None, window_bits=0):
        """window_bits: Pippenger window (0 = default, tuned for witness columns; 14 suits columns of full-width scalars)"""
        self.L = _lib.init()
        self.k = k
        h = ctypes.c_void_p()
        ga = np.ascontiguousarray(g, dtype=np.uint64) if g is not None else None
        gl = np.ascontiguousarray(g_lagrange, dtype=np.uint64) if g_lagrange is not None else None
        check(self.L.vdb_srs_load_window(ctypes.c_uint32(k), _p(ga) if ga is not None else None, _p(gl) if gl is not None else None,
                                         ctypes.c_uint32(window_bits), ctypes.byref(h)))
        self.h = h

    def info(self):
        k, c, w = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint32()
        check(self.L.vdb_srs_info(self.h, ctypes.byref(k), ctypes.byref(c), ctypes.byref(w)))
        return k.value, c.value, w.value

    def free(self):
        if self.h is not None:
            self.L.vdb_srs_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class SrsAll:
    """One Srs handle per bound device, the bases replicated (vdb_srs_load_all); commits batches of columns over all of them."""

    def __init__(self, k, g=None, g_lagrange=None, window_bits=0):
        self.L = _lib.init()
        self.k = k
        n = devices_bound()
        self.handles = (ctypes.c_void_p * n)()
        ga = np.ascontiguousarray(g, dtype=np.uint64) if g is not None else None
        gl = np.ascontiguousarray(g_lagrange, dtype=np.uint64) if g_lagrange is not None else None
        check(self.L.vdb_srs_load_all(ctypes.c_uint32(k), _p(ga) if ga is not None else None, _p(gl) if gl is not None else None,
                                      ctypes.c_uint32(window_bits), self.handles, n))

    def devices(self):
        out = []
        for h in self.handles:
            d = ctypes.c_int(-1)
            check(self.L.vdb_srs_device(h, ctypes.byref(d)))
            out.append(d.value)
        return out

    def msm_batch(self, cols, basis=1):
        """cols: (n_cols, n, 4) host scalars -> (n_cols, 8): device i commits the i-th contiguous block of the columns"""
        cols = _fr(cols)
        n_cols, n = cols.shape[0], cols.shape[1]
        out = np.zeros((n_cols, 8), dtype=np.uint64)
        check(self.L.vdb_msm_batch_multi(self.handles, len(self.handles), ctypes.c_int(basis), _col_ptrs([cols[i] for i in range(n_cols)]),
                                         _sz(n_cols), _sz(n), _p(out)))
        return out

    def free(self):
        for i, h in enumerate(self.handles):
            if h:
                self.L.vdb_srs_free(h)
                self.handles[i] = None


def ntt_batch_multi(cols, omega, flags=0):
    """ntt_batch with the columns cut into one block per bound device"""
    L = _lib.init()
    cols = np.array(cols, dtype=np.uint64, copy=True)
    n_cols, n = cols.shape[0], cols.shape[1]
    omega = _fr(omega)
    check(L.vdb_ntt_batch_multi(_col_ptrs([cols[i] for i in range(n_cols)]), _sz(n_cols), ctypes.c_uint32(n.bit_length() - 1), _p(omega), ctypes.c_int(flags)))
    return cols


def srs_setup_unsafe(k, tau_mont):
    """(g, g_lagrange) for a known tau (Montgomery Fr limbs)."""
    lib = _lib.init()
    tau = _fr(tau_mont)
    g = np.zeros((1 << k, 8), dtype=np.uint64)
    gl = np.zeros((1 << k, 8), dtype=np.uint64)
    check(lib.vdb_srs_setup_unsafe(ctypes.c_uint32(k), _p(tau), _p(g), _p(gl)))
    return g, gl


def msm_batch(srs, cols, basis=1):
    """cols: (n_cols, n, 4) Montgomery scalars (host) -> (n_cols, 8) affine points."""
    cols = _fr(cols)
    n_cols, n = cols.shape[0], cols.shape[1]
    out = np.zeros((n_cols, 8), dtype=np.uint64)
    check(srs.L.vdb_msm_batch(srs.h, ctypes.c_int(basis), _col_ptrs([cols[i] for i in range(n_cols)]), _sz(n_cols), _sz(n), _p(out)))
    return out


def msm(srs, scalars, basis=1):
    scalars = _fr(scalars)
    out = np.zeros(8, dtype=np.uint64)
    check(srs.L.vdb_msm(srs.h, ctypes.c_int(basis), _p(scalars), _sz(scalars.size // 4), _p(out)))
    return out


def msm_batch_dev(srs, dev_ptr, n_cols, n, basis=1):
    out = np.zeros((n_cols, 8), dtype=np.uint64)
    check(srs.L.vdb_msm_batch_dev(srs.h, ctypes.c_int(basis), dev_ptr, _sz(n_cols), _sz(n), _p(out)))
    return out


# ---------------------------------------------------------------- fixed point + witness streams
METRICS = dict(euclidean=0, cosine=1, manhattan=2, hamming=3)


def quantize(x, P=48):
    x = np.ascontiguousarray(x, dtype=np.float64)
    o = np.zeros(x.shape + (4,), dtype=np.uint64)
    check(_lib.load().vdb_fp_quantize(ctypes.c_uint32(P), _p(x), _p(o), _sz(x.size)))
    return o


def dequantize(a, P=48):
    a = _fr(a)
    o = np.zeros(a.shape[:-1], dtype=np.float64)
    check(_lib.load().vdb_fp_dequantize(ctypes.c_uint32(P), _p(a), _p(o), _sz(a.size // 4)))
    return o


def _u64():
    return ctypes.c_uint64(0)


def _split_flags(flags):
    """flag byte per advice cell: bit 0 = gate start (selector), bit 1 = data-independent constant cell"""
    if flags is None:
        return dict(selectors=None, const_mask=None, flags=None)
    return dict(selectors=flags & 1, const_mask=(flags >> 1) & 1, flags=flags)


def wit_distance(metric, a, b, P=48, L=13, selectors=False):
    """a, b: (n_pairs, dim, 4).  Returns dict(stream, lookup, selectors, result)."""
    lib = _lib.init()
    a, b = _fr(a), _fr(b)
    n, dim = a.shape[0], a.shape[1]
    cells, lk = _u64(), _u64()
    check(lib.vdb_wit_distance_size(METRICS[metric], ctypes.c_uint32(P), ctypes.c_uint32(L), _sz(n), _sz(dim), ctypes.byref(cells), ctypes.byref(lk)))
    stream = np.zeros((cells.value, 4), dtype=np.uint64)
    lookup = np.zeros((lk.value, 4), dtype=np.uint64)
    sel = np.zeros(cells.value, dtype=np.uint8) if selectors else None
    res = np.zeros((n, 4), dtype=np.uint64)
    check(lib.vdb_wit_distance(METRICS[metric], ctypes.c_uint32(P), ctypes.c_uint32(L), _p(a), _p(b), _sz(n), _sz(dim), _p(stream), _p(lookup),
                               _p(sel) if selectors else None, _p(res)))
    return dict(stream=stream, lookup=lookup, **_split_flags(sel), result=res)


FP_OPS = dict(qadd=0, qsub=1, qmul=2, qdiv=3, neg=4, qabs=5, is_neg=6, qmin=7, qsqrt=8, qlog2=9, qexp2=10, qlog=11, qexp=12, qpow=13, bit_xor=14,
              cond_neg=15, signed_div_scale=16, qmax=17, sign=18, clip=19, qmod=20, qsin=21, qcos=22, qtan=23, qsinh=24, qcosh=25, qtanh=26)


def wit_fp_op(op, a, b=None, P=48, L=13, selectors=False):
    """n independent FixedPointChip calls op(a_i [, b_i]) (vdb_wit_fp_op): a, b (n, 4) quantized values; instance i's cells are
    stream[i * cells_per_call : (i + 1) * cells_per_call]"""
    lib = _lib.init()
    a = _fr(a).reshape(-1, 4)
    n = a.shape[0]
    b = None if b is None else _fr(b).reshape(-1, 4)
    assert b is None or b.shape == a.shape
    cells, lk = _u64(), _u64()
    check(lib.vdb_wit_fp_op_size(FP_OPS[op], ctypes.c_uint32(P), ctypes.c_uint32(L), _sz(n), ctypes.byref(cells), ctypes.byref(lk)))
    stream = np.zeros((cells.value, 4), dtype=np.uint64)
    lookup = np.zeros((lk.value, 4), dtype=np.uint64)
    sel = np.zeros(cells.value, dtype=np.uint8) if selectors else None
    res = np.zeros((n, 4), dtype=np.uint64)
    check(lib.vdb_wit_fp_op(FP_OPS[op], ctypes.c_uint32(P), ctypes.c_uint32(L), _p(a), _p(b) if b is not None else None, _sz(n), _p(stream), _p(lookup),
                            _p(sel) if selectors else None, _p(res)))
    return dict(stream=stream, lookup=lookup, **_split_flags(sel), result=res)


@contextlib.contextmanager
def wit_window(adv, lookup):
    """Within the block the witness entry points store only the stream cells in [adv[0], adv[1]) and the lookup cells in
    [lookup[0], lookup[1]) — a rank's window, positions counted from the stream pointers handed to each call; every value is still
    computed (vdb_wit_set_window).  The full window is restored on the way out."""
    lib = _lib.init()
    check(lib.vdb_wit_set_window(ctypes.c_uint64(adv[0]), ctypes.c_uint64(adv[1]), ctypes.c_uint64(lookup[0]), ctypes.c_uint64(lookup[1])))
    try:
        yield
    finally:
        check(lib.vdb_wit_set_window(ctypes.c_uint64(0), ctypes.c_uint64(2**64 - 1), ctypes.c_uint64(0), ctypes.c_uint64(2**64 - 1)))


def wit_nearest(metric, query, vectors, P=48, L=13, selectors=False):
    """nearest_vector(query (dim, 4), vectors (n, dim, 4)): wit_nearest_batch of the one query; dict(stream, lookup, selectors,
    indicator (n, 4), result (dim, 4))"""
    out = wit_nearest_batch(metric, _fr(query)[None], vectors, P, L, selectors)
    out["indicator"], out["result"] = out.pop("indicators")[0], out.pop("results")[0]
    return out


def wit_nearest_batch(metric, queries, vectors, P=48, L=13, selectors=False):
    """nearest_vector of every row of `queries` (q, dim, 4) over the one database `vectors` (n, dim, 4), the calls end to end in the
    streams: wit_nearest_topk's one round; dict(stream, lookup, selectors, indicators (q, n, 4), results (q, dim, 4))"""
    out = wit_nearest_topk(metric, queries, vectors, 1, P, L, selectors)
    out["indicators"], out["results"] = out["indicators"][:, 0], out["results"][:, 0]
    return out


def wit_nearest_topk(metric, queries, vectors, topk, P=48, L=13, selectors=False):
    """the `topk` nearest rows of the database `vectors` (n, dim, 4) for every row of `queries` (q, dim, 4), nearest first
    (vdb_wit_nearest_topk: nearest_vector's closing stages once per round, a round's winners masked before the next; on a tie every
    tied row is a winner of that round and its result is the last of them): dict(stream, lookup, selectors, indicators (q, topk, n, 4),
    results (q, topk, dim, 4))"""
    lib = _lib.init()
    queries, vectors = _fr(queries), _fr(vectors)
    q, n, dim = queries.shape[0], vectors.shape[0], vectors.shape[1]
    assert queries.shape[1] == dim
    cells, lk = _u64(), _u64()
    check(lib.vdb_wit_nearest_topk_size(METRICS[metric], ctypes.c_uint32(P), ctypes.c_uint32(L), _sz(q), _sz(n), _sz(dim), _sz(topk), ctypes.byref(cells),
                                        ctypes.byref(lk)))
    stream = np.zeros((cells.value, 4), dtype=np.uint64)
    lookup = np.zeros((lk.value, 4), dtype=np.uint64)
    sel = np.zeros(cells.value, dtype=np.uint8) if selectors else None
    ind = np.zeros((q, topk, n, 4), dtype=np.uint64)
    res = np.zeros((q, topk, dim, 4), dtype=np.uint64)
    check(lib.vdb_wit_nearest_topk(METRICS[metric], ctypes.c_uint32(P), ctypes.c_uint32(L), _p(queries), _p(vectors), _sz(q), _sz(n), _sz(dim), _sz(topk),
                                   _p(stream), _p(lookup), _p(sel) if selectors else None, _p(ind), _p(res)))
    return dict(stream=stream, lookup=lookup, **_split_flags(sel), indicators=ind, results=res)


def nearest_values(metric, queries, vectors, P=48, L=13):
    """nearest_vector's answer for every row of `queries` (q, dim, 4) over `vectors` (n, dim, 4) as values alone (vdb_nearest_values: no
    stream is emitted): (idx (q,) uint32, dist (q, 4)), dist the minimum of the circuit's fixed-point distance(vector_i, query) bit for
    bit, idx the last i at it"""
    lib = _lib.init()
    queries, vectors = _fr(queries), _fr(vectors)
    q, n, dim = queries.shape[0], vectors.shape[0], vectors.shape[1]
    assert queries.ndim == 3 and vectors.ndim == 3 and queries.shape[1] == dim
    idx = np.zeros(q, dtype=np.uint32)
    dist = np.zeros((q, 4), dtype=np.uint64)
    check(lib.vdb_nearest_values(ctypes.c_uint32(P), ctypes.c_uint32(L), METRICS[metric], _p(queries), _p(vectors), _sz(q), _sz(n), _sz(dim), _p(idx),
                                 _p(dist)))
    return idx, dist


def nearest_topk_values(metric, queries, vectors, p, P=48, L=13):
    """the winners of p rounds of top-k for every row of `queries` (q, dim, 4) over `vectors` (n, dim, 4) as values alone
    (vdb_nearest_topk_values: no stream is emitted): (idx (q, p) uint32, dist (q, p, 4)), dist[., r] the minimum round r's qmin chain ends
    in, idx[., r] the last i at it — the vector the round's select_by_indicator states"""
    lib = _lib.init()
    queries, vectors = _fr(queries), _fr(vectors)
    q, n, dim, p = queries.shape[0], vectors.shape[0], vectors.shape[1], int(p)
    assert queries.ndim == 3 and vectors.ndim == 3 and queries.shape[1] == dim
    idx = np.zeros((q, max(p, 0)), dtype=np.uint32)
    dist = np.zeros((q, max(p, 0), 4), dtype=np.uint64)
    check(lib.vdb_nearest_topk_values(ctypes.c_uint32(P), ctypes.c_uint32(L), METRICS[metric], _p(queries), _p(vectors), _sz(q), _sz(n), _sz(dim), _sz(p),
                                      _p(idx), _p(dist)))
    return idx, dist


def wit_kmeans(metric, vectors, K, I, P=48, L=13, zero_cached=False, selectors=False):
    lib = _lib.init()
    vectors = _fr(vectors)
    n, dim = vectors.shape[0], vectors.shape[1]
    cells, lk = _u64(), _u64()
    check(lib.vdb_wit_kmeans_size(METRICS[metric], ctypes.c_uint32(P), ctypes.c_uint32(L), _sz(n), _sz(dim), _sz(K), _sz(I), int(zero_cached),
                                  ctypes.byref(cells), ctypes.byref(lk)))
    stream = np.zeros((cells.value, 4), dtype=np.uint64)
    lookup = np.zeros((lk.value, 4), dtype=np.uint64)
    sel = np.zeros(cells.value, dtype=np.uint8) if selectors else None
    cent = np.zeros((K, dim, 4), dtype=np.uint64)
    ind = np.zeros((n, K, 4), dtype=np.uint64)
    check(lib.vdb_wit_kmeans(METRICS[metric], ctypes.c_uint32(P), ctypes.c_uint32(L), _p(vectors), _sz(n), _sz(dim), _sz(K), _sz(I), int(zero_cached),
                             _p(stream), _p(lookup), _p(sel) if selectors else None, _p(cent), _p(ind)))
    return dict(stream=stream, lookup=lookup, **_split_flags(sel), centroids=cent, indicators=ind)


def wit_merkle(vectors, zero_cached=False, selectors=False):
    lib = _lib.init()
    vectors = _fr(vectors)
    n, dim = vectors.shape[0], vectors.shape[1]
    cells = _u64()
    check(lib.vdb_wit_merkle_size(_sz(n), _sz(dim), int(zero_cached), ctypes.byref(cells)))
    stream = np.zeros((cells.value, 4), dtype=np.uint64)
    sel = np.zeros(cells.value, dtype=np.uint8) if selectors else None
    root = np.zeros(4, dtype=np.uint64)
    check(lib.vdb_wit_merkle(_p(vectors), _sz(n), _sz(dim), int(zero_cached), _p(stream), _p(sel) if selectors else None, _p(root)))
    return dict(stream=stream, **_split_flags(sel), root=root)


def merkle_levels(n):
    """(lp, depth) of merkle_commitment's tree over n vectors: the padded leaf count and the number of levels above the leaves"""
    lp = 1
    while lp < n:
        lp <<= 1
    return lp, lp.bit_length() - 1


def merkle_tree_build(vectors):
    """the digests of every level of merkle_commitment's tree over `vectors` (n, dim, 4), as vdb_merkle_tree_build_dev leaves them on
    the device: (2 lp, 4), the leaves first, the root at entry 2 lp - 2"""
    lib = _lib.init()
    vectors = _fr(vectors)
    n, dim = vectors.shape[0], vectors.shape[1]
    lp, _ = merkle_levels(n)
    d_vec, d_lv = DeviceBuffer(vectors.nbytes), DeviceBuffer(2 * lp * 32)
    try:
        d_vec.upload(vectors)
        check(lib.vdb_merkle_tree_build_dev(d_vec.ptr, _sz(n), _sz(dim), d_lv.ptr))
        return d_lv.download((2 * lp, 4))
    finally:
        d_vec.free()
        d_lv.free()


def merkle_tree_grow(levels, n, grow):
    """the tree `levels` (merkle_tree_build's array over n vectors) with its padded leaf count doubled `grow` times, the new slots
    empty (vdb_merkle_tree_grow_dev): (2 lp 2^grow, 4) in the same layout"""
    lib = _lib.init()
    levels = np.ascontiguousarray(levels, dtype=np.uint64)
    lp, _ = merkle_levels(n)
    assert levels.shape == (2 * lp, 4) and grow >= 0
    d_lv, d_out = DeviceBuffer(levels.nbytes), DeviceBuffer(2 * (lp << grow) * 32)
    try:
        d_lv.upload(levels)
        check(lib.vdb_merkle_tree_grow_dev(d_lv.ptr, _sz(n), int(grow), d_out.ptr))
        return d_out.download((2 * (lp << grow), 4))
    finally:
        d_lv.free()
        d_out.free()


def wit_merkle_update(levels, n, new_vectors, indices, selectors=False, kinds=None, grow=0):
    """a batch of Merkle path updates (vdb_wit_merkle_update_ops) against the tree `levels` (merkle_tree_build's array over n vectors,
    after merkle_tree_grow when grow > 0): slot indices[j] takes the next row of new_vectors (w, dim, 4), or is emptied where
    kinds[j] = 1 (None: all writes), in order.  dict(stream, selectors, input_cells, public (3 m + 2, 4): [old root | idx, old leaf,
    new leaf per update | new root], levels: the tree after the batch)"""
    lib = _lib.init()
    new_vectors = _fr(new_vectors)
    levels = np.array(levels, dtype=np.uint64, copy=True)
    idx = np.ascontiguousarray(indices, dtype=np.uint64)
    m, dim = idx.shape[0], new_vectors.shape[1]
    kinds = np.zeros(m, dtype=np.uint8) if kinds is None else np.ascontiguousarray(kinds, dtype=np.uint8)
    assert idx.shape == (m,) and kinds.shape == (m,) and levels.shape == (2 * (merkle_levels(n)[0] << grow), 4)
    assert new_vectors.shape[0] == int((kinds == 0).sum()), "one new vector per write"
    cells, n_in = _u64(), _u64()
    check(lib.vdb_wit_merkle_update_ops_size(_sz(n), _sz(dim), _sz(m), _p(kinds), int(grow), ctypes.byref(cells), ctypes.byref(n_in)))
    stream = np.zeros((cells.value, 4), dtype=np.uint64)
    sel = np.zeros(cells.value, dtype=np.uint8) if selectors else None
    pub = np.zeros((3 * m + 2, 4), dtype=np.uint64)
    check(lib.vdb_wit_merkle_update_ops(_p(levels), _sz(n), _sz(dim), int(grow), _p(new_vectors) if new_vectors.shape[0] else None, _p(idx), _p(kinds),
                                        _sz(m), _p(stream), _p(sel) if selectors else None, _p(pub)))
    return dict(stream=stream, **_split_flags(sel), input_cells=n_in.value, public=pub, levels=levels)


def ann_forest_layout(cluster_ids, K):
    """(digests of the forest of vdb_ann_index_build_dev, the K + 2 digest offsets at which its segments start): segment c < K is the tree
    of cluster c, segment K the centroids' tree (vdb_ann_index_forest_size; VdbError on an id >= K, an empty cluster or K = 0)"""
    lib = _lib.init()
    ids = np.ascontiguousarray(cluster_ids, dtype=np.uint32)
    digests, seg = _u64(), np.zeros(int(K) + 2, dtype=np.uint64)
    check(lib.vdb_ann_index_forest_size(_p(ids), _sz(ids.size), _sz(K), ctypes.byref(digests), _p(seg)))
    return digests.value, seg


def ann_index_build(vectors, cluster_ids, centroids):
    """the index of approximate-nearest-neighbour queries (vdb_ann_index_build_dev) over `vectors` (n, dim, 4), their cluster ids (n,) and
    `centroids` (K, dim, 4), downloaded: dict(grouped (n, dim, 4), slots (n,), offsets (K + 1,), forest (digests, 4), segments (K + 2,),
    roots (K + 2, 4): [centroids' root | cluster roots | index root])"""
    lib = _lib.init()
    vectors, centroids = _fr(vectors), _fr(centroids)
    n, dim, K = vectors.shape[0], vectors.shape[1], centroids.shape[0]
    ids = np.ascontiguousarray(cluster_ids, dtype=np.uint32)
    assert ids.shape == (n,) and centroids.shape[1] == dim
    digests, seg = ann_forest_layout(ids, K)
    bufs = [DeviceBuffer(vectors.nbytes), DeviceBuffer(centroids.nbytes), DeviceBuffer(vectors.nbytes), DeviceBuffer(n * 4), DeviceBuffer((K + 1) * 8),
            DeviceBuffer(digests * 32), DeviceBuffer((K + 2) * 32)]
    try:
        bufs[0].upload(vectors)
        bufs[1].upload(centroids)
        check(lib.vdb_ann_index_build_dev(bufs[0].ptr, _p(ids), bufs[1].ptr, _sz(n), _sz(K), _sz(dim), bufs[2].ptr, bufs[3].ptr, bufs[4].ptr, bufs[5].ptr,
                                          bufs[6].ptr))
        return dict(grouped=bufs[2].download((n, dim, 4)), slots=bufs[3].download((n,), dtype=np.uint32), offsets=bufs[4].download((K + 1,), dtype=np.uint64),
                    forest=bufs[5].download((digests, 4)), segments=seg, roots=bufs[6].download((K + 2, 4)))
    finally:
        for b in bufs:
            b.free()


def wit_ann_probe(metric, query, centroids, members_list, cluster_roots, topk=1, P=48, L=13, selectors=False):
    """the circuit of one query over the p nearest clusters that returns the `topk` nearest candidates (vdb_wit_ann_probe) on query
    (dim, 4), centroids (K, dim, 4), members_list: the rows (n_r, dim, 4) of the p clusters the centroid rounds state, in round order, and
    the K cluster roots (K, 4): dict(stream, lookup, selectors, n_in, centroid_indicators (p, K, 4), candidate_indicators (topk, N, 4),
    results (topk, dim, 4), index_root (4,), public (topk dim + 1, 4))"""
    lib = _lib.init()
    query, centroids, cluster_roots = _fr(query), _fr(centroids), _fr(cluster_roots)
    members_list = [_fr(m) for m in members_list]
    K, dim, p, t = centroids.shape[0], centroids.shape[1], len(members_list), int(topk)
    assert query.shape == (dim, 4) and cluster_roots.shape == (K, 4) and all(m.ndim == 3 and m.shape[1:] == (dim, 4) for m in members_list)
    sizes = np.ascontiguousarray([m.shape[0] for m in members_list], dtype=np.uint64)
    cand = np.ascontiguousarray(np.concatenate(members_list)) if p else np.zeros((0, dim, 4), dtype=np.uint64)
    N = cand.shape[0]
    cells, lk, n_in = _u64(), _u64(), _u64()
    m = METRICS[metric]
    check(lib.vdb_wit_ann_probe_size(m, ctypes.c_uint32(P), ctypes.c_uint32(L), _sz(K), _sz(dim), _sz(p), _p(sizes), _sz(t), ctypes.byref(cells),
                                     ctypes.byref(lk), ctypes.byref(n_in)))
    stream = np.zeros((cells.value, 4), dtype=np.uint64)
    lookup = np.zeros((lk.value, 4), dtype=np.uint64)
    sel = np.zeros(cells.value, dtype=np.uint8) if selectors else None
    ind_c, ind_m, pub = np.zeros((p, K, 4), dtype=np.uint64), np.zeros((t, N, 4), dtype=np.uint64), np.zeros((t * dim + 1, 4), dtype=np.uint64)
    check(lib.vdb_wit_ann_probe(m, ctypes.c_uint32(P), ctypes.c_uint32(L), _p(query), _p(centroids), _p(cand), _p(cluster_roots), _sz(K), _sz(dim), _sz(p),
                                _p(sizes), _sz(t), _p(stream), _p(lookup), _p(sel) if selectors else None, _p(ind_c), _p(ind_m), _p(pub)))
    return dict(stream=stream, lookup=lookup, **_split_flags(sel), n_in=n_in.value, centroid_indicators=ind_c, candidate_indicators=ind_m,
                results=pub[:t * dim].reshape(t, dim, 4), index_root=pub[t * dim], public=pub)


def wit_ann_query(metric, query, centroids, members, cluster_roots, P=48, L=13, selectors=False):
    """the circuit of one query of the nearest cluster alone (vdb_wit_ann_query) on query (dim, 4), centroids (K, dim, 4), the members of
    the cluster searched (n_c, dim, 4) and the K cluster roots (K, 4): wit_ann_probe of the one cluster at topk = 1; dict(stream, lookup,
    selectors, n_in, centroid_indicator (K, 4), member_indicator (n_c, 4), result (dim, 4), index_root (4,), public (dim + 1, 4))"""
    out = wit_ann_probe(metric, query, centroids, [members], cluster_roots, 1, P, L, selectors)
    out["centroid_indicator"], out["member_indicator"] = out.pop("centroid_indicators")[0], out.pop("candidate_indicators")[0]
    out["result"] = out.pop("results")[0]
    return out


def _wit_ann_cluster(size, call, metric, centroids, members, roots, cluster, P, L, selectors, flag, per_member):
    """the buffers of a host-array audit of one cluster and its dict: `size` / `call` the library's two entry points, which take the metric
    (where the audit has one: `metric` not None), P and L ahead of what the audits share; `flag`: the key of the flag bytes, one per member
    or one per word"""
    centroids, members, roots = _fr(centroids), _fr(members), _fr(roots)
    K, dim, n_c = centroids.shape[0], centroids.shape[1], members.shape[0]
    assert members.shape[1] == dim and roots.shape == (K + 1, 4)
    cells, lk, n_in = _u64(), _u64(), _u64()
    ahead = ([] if metric is None else [METRICS[metric]]) + [ctypes.c_uint32(P), ctypes.c_uint32(L)]
    check(size(*ahead, _sz(K), _sz(n_c), _sz(dim), ctypes.byref(cells), ctypes.byref(lk), ctypes.byref(n_in)))
    stream = np.zeros((cells.value, 4), dtype=np.uint64)
    lookup = np.zeros((lk.value, 4), dtype=np.uint64)
    sel = np.zeros(cells.value, dtype=np.uint8) if selectors else None
    flags, pub = np.zeros(n_c if per_member else dim, dtype=np.uint8), np.zeros((2, 4), dtype=np.uint64)
    check(call(*ahead, _p(centroids), _p(members), _p(roots), _sz(K), _sz(cluster), _sz(n_c), _sz(dim), _p(stream), _p(lookup),
               _p(sel) if selectors else None, _p(flags), _p(pub)))
    return dict(stream=stream, lookup=lookup, **_split_flags(sel), n_in=n_in.value, **{flag: flags}, public=pub)


def wit_ann_audit(metric, centroids, members, roots, cluster, P=48, L=13, selectors=False):
    """the audit of one cluster's routing (vdb_wit_ann_audit) on centroids (K, dim, 4), the members of cluster `cluster` (n_c, dim, 4) and
    roots (K + 1, 4): [centroids' root | cluster roots]: dict(stream, lookup, selectors, flags, n_in, routed (n_c,) uint8: member i's own
    centroid attains the minimum, public (2, 4): [index_root | c])"""
    lib = _lib.init()
    return _wit_ann_cluster(lib.vdb_wit_ann_audit_size, lib.vdb_wit_ann_audit, metric, centroids, members, roots, cluster, P, L, selectors, "routed", True)


def wit_ann_mean(centroids, members, roots, cluster, P=48, L=13, selectors=False):
    """the mean audit of one cluster (vdb_wit_ann_mean) on centroids (K, dim, 4), the members of cluster `cluster` (n_c, dim, 4) and roots
    (K + 1, 4): [centroids' root | cluster roots]: dict(stream, lookup, selectors, flags, n_in, mean_ok (dim,) uint8: word j of centroid
    `cluster` is qdiv(sum of the members' words j, quantization(n_c)), public (2, 4): [index_root | c])"""
    lib = _lib.init()
    return _wit_ann_cluster(lib.vdb_wit_ann_mean_size, lib.vdb_wit_ann_mean, None, centroids, members, roots, cluster, P, L, selectors, "mean_ok", False)


def wit_ann_recentre(centroid_levels, members, roots, c, P=48, L=13, selectors=False):
    """the recentre of cluster `c` (vdb_wit_ann_recentre), the streams alone: `centroid_levels` the centroids' tree (2 lp_K, 4)
    (merkle_tree_build's array over the K centroids), the members of the cluster (n_c, dim, 4) and roots (K + 1, 4): [centroids' root |
    cluster roots]: dict(stream, lookup, selectors, flags, n_in, update_base, public (3, 4): [index_root_old | c | index_root_new],
    new_centroid (dim, 4): qdiv(sum of the members' words, quantization(n_c)), levels: the centroids' tree after the write)"""
    lib = _lib.init()
    members, roots = _fr(members), _fr(roots)
    n_c, dim, K = members.shape[0], members.shape[1], roots.shape[0] - 1
    levels = np.array(centroid_levels, dtype=np.uint64, copy=True)
    assert roots.shape == (K + 1, 4) and levels.shape == (2 * merkle_levels(max(K, 1))[0], 4)
    cells, lk, n_in, ub = _u64(), _u64(), _u64(), _u64()
    check(lib.vdb_wit_ann_recentre_size(ctypes.c_uint32(P), ctypes.c_uint32(L), _sz(K), _sz(n_c), _sz(dim), ctypes.byref(cells), ctypes.byref(lk),
                                        ctypes.byref(n_in), ctypes.byref(ub)))
    stream, lookup = np.zeros((cells.value, 4), dtype=np.uint64), np.zeros((lk.value, 4), dtype=np.uint64)
    sel = np.zeros(cells.value, dtype=np.uint8) if selectors else None
    new, pub = np.zeros((dim, 4), dtype=np.uint64), np.zeros((3, 4), dtype=np.uint64)
    check(lib.vdb_wit_ann_recentre(ctypes.c_uint32(P), ctypes.c_uint32(L), _p(levels), _p(members), _p(roots), _sz(K), _sz(c), _sz(n_c), _sz(dim), _p(stream),
                                   _p(lookup), _p(sel) if selectors else None, _p(new), _p(pub)))
    return dict(stream=stream, lookup=lookup, **_split_flags(sel), n_in=n_in.value, update_base=ub.value, public=pub, new_centroid=new, levels=levels)


def wit_ann_cover(db_leaves, cluster_leaves, sizes, centroids_root, selectors=False):
    """the cover of the database by the index (vdb_wit_ann_cover), the streams alone: `db_leaves` (n, 4) the database's leaf digests in
    slot order, `cluster_leaves` (n, 4) the clusters' leaf digests in grouped order, `sizes` the K cluster sizes (they sum to n) and the
    centroids' root (4,).  The K + 1 trees are hashed over what is given: dict(stream, selectors, flags, n_in, public (2, 4):
    [database_root | index_root])"""
    lib = _lib.init()
    a, b, croot = _fr(db_leaves), _fr(cluster_leaves), _fr(centroids_root).reshape(4)
    sizes = np.ascontiguousarray(sizes, dtype=np.uint64)
    K, n = sizes.size, a.shape[0]
    assert a.shape == (n, 4) and b.shape == (n, 4)
    cells, n_in = _u64(), _u64()
    check(lib.vdb_wit_ann_cover_size(_p(sizes), _sz(K), _sz(n), ctypes.byref(cells), ctypes.byref(n_in)))
    stream = np.zeros((cells.value, 4), dtype=np.uint64)
    sel = np.zeros(cells.value, dtype=np.uint8) if selectors else None
    pub = np.zeros((2, 4), dtype=np.uint64)
    check(lib.vdb_wit_ann_cover(_p(a), _p(b), _p(croot), _p(sizes), _sz(K), _sz(n), _p(stream), _p(sel) if selectors else None, _p(pub)))
    return dict(stream=stream, **_split_flags(sel), n_in=n_in.value, public=pub)


def ann_index_db_tree(forest, sizes, slots):
    """the database tree of an index (vdb_ann_index_db_tree_dev) from its downloaded `forest` (digests, 4), the K cluster `sizes` and the
    `slots` (n,) of ann_index_build: (2 lp, 4), bit for bit merkle_tree_build over the rows in slot order; VdbError where `slots` is no
    permutation of 0 .. n - 1"""
    lib = _lib.init()
    forest, sizes = _fr(forest), np.ascontiguousarray(sizes, dtype=np.uint64)
    slots = np.ascontiguousarray(slots, dtype=np.uint32)
    K, n = sizes.size, slots.size
    lp, _ = merkle_levels(max(n, 1))
    assert forest.shape[0] >= sum(2 * merkle_levels(int(x))[0] for x in sizes), "the forest does not hold the K cluster trees"
    d_f, d_s, d_lv = DeviceBuffer(max(forest.nbytes, 32)), DeviceBuffer(max(slots.nbytes, 32)), DeviceBuffer(2 * lp * 32)
    try:
        d_f.upload(forest)
        d_s.upload(slots)
        check(lib.vdb_ann_index_db_tree_dev(d_f.ptr, _p(sizes), d_s.ptr, _sz(K), _sz(n), d_lv.ptr))
        return d_lv.download((2 * lp, 4))
    finally:
        for d in (d_f, d_s, d_lv):
            d.free()


def ann_cluster_means(grouped, offsets, P=48, L=13):
    """the means of all K clusters of grouped rows (n, dim, 4), cluster k the rows [offsets[k], offsets[k + 1]) (vdb_ann_cluster_means: values
    only): (K, dim, 4), means[k][j] = qdiv(sum of the cluster's words j, quantization(n_k)) bit for bit as vdb_wit_ann_mean constrains it"""
    lib = _lib.init()
    grouped = _fr(grouped)
    offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
    assert grouped.ndim == 3 and offsets.ndim == 1 and offsets.size >= 1
    n, dim, K = grouped.shape[0], grouped.shape[1], offsets.size - 1
    means = np.zeros((K, dim, 4), dtype=np.uint64)
    check(lib.vdb_ann_cluster_means(ctypes.c_uint32(P), ctypes.c_uint32(L), _p(grouped), _p(offsets), _sz(n), _sz(K), _sz(dim), _p(means)))
    return means


def _wit_ann_batch(levels, cells, n_pub, selectors, call, **sizes):
    """the buffers of a host-array call against the index root and its dict: call(levels, stream, selectors or None, public) -> its code"""
    levels = np.array(levels, dtype=np.uint64, copy=True)
    stream, pub = np.zeros((cells, 4), dtype=np.uint64), np.zeros((n_pub, 4), dtype=np.uint64)
    sel = np.zeros(cells, dtype=np.uint8) if selectors else None
    check(call(_p(levels), _p(stream), _p(sel) if selectors else None, _p(pub)))
    return dict(stream=stream, **_split_flags(sel), **sizes, public=pub, levels=levels)


def wit_ann_update(levels, roots, cluster, n_c, new_vectors, indices, grow=0, selectors=False):
    """m writes into cluster `cluster` of a committed index (vdb_wit_ann_update), the streams alone: `levels` cluster c's tree over its
    n_c members (merkle_tree_build's array, after merkle_tree_grow when grow > 0), `roots` (K + 1, 4): [centroids' root | cluster roots],
    new_vectors (m, dim, 4), indices (m,): slots of the cluster, each below the fill at its turn or equal to it (an append).
    dict(stream, selectors, flags, input_cells, update_base, public (3 m + 3, 4): [index_root_old | c | idx, old leaf, new leaf per write |
    index_root_new], levels: the cluster's tree after the batch)"""
    lib = _lib.init()
    new_vectors, roots = _fr(new_vectors), _fr(roots)
    idx = np.ascontiguousarray(indices, dtype=np.uint64)
    m, dim, K = idx.shape[0], new_vectors.shape[1], roots.shape[0] - 1
    assert idx.shape == (m,) and new_vectors.shape[0] == m and np.shape(levels) == (2 * (merkle_levels(n_c)[0] << grow), 4)
    cells, n_in, ub = _u64(), _u64(), _u64()
    check(lib.vdb_wit_ann_update_size(_sz(K), _sz(n_c), _sz(dim), _sz(m), int(grow), ctypes.byref(cells), ctypes.byref(n_in), ctypes.byref(ub)))
    call = lambda lv, st, sl, pb: lib.vdb_wit_ann_update(lv, _p(roots), _sz(K), _sz(cluster), _sz(n_c), _sz(dim), int(grow), _p(new_vectors), _p(idx),
                                                         _sz(m), st, sl, pb)
    return _wit_ann_batch(levels, cells.value, 3 * m + 3, selectors, call, input_cells=n_in.value, update_base=ub.value)


def ann_index_apply_layout(sizes, cluster, grow, indices):
    """(appends, digests of the forest after the batch, its K + 2 segment offsets) of vdb_ann_index_apply_dev (vdb_ann_index_apply_size;
    VdbError on a write above the fill, or a `grow` that is not the smallest that fits the appends)"""
    lib = _lib.init()
    sizes, idx = np.ascontiguousarray(sizes, dtype=np.uint64), np.ascontiguousarray(indices, dtype=np.uint64)
    K = sizes.shape[0]
    appends, digests, seg = _u64(), _u64(), np.zeros(K + 2, dtype=np.uint64)
    check(lib.vdb_ann_index_apply_size(_p(sizes), _sz(K), _sz(cluster), int(grow), _p(idx), _sz(idx.shape[0]), ctypes.byref(appends), ctypes.byref(digests),
                                       _p(seg)))
    return appends.value, digests.value, seg


def ann_index_apply(index, cluster, grow, updated_levels, new_vectors, indices, db_slots):
    """the index after a batch of writes into one cluster (vdb_ann_index_apply_dev), host arrays in and out: `index` an ann_index_build
    dict, updated_levels the cluster's tree the witness call left, db_slots one database slot per append -> a dict of the same form"""
    lib = _lib.init()
    new_vectors, updated = _fr(new_vectors), _fr(updated_levels)
    idx = np.ascontiguousarray(indices, dtype=np.uint64)
    slots_new = np.ascontiguousarray(db_slots, dtype=np.uint32)
    sizes = np.diff(np.asarray(index["offsets"], dtype=np.uint64)).astype(np.uint64)
    K, dim, n = sizes.shape[0], new_vectors.shape[1], index["grouped"].shape[0]
    appends, digests, seg = ann_index_apply_layout(sizes, cluster, grow, idx)
    assert slots_new.shape == (appends,) and idx.shape == (new_vectors.shape[0],)
    n2 = n + appends
    src = [index["grouped"], np.ascontiguousarray(index["slots"], dtype=np.uint32), index["forest"], index["roots"], updated, new_vectors]
    ins = [DeviceBuffer(max(a.nbytes, 32)) for a in src]
    outs = [DeviceBuffer(max(b, 32)) for b in (n2 * dim * 32, n2 * 4, (K + 1) * 8, digests * 32, (K + 2) * 32)]
    try:
        for b, a in zip(ins, src):
            b.upload(np.ascontiguousarray(a))
        check(lib.vdb_ann_index_apply_dev(ins[0].ptr, ins[1].ptr, ins[2].ptr, ins[3].ptr, _p(sizes), _sz(K), _sz(dim), _sz(cluster), int(grow), ins[4].ptr,
                                          ins[5].ptr, _p(idx), _p(slots_new) if appends else None, _sz(idx.shape[0]), *[o.ptr for o in outs]))
        return dict(grouped=outs[0].download((n2, dim, 4)), slots=outs[1].download((n2,), dtype=np.uint32), offsets=outs[2].download((K + 1,), dtype=np.uint64),
                    forest=outs[3].download((digests, 4)), segments=seg, roots=outs[4].download((K + 2, 4)))
    finally:
        for b in ins + outs:
            b.free()


def ann_write_db_indices(cluster_slots, indices, n_db):
    """the database slot of every write of a batch into one cluster (vdb_ann_write_db_indices: values only, no device call): a replacement
    takes the slot `cluster_slots` records for its member, an append n_db + the appends so far, a write to a member the batch appended
    that member's -> (db_idx (m,) uint64, appends); VdbError on a write above the fill or a recorded slot outside the database"""
    lib = _lib.load()
    slots, idx = np.ascontiguousarray(cluster_slots, dtype=np.uint64), np.ascontiguousarray(indices, dtype=np.uint64)
    out, appends = np.zeros(max(idx.shape[0], 1), dtype=np.uint64), _u64()
    check(lib.vdb_ann_write_db_indices(_p(slots), _sz(slots.shape[0]), _sz(n_db), _p(idx), _sz(idx.shape[0]), _p(out), ctypes.byref(appends), None))
    return out[:idx.shape[0]], appends.value


def wit_ann_write(levels_c, levels_db, roots, cluster, n_c, n_db, new_vectors, indices, db_indices, grow_c=None, grow_db=None, selectors=False):
    """a linked write (vdb_wit_ann_write), the streams alone: m writes into cluster `cluster` of a committed index and the same m leaf
    changes in the database tree.  levels_c: cluster c's tree over its n_c members, levels_db: the database tree over its n_db rows, each
    AFTER merkle_tree_grow when its grow > 0 (None: the smallest number that fits, which the array's shape must match); `roots` (K + 1, 4):
    [centroids' root | cluster roots]; new_vectors (m, dim, 4); indices (m,): slots of the cluster as wit_ann_update; db_indices (m,): the
    database slots (ann_write_db_indices).  dict(stream, selectors, flags, input_cells, update_base, update_db_base, grow_c, grow_db,
    public (4 m + 5, 4): [database_root_old | index_root_old | c | idx, db_idx, old leaf, new leaf per write | database_root_new |
    index_root_new], levels_c, levels_db: the two trees after the batch)"""
    lib = _lib.init()
    new_vectors, roots = _fr(new_vectors), _fr(roots)
    idx, dbi = np.ascontiguousarray(indices, dtype=np.uint64), np.ascontiguousarray(db_indices, dtype=np.uint64)
    m, dim, K = idx.shape[0], new_vectors.shape[1], roots.shape[0] - 1
    fill = n_c
    for s in idx.tolist():
        fill += s == fill
    cells, n_in, ub, udb, gc, gdb = _u64(), _u64(), _u64(), _u64(), ctypes.c_uint(), ctypes.c_uint()
    check(lib.vdb_wit_ann_write_size(_sz(K), _sz(n_c), _sz(n_db), _sz(dim), _sz(m), _sz(fill - n_c), ctypes.byref(cells), ctypes.byref(n_in), ctypes.byref(ub),
                                     ctypes.byref(udb), ctypes.byref(gc), ctypes.byref(gdb)))
    grow_c, grow_db = gc.value if grow_c is None else int(grow_c), gdb.value if grow_db is None else int(grow_db)
    lc, ld = np.array(levels_c, dtype=np.uint64, copy=True), np.array(levels_db, dtype=np.uint64, copy=True)
    assert idx.shape == (m,) and dbi.shape == (m,) and new_vectors.shape[0] == m
    assert lc.shape == (2 * (merkle_levels(n_c)[0] << grow_c), 4) and ld.shape == (2 * (merkle_levels(n_db)[0] << grow_db), 4)
    stream, pub = np.zeros((cells.value, 4), dtype=np.uint64), np.zeros((4 * m + 5, 4), dtype=np.uint64)
    sel = np.zeros(cells.value, dtype=np.uint8) if selectors else None
    check(lib.vdb_wit_ann_write(_p(lc), _p(ld), _p(roots), _sz(K), _sz(cluster), _sz(n_c), _sz(n_db), _sz(dim), grow_c, grow_db, _p(new_vectors), _p(idx),
                                _p(dbi), _sz(m), _p(stream), _p(sel) if selectors else None, _p(pub)))
    return dict(stream=stream, **_split_flags(sel), input_cells=n_in.value, update_base=ub.value, update_db_base=udb.value, grow_c=grow_c, grow_db=grow_db,
                public=pub, levels_c=lc, levels_db=ld)


def ann_index_write_layout(sizes, cluster, indices):
    """(appends, g_c, g_db, digests of the forest after the batch, its K + 2 segment offsets, digests of the database tree after it) of
    vdb_ann_index_write_dev (vdb_ann_index_write_size; VdbError on a write above the fill)"""
    lib = _lib.init()
    sizes, idx = np.ascontiguousarray(sizes, dtype=np.uint64), np.ascontiguousarray(indices, dtype=np.uint64)
    K = sizes.shape[0]
    appends, gc, gdb, digests, seg, dbd = _u64(), ctypes.c_uint(), ctypes.c_uint(), _u64(), np.zeros(K + 2, dtype=np.uint64), _u64()
    check(lib.vdb_ann_index_write_size(_p(sizes), _sz(K), _sz(cluster), _p(idx), _sz(idx.shape[0]), ctypes.byref(appends), ctypes.byref(gc), ctypes.byref(gdb),
                                       ctypes.byref(digests), _p(seg), ctypes.byref(dbd)))
    return appends.value, gc.value, gdb.value, digests.value, seg, dbd.value


def ann_index_write(index, cluster, updated_levels, updated_db_levels, new_vectors, indices, grow_c=None, grow_db=None):
    """both resident objects after a linked write (vdb_ann_index_write_dev), host arrays in and out: `index` an ann_index_build dict,
    updated_levels / updated_db_levels the two trees the witness call left -> a dict of the same form with db_tree: the database tree of
    the new index; the appends take the database slots n, n + 1, ..."""
    lib = _lib.init()
    new_vectors, uc, ud = _fr(new_vectors), _fr(updated_levels), _fr(updated_db_levels)
    idx = np.ascontiguousarray(indices, dtype=np.uint64)
    sizes = np.diff(np.asarray(index["offsets"], dtype=np.uint64)).astype(np.uint64)
    K, dim, n = sizes.shape[0], new_vectors.shape[1], index["grouped"].shape[0]
    appends, gc, gdb, digests, seg, dbd = ann_index_write_layout(sizes, cluster, idx)
    grow_c, grow_db = gc if grow_c is None else int(grow_c), gdb if grow_db is None else int(grow_db)
    assert idx.shape == (new_vectors.shape[0],)
    n2 = n + appends
    src = [index["grouped"], np.ascontiguousarray(index["slots"], dtype=np.uint32), index["forest"], index["roots"], uc, ud, new_vectors]
    ins = [DeviceBuffer(max(a.nbytes, 32)) for a in src]
    outs = [DeviceBuffer(max(b, 32)) for b in (n2 * dim * 32, n2 * 4, (K + 1) * 8, digests * 32, (K + 2) * 32, ud.nbytes)]
    try:
        for b, a in zip(ins, src):
            b.upload(np.ascontiguousarray(a))
        check(lib.vdb_ann_index_write_dev(ins[0].ptr, ins[1].ptr, ins[2].ptr, ins[3].ptr, _p(sizes), _sz(K), _sz(dim), _sz(cluster), grow_c, grow_db,
                                          ins[4].ptr, ins[5].ptr, ins[6].ptr, _p(idx), _sz(idx.shape[0]), *[o.ptr for o in outs]))
        return dict(grouped=outs[0].download((n2, dim, 4)), slots=outs[1].download((n2,), dtype=np.uint32), offsets=outs[2].download((K + 1,), dtype=np.uint64),
                    forest=outs[3].download((digests, 4)), segments=seg, roots=outs[4].download((K + 2, 4)), db_tree=outs[5].download((ud.shape[0], 4)))
    finally:
        for b in ins + outs:
            b.free()


def wit_ann_delete(levels, roots, cluster, n_c, dim, slots, selectors=False):
    """m deletes from cluster `cluster` of a committed index (vdb_wit_ann_delete), the streams alone: `levels` cluster c's tree over its
    n_c members (merkle_tree_build's array), `roots` (K + 1, 4): [centroids' root | cluster roots], slots (m,): slot j is below the fill
    at its turn (n_c - j); the last member moves into it.  dict(stream, selectors, flags, input_cells, update_base, shrink_base, shrink,
    public (4 m + 3, 4): [index_root_old | c | slot, removed leaf, last, moved leaf per delete | index_root_new], levels: the cluster's
    tree after the batch, at its old size)"""
    lib = _lib.init()
    roots = _fr(roots)
    idx = np.ascontiguousarray(slots, dtype=np.uint64)
    m, K = idx.shape[0], roots.shape[0] - 1
    assert idx.shape == (m,) and np.shape(levels) == (2 * merkle_levels(n_c)[0], 4)
    cells, n_in, ub, sb, s = _u64(), _u64(), _u64(), _u64(), ctypes.c_uint()
    check(lib.vdb_wit_ann_delete_size(_sz(K), _sz(n_c), _sz(dim), _sz(m), ctypes.byref(cells), ctypes.byref(n_in), ctypes.byref(ub), ctypes.byref(sb),
                                      ctypes.byref(s)))
    call = lambda lv, st, sl, pb: lib.vdb_wit_ann_delete(lv, _p(roots), _sz(K), _sz(cluster), _sz(n_c), _sz(dim), _p(idx), _sz(m), st, sl, pb)
    return _wit_ann_batch(levels, cells.value, 4 * m + 3, selectors, call, input_cells=n_in.value, update_base=ub.value, shrink_base=sb.value, shrink=s.value)


def ann_index_remove_layout(sizes, cluster, slots):
    """(halvings of the cluster's tree, digests of the forest after the batch, its K + 2 segment offsets) of vdb_ann_index_remove_dev
    (vdb_ann_index_remove_size; VdbError on a slot at or above the fill at its turn, or a batch that would empty the cluster)"""
    lib = _lib.init()
    sizes, idx = np.ascontiguousarray(sizes, dtype=np.uint64), np.ascontiguousarray(slots, dtype=np.uint64)
    K = sizes.shape[0]
    s, digests, seg = ctypes.c_uint(), _u64(), np.zeros(K + 2, dtype=np.uint64)
    check(lib.vdb_ann_index_remove_size(_p(sizes), _sz(K), _sz(cluster), _p(idx), _sz(idx.shape[0]), ctypes.byref(s), ctypes.byref(digests), _p(seg)))
    return s.value, digests.value, seg


def ann_index_remove(index, cluster, updated_levels, slots):
    """the index after a batch of deletes from one cluster (vdb_ann_index_remove_dev), host arrays in and out: `index` an ann_index_build
    dict, updated_levels the cluster's tree the witness call left (at its old size) -> a dict of the same form over the compacted
    database: its slots are 0 .. n - m - 1"""
    lib = _lib.init()
    updated = _fr(updated_levels)
    idx = np.ascontiguousarray(slots, dtype=np.uint64)
    sizes = np.diff(np.asarray(index["offsets"], dtype=np.uint64)).astype(np.uint64)
    K, dim, n, m = sizes.shape[0], index["grouped"].shape[1], index["grouped"].shape[0], idx.shape[0]
    _, digests, seg = ann_index_remove_layout(sizes, cluster, idx)
    n2 = n - m
    src = [index["grouped"], index["forest"], index["roots"], updated]
    ins = [DeviceBuffer(max(a.nbytes, 32)) for a in src]
    outs = [DeviceBuffer(max(b, 32)) for b in (n2 * dim * 32, n2 * 4, (K + 1) * 8, digests * 32, (K + 2) * 32)]
    try:
        for b, a in zip(ins, src):
            b.upload(np.ascontiguousarray(a))
        check(lib.vdb_ann_index_remove_dev(ins[0].ptr, ins[1].ptr, ins[2].ptr, _p(sizes), _sz(K), _sz(dim), _sz(cluster), ins[3].ptr, _p(idx), _sz(m),
                                           *[o.ptr for o in outs]))
        return dict(grouped=outs[0].download((n2, dim, 4)), slots=outs[1].download((n2,), dtype=np.uint32), offsets=outs[2].download((K + 1,), dtype=np.uint64),
                    forest=outs[3].download((digests, 4)), segments=seg, roots=outs[4].download((K + 2, 4)))
    finally:
        for b in ins + outs:
            b.free()


def wit_ann_move(levels_src, levels_dst, roots, src, dst, n_a, n_b, slots, grow=None, selectors=False):
    """m moves from cluster `src` to cluster `dst` of a committed index (vdb_wit_ann_move), the streams alone: levels_src a's tree over
    its n_a members, levels_dst b's tree over its n_b members AFTER merkle_tree_grow when grow > 0 (grow None: the smallest number that
    fits, which the shape of levels_dst must match), `roots` (K + 1, 4): [centroids' root | cluster roots], slots (m,): slot j of a is
    below a's fill at its turn (n_a - j).  dict(stream, selectors, flags, input_cells, delete_base, shrink_base, append_base, shrink, grow,
    public (6 m + 4, 4): [index_root_old | a | b | slot, leaf, last, moved leaf, dest, dest old leaf per move | index_root_new],
    levels_src, levels_dst: the two trees after the batch, a's at its old size)"""
    lib = _lib.init()
    roots = _fr(roots)
    idx = np.ascontiguousarray(slots, dtype=np.uint64)
    m, K = idx.shape[0], roots.shape[0] - 1
    cells, n_in, db, sb, ab, s, g = _u64(), _u64(), _u64(), _u64(), _u64(), ctypes.c_uint(), ctypes.c_uint()
    check(lib.vdb_wit_ann_move_size(_sz(K), _sz(n_a), _sz(n_b), _sz(m), ctypes.byref(cells), ctypes.byref(n_in), ctypes.byref(db), ctypes.byref(sb),
                                    ctypes.byref(ab), ctypes.byref(s), ctypes.byref(g)))
    grow = g.value if grow is None else int(grow)
    la, lb = np.array(levels_src, dtype=np.uint64, copy=True), np.array(levels_dst, dtype=np.uint64, copy=True)
    assert idx.shape == (m,) and la.shape == (2 * merkle_levels(n_a)[0], 4) and lb.shape == (2 * (merkle_levels(n_b)[0] << grow), 4)
    stream, pub = np.zeros((cells.value, 4), dtype=np.uint64), np.zeros((6 * m + 4, 4), dtype=np.uint64)
    sel = np.zeros(cells.value, dtype=np.uint8) if selectors else None
    check(lib.vdb_wit_ann_move(_p(la), _p(lb), _p(roots), _sz(K), _sz(src), _sz(dst), _sz(n_a), _sz(n_b), grow, _p(idx), _sz(m), _p(stream),
                               _p(sel) if selectors else None, _p(pub)))
    return dict(stream=stream, **_split_flags(sel), input_cells=n_in.value, delete_base=db.value, shrink_base=sb.value, append_base=ab.value,
                shrink=s.value, grow=g.value, public=pub, levels_src=la, levels_dst=lb)


def ann_index_move_layout(sizes, src, dst, slots):
    """(halvings of a's tree, doublings of b's, digests of the forest after the batch, its K + 2 segment offsets) of
    vdb_ann_index_move_dev (vdb_ann_index_move_size; VdbError on src == dst, a slot at or above a's fill at its turn, or a batch that
    would empty a)"""
    lib = _lib.init()
    sizes, idx = np.ascontiguousarray(sizes, dtype=np.uint64), np.ascontiguousarray(slots, dtype=np.uint64)
    K = sizes.shape[0]
    s, g, digests, seg = ctypes.c_uint(), ctypes.c_uint(), _u64(), np.zeros(K + 2, dtype=np.uint64)
    check(lib.vdb_ann_index_move_size(_p(sizes), _sz(K), _sz(src), _sz(dst), _p(idx), _sz(idx.shape[0]), ctypes.byref(s), ctypes.byref(g),
                                      ctypes.byref(digests), _p(seg)))
    return s.value, g.value, digests.value, seg


def ann_index_move(index, src, dst, updated_src, updated_dst, slots, grow=None):
    """the index after a batch of moves from cluster src to cluster dst (vdb_ann_index_move_dev), host arrays in and out: `index` an
    ann_index_build dict, updated_src / updated_dst the two trees the witness call left -> a dict of the same form over the SAME
    database: the slots entries travel with their rows"""
    lib = _lib.init()
    ua, ub = _fr(updated_src), _fr(updated_dst)
    idx = np.ascontiguousarray(slots, dtype=np.uint64)
    sizes = np.diff(np.asarray(index["offsets"], dtype=np.uint64)).astype(np.uint64)
    K, dim, n, m = sizes.shape[0], index["grouped"].shape[1], index["grouped"].shape[0], idx.shape[0]
    _, g, digests, seg = ann_index_move_layout(sizes, src, dst, idx)
    grow = g if grow is None else int(grow)
    src_arrays = [index["grouped"], np.ascontiguousarray(index["slots"], dtype=np.uint32), index["forest"], index["roots"], ua, ub]
    ins = [DeviceBuffer(max(a.nbytes, 32)) for a in src_arrays]
    outs = [DeviceBuffer(max(b, 32)) for b in (n * dim * 32, n * 4, (K + 1) * 8, digests * 32, (K + 2) * 32)]
    try:
        for b, a in zip(ins, src_arrays):
            b.upload(np.ascontiguousarray(a))
        check(lib.vdb_ann_index_move_dev(ins[0].ptr, ins[1].ptr, ins[2].ptr, ins[3].ptr, _p(sizes), _sz(K), _sz(dim), _sz(src), _sz(dst), grow, ins[4].ptr,
                                         ins[5].ptr, _p(idx), _sz(m), *[o.ptr for o in outs]))
        return dict(grouped=outs[0].download((n, dim, 4)), slots=outs[1].download((n,), dtype=np.uint32), offsets=outs[2].download((K + 1,), dtype=np.uint64),
                    forest=outs[3].download((digests, 4)), segments=seg, roots=outs[4].download((K + 2, 4)))
    finally:
        for b in ins + outs:
            b.free()


def wit_merkle_open(levels, n, indices, vectors=None, selectors=False):
    """m openings (vdb_wit_merkle_open) of the tree `levels` (merkle_tree_build's array over n vectors, or what a batch of updates left):
    slot indices[j] is read.  `vectors` (m, dim, 4): the vectors read (vector mode); None: leaf mode, any slot of the padded tree.
    dict(stream, selectors, input_cells, public: [root | idx, leaf per read | in vector mode the vectors word by word])"""
    lib = _lib.init()
    levels = np.ascontiguousarray(levels, dtype=np.uint64)
    idx = np.ascontiguousarray(indices, dtype=np.uint64)
    m = idx.shape[0]
    assert idx.shape == (m,) and levels.shape == (2 * merkle_levels(n)[0], 4)
    dim = 1                                                   # leaf mode reads no vector: the word count only has to be a valid one
    if vectors is not None:
        vectors = _fr(vectors)
        assert vectors.shape[0] == m
        dim = vectors.shape[1]
    cells, n_in = _u64(), _u64()
    check(lib.vdb_wit_merkle_open_size(_sz(n), _sz(dim), _sz(m), int(vectors is not None), ctypes.byref(cells), ctypes.byref(n_in)))
    stream = np.zeros((cells.value, 4), dtype=np.uint64)
    sel = np.zeros(cells.value, dtype=np.uint8) if selectors else None
    pub = np.zeros((1 + 2 * m + (m * dim if vectors is not None else 0), 4), dtype=np.uint64)
    check(lib.vdb_wit_merkle_open(_p(levels), _sz(n), _sz(dim), _p(vectors) if vectors is not None else None, _p(idx), _sz(m), _p(stream),
                                  _p(sel) if selectors else None, _p(pub)))
    return dict(stream=stream, **_split_flags(sel), input_cells=n_in.value, public=pub)


def layout_plan(selectors, k, minimum_rows=9):
    lib = _lib.init()
    selectors = np.ascontiguousarray(selectors, dtype=np.uint8)
    nbp = _u64()
    check(lib.vdb_layout_plan(_p(selectors), ctypes.c_uint64(selectors.size), ctypes.c_uint32(k), ctypes.c_uint32(minimum_rows), None, ctypes.c_uint64(0),
                              ctypes.byref(nbp)))
    bp = np.zeros(max(nbp.value, 1), dtype=np.uint64)
    check(lib.vdb_layout_plan(_p(selectors), ctypes.c_uint64(selectors.size), ctypes.c_uint32(k), ctypes.c_uint32(minimum_rows), _p(bp),
                              ctypes.c_uint64(bp.size), ctypes.byref(nbp)))
    return bp[:nbp.value]


def layout_columns(stream, break_points, k, lookup=None, minimum_rows=9):
    lib = _lib.init()
    stream = _fr(stream)
    bp = np.ascontiguousarray(break_points, dtype=np.uint64)
    cols = np.zeros((bp.size + 1, 1 << k, 4), dtype=np.uint64)
    lcols = None
    n_lc = 0
    if lookup is not None and len(lookup):
        lookup = _fr(lookup)
        max_rows = (1 << k) - minimum_rows
        n_lc = (lookup.shape[0] + max_rows - 1) // max_rows
        lcols = np.zeros((n_lc, 1 << k, 4), dtype=np.uint64)
    check(lib.vdb_layout_columns(_p(stream), ctypes.c_uint64(stream.shape[0]), _p(bp), ctypes.c_uint64(bp.size), _p(lookup) if lcols is not None else None,
                                 ctypes.c_uint64(lookup.shape[0] if lcols is not None else 0), ctypes.c_uint32(k), ctypes.c_uint32(minimum_rows), _p(cols),
                                 _p(lcols) if lcols is not None else None, ctypes.c_uint64(n_lc)))
    return cols, lcols


# ---------------------------------------------------------------- Poseidon
def poseidon_hash_many(msgs):
    L = _lib.init()
    msgs = _fr(msgs)
    n, ln = msgs.shape[0], msgs.shape[1]
    o = np.zeros((n, 4), dtype=np.uint64)
    check(L.vdb_poseidon_hash_many(_p(msgs), _sz(n), _sz(ln), _p(o)))
    return o


def poseidon_merkle_root(vectors):
    L = _lib.init()
    vectors = _fr(vectors)
    o = np.zeros(4, dtype=np.uint64)
    check(L.vdb_poseidon_merkle_root(_p(vectors), _sz(vectors.shape[0]), _sz(vectors.shape[1]), _p(o)))
    return o


def poseidon_permute(states):
    L = _lib.init()
    s = np.array(states, dtype=np.uint64, copy=True)
    check(L.vdb_poseidon_permute(_p(s), _sz(s.size // 12)))
    return s


def random_scalars_dev(dst_ptr, n, seed=None):
    """n uniformly random field elements written to device memory at dst_ptr: 64 bytes of entropy each, reduced mod r on
    the device (vdb_fr_from_wide_dev = halo2curves Fr::random).  seed=None draws from the operating system (os.urandom), as
    halo2's prover does for its blinding scalars; an integer seed gives a reproducible stream (tests only)."""
    import os
    lib = _lib.init()
    raw = os.urandom(64 * n) if seed is None else np.random.default_rng(seed).bytes(64 * n)
    wide = DeviceBuffer(max(64 * n, 64))
    try:
        wide.upload(np.frombuffer(raw, dtype=np.uint8))
        check(lib.vdb_fr_from_wide_dev(wide.ptr, _sz(n), dst_ptr))
        sync()        # `wide` is freed on return
    finally:
        wide.free()


class MockReport(ctypes.Structure):
    """vdb_mock_report (include/vdb.h)"""
    _fields_ = [(n, ctypes.c_uint64) for n in ("gate_rows_violated", "first_gate_row", "lookup_cells_out_of_table", "first_lookup_cell",
                                               "copies_unequal", "first_copy", "lookup_copies_unequal", "first_lookup_copy",
                                               "constants_changed", "first_constant", "instances_unequal", "first_instance")]

    def violations(self):
        return int(self.gate_rows_violated + self.lookup_cells_out_of_table + self.copies_unequal + self.lookup_copies_unequal + self.constants_changed
                   + self.instances_unequal)

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


def mock_check_dev(stream_ptr, n_cells, flags_ptr, lookup_ptr, n_lookup, lookup_bits, copy_of_ptr=None, lookup_src_ptr=None, const_stream_ptr=None,
                   const_idx_ptr=None, const_table_ptr=None, n_consts=0):
    """MockProver-style check of a device-resident witness (vdb_mock_check_dev): every gate row, lookup cell, copy and constant"""
    rep = MockReport()
    check(_lib.init().vdb_mock_check_dev(stream_ptr, ctypes.c_uint64(n_cells), flags_ptr, lookup_ptr, ctypes.c_uint64(n_lookup), ctypes.c_uint32(lookup_bits),
                                         copy_of_ptr, lookup_src_ptr, const_stream_ptr, const_idx_ptr, const_table_ptr, ctypes.c_uint64(n_consts),
                                         ctypes.byref(rep)))
    return rep


def mock_check_instances_dev(rep, stream_ptr, n_cells, cells_ptr, values_ptr, n_instances):
    """the `instances` argument of MockProver::run on a device-resident witness (vdb_mock_check_instances_dev): stream cell cells[i]
    must hold values[i]; fills rep.instances_unequal / first_instance"""
    check(_lib.init().vdb_mock_check_instances_dev(stream_ptr, ctypes.c_uint64(n_cells), cells_ptr, values_ptr, ctypes.c_uint64(n_instances), ctypes.byref(rep)))
    return rep


def mock_check(stream, flags, lookup, lookup_bits, copy_of=None, lookup_src=None, const_stream=None):
    """the same on host arrays (uploaded): stream (n, 4), flags (n,) uint8, lookup (m, 4); copy maps as int64 arrays"""
    stream, lookup = _fr(stream), _fr(lookup) if lookup is not None and len(lookup) else np.zeros((0, 4), dtype=np.uint64)
    arrays = [stream, np.ascontiguousarray(flags, dtype=np.uint8), lookup]
    opt = [None if a is None else np.ascontiguousarray(a, dtype=np.int64) for a in (copy_of, lookup_src)] + [None if const_stream is None else _fr(const_stream)]
    bufs = [DeviceBuffer(max(a.nbytes, 32)) for a in arrays] + [None if a is None else DeviceBuffer(max(a.nbytes, 32)) for a in opt]
    try:
        for b, a in zip(bufs, arrays + opt):
            if b is not None and a.nbytes:
                b.upload(a)
        return mock_check_dev(bufs[0].ptr, stream.shape[0], bufs[1].ptr, bufs[2].ptr, lookup.shape[0], lookup_bits,
                              *(None if b is None else b.ptr for b in bufs[3:]))
    finally:
        for b in bufs:
            if b is not None:
                b.free()


# ---------------------------------------------------------------- device buffers
def extended_to_coeff(ext_cols, k, ext_k=2):
    """inverse of coeff_to_extended; ext_cols: (n_cols, 2^(k+ext_k), 4) on the host"""
    lib = _lib.init()
    e = _fr(ext_cols)
    buf = DeviceBuffer(max(e.nbytes, 32))
    try:
        buf.upload(e)
        check(lib.vdb_extended_to_coeff_dev(buf.ptr, _sz(e.shape[0]), ctypes.c_uint32(k), ctypes.c_uint32(ext_k)))
        sync()
        return buf.download(e.shape)
    finally:
        buf.free()


def eval_polys(coeffs, x):
    """out[c] = sum_i coeffs[c][i] * x^i; coeffs: (n_cols, n, 4) uint64 on the host (uploaded), x: (4,)"""
    lib = _lib.init()
    coeffs, x = _fr(coeffs), _fr(x)
    out = np.zeros((coeffs.shape[0], 4), dtype=np.uint64)
    buf = DeviceBuffer(max(coeffs.nbytes, 32))
    try:
        buf.upload(coeffs)
        check(lib.vdb_eval_polys_dev(buf.ptr, _sz(coeffs.shape[0]), _sz(coeffs.shape[1]), _p(x), _p(out)))
        return out
    finally:
        buf.free()


def lookup_permute(inputs, table, usable_rows, max_bits):
    """inputs: (n_cols, n, 4), table: (n, 4) Montgomery Fr on the host; returns (permuted_input, permuted_table)"""
    lib = _lib.init()
    inputs, table = _fr(inputs), _fr(table)
    n_cols, n = inputs.shape[0], inputs.shape[1]
    bufs = [DeviceBuffer(max(inputs.nbytes, 32)), DeviceBuffer(max(table.nbytes, 32)), DeviceBuffer(max(inputs.nbytes, 32)), DeviceBuffer(max(inputs.nbytes, 32))]
    try:
        bufs[0].upload(inputs)
        bufs[1].upload(table)
        check(lib.vdb_lookup_permute_dev(bufs[0].ptr, bufs[1].ptr, _sz(n_cols), _sz(n), _sz(usable_rows), ctypes.c_uint32(max_bits), bufs[2].ptr, bufs[3].ptr))
        sync()
        return bufs[2].download((n_cols, n, 4)), bufs[3].download((n_cols, n, 4))
    finally:
        for b in bufs:
            b.free()


def fr_delta():
    """halo2curves bn256 Fr::DELTA (Montgomery)"""
    out = np.zeros(4, dtype=np.uint64)
    check(_lib.load().vdb_fr_delta(_p(out)))
    return out


def _with_buffers(arrays, n_out_bytes, call):
    bufs = [DeviceBuffer(max(a.nbytes, 32)) for a in arrays] + [DeviceBuffer(max(nb, 32)) for nb in n_out_bytes]
    try:
        for b, a in zip(bufs, arrays):
            b.upload(a)
        call(*[b.ptr for b in bufs])
        sync()
        return bufs[len(arrays):]
    except Exception:
        for b in bufs[len(arrays):]:
            b.free()
        raise
    finally:
        for b in bufs[: len(arrays)]:
            b.free()


def permutation_sigma(mapping, k, delta=None):
    """mapping: (n_cols, 2^k) uint64 words col' << 32 | row'; returns the sigma columns (n_cols, 2^k, 4)"""
    lib = _lib.init()
    mapping = np.ascontiguousarray(mapping, dtype=np.uint64)
    n_cols, n = mapping.shape
    delta = fr_delta() if delta is None else _fr(delta)
    (out,) = _with_buffers([mapping], [n_cols * n * 32],
                           lambda m, o: check(lib.vdb_permutation_sigma_dev(m, _sz(n_cols), ctypes.c_uint32(k), _p(delta), o)))
    try:
        return out.download((n_cols, n, 4))
    finally:
        out.free()


def permutation_product(cols, sigma, usable_rows, chunk_len, beta, gamma, delta=None):
    """running products of the permutation argument, one column per chunk of chunk_len columns: (n_chunks, 2^k, 4)"""
    lib = _lib.init()
    cols, sigma = _fr(cols), _fr(sigma)
    n_cols, n = cols.shape[0], cols.shape[1]
    k = n.bit_length() - 1
    n_chunks = -(-n_cols // chunk_len)
    delta = fr_delta() if delta is None else _fr(delta)
    beta, gamma = _fr(beta), _fr(gamma)
    (out,) = _with_buffers([cols, sigma], [n_chunks * n * 32], lambda c, s, o: check(lib.vdb_permutation_product_dev(
        c, s, _sz(n_cols), ctypes.c_uint32(k), _sz(usable_rows), _sz(chunk_len), _p(beta), _p(gamma), _p(delta), o)))
    try:
        return out.download((n_chunks, n, 4))
    finally:
        out.free()


def lookup_product(inputs, table, perm_inputs, perm_table, usable_rows, beta, gamma):
    """running products of the lookup argument, one per input column: (n_cols, n, 4)"""
    lib = _lib.init()
    inputs, table, perm_inputs, perm_table = _fr(inputs), _fr(table), _fr(perm_inputs), _fr(perm_table)
    n_cols, n = inputs.shape[0], inputs.shape[1]
    beta, gamma = _fr(beta), _fr(gamma)
    (out,) = _with_buffers([inputs, table, perm_inputs, perm_table], [n_cols * n * 32], lambda a, t, pa, pt, o: check(lib.vdb_lookup_product_dev(
        a, t, pa, pt, _sz(n_cols), _sz(n), _sz(usable_rows), _p(beta), _p(gamma), o)))
    try:
        return out.download((n_cols, n, 4))
    finally:
        out.free()


def kate_div(coeffs, x):
    """(p(X) - p(x)) / (X - x) per polynomial; returns (quotients (n_cols, n, 4), remainders p(x) (n_cols, 4))"""
    lib = _lib.init()
    coeffs, x = _fr(coeffs), _fr(x)
    n_cols, n = coeffs.shape[0], coeffs.shape[1]
    rem = np.zeros((n_cols, 4), dtype=np.uint64)
    (out,) = _with_buffers([coeffs], [n_cols * n * 32], lambda c, o: check(lib.vdb_kate_div_dev(c, _sz(n_cols), _sz(n), _p(x), o, _p(rem))))
    try:
        return out.download((n_cols, n, 4)), rem
    finally:
        out.free()


def poly_lincomb(polys, v):
    """sum_c v^(n_cols-1-c) p_c, coefficient-wise: (n, 4)"""
    lib = _lib.init()
    polys, v = _fr(polys), _fr(v)
    n_cols, n = polys.shape[0], polys.shape[1]
    zero = np.zeros((n, 4), dtype=np.uint64)
    bufs = [DeviceBuffer(max(polys.nbytes, 32)), DeviceBuffer(max(zero.nbytes, 32))]
    try:
        bufs[0].upload(polys)
        bufs[1].upload(zero)
        check(lib.vdb_poly_lincomb_dev(bufs[0].ptr, _sz(n_cols), _sz(n), _p(v), bufs[1].ptr))
        sync()
        return bufs[1].download((n, 4))
    finally:
        for b in bufs:
            b.free()


def grand_product(num, den):
    """z[c][0] = 1, z[c][i+1] = z[c][i] * num[c][i] / den[c][i]; num, den: (n_cols, n, 4) uint64 (Montgomery Fr)."""
    lib = _lib.init()
    num, den = _fr(num), _fr(den)
    n_cols, n = num.shape[0], num.shape[1]
    bufs = [DeviceBuffer(max(num.nbytes, 32)) for _ in range(3)]
    try:
        bufs[0].upload(num)
        bufs[1].upload(den)
        check(lib.vdb_grand_product_dev(bufs[0].ptr, bufs[1].ptr, _sz(n_cols), _sz(n), bufs[2].ptr))
        sync()
        return bufs[2].download((n_cols, n, 4))
    finally:
        for b in bufs:
            b.free()


class Transcript:
    """Fiat–Shamir transcript + proof bytes (vdb_transcript_*): Poseidon sponge of width t; host code, no GPU needed."""

    def __init__(self, t=5, r_f=8, r_p=60):
        self.L = _lib.load()
        self.h = ctypes.c_void_p()
        check(self.L.vdb_transcript_new(t, r_f, r_p, ctypes.byref(self.h)))

    def set_sign_bit(self, bit):
        """bit of a compressed point's last byte that says "y is odd": 6 (default) or 7"""
        check(self.L.vdb_transcript_set_sign_bit(self.h, ctypes.c_uint32(bit)))

    def common_scalar(self, s):
        check(self.L.vdb_transcript_common_scalar(self.h, _p(_fr(s))))

    def common_point(self, pt):
        check(self.L.vdb_transcript_common_point(self.h, _p(np.ascontiguousarray(pt, dtype=np.uint64))))

    def write_scalar(self, s):
        check(self.L.vdb_transcript_write_scalar(self.h, _p(_fr(s))))

    def write_point(self, pt):
        check(self.L.vdb_transcript_write_point(self.h, _p(np.ascontiguousarray(pt, dtype=np.uint64))))

    def write_points(self, pts):
        pts = np.ascontiguousarray(pts, dtype=np.uint64).reshape(-1, 8)
        check(self.L.vdb_transcript_write_points(self.h, _p(pts), _sz(pts.shape[0])))

    def write_scalars(self, ss):
        ss = np.ascontiguousarray(ss, dtype=np.uint64).reshape(-1, 4)
        check(self.L.vdb_transcript_write_scalars(self.h, _p(ss), _sz(ss.shape[0])))

    def common_points(self, pts):
        pts = np.ascontiguousarray(pts, dtype=np.uint64).reshape(-1, 8)
        check(self.L.vdb_transcript_common_points(self.h, _p(pts), _sz(pts.shape[0])))

    def common_scalars(self, ss):
        ss = np.ascontiguousarray(ss, dtype=np.uint64).reshape(-1, 4)
        check(self.L.vdb_transcript_common_scalars(self.h, _p(ss), _sz(ss.shape[0])))

    def flush(self):
        """absorb the complete chunks written so far now (vdb_transcript_flush): host work beside queued device work"""
        check(self.L.vdb_transcript_flush(self.h))

    def squeeze(self):
        out = np.zeros(4, dtype=np.uint64)
        check(self.L.vdb_transcript_squeeze(self.h, _p(out)))
        return out

    def proof(self):
        n = ctypes.c_size_t()
        check(self.L.vdb_transcript_proof_len(self.h, ctypes.byref(n)))
        buf = np.zeros(max(n.value, 1), dtype=np.uint8)
        check(self.L.vdb_transcript_proof_bytes(self.h, _p(buf), _sz(buf.size)))
        return buf[: n.value].tobytes()

    def free(self):
        if self.h:
            self.L.vdb_transcript_free(self.h)
            self.h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class DeviceBuffer:
    """A raw HBM allocation owned by the library's context."""

    def __init__(self, nbytes):
        self.L = _lib.init()
        self.nbytes = int(nbytes)
        p = ctypes.c_void_p()
        check(self.L.vdb_malloc(ctypes.byref(p), _sz(self.nbytes)))
        self.ptr = p

    def upload(self, arr, offset=0):
        arr = np.ascontiguousarray(arr)
        assert offset + arr.nbytes <= self.nbytes
        check(self.L.vdb_memcpy_h2d(ctypes.c_void_p(self.ptr.value + offset), _p(arr), _sz(arr.nbytes)))

    def download(self, shape, dtype=np.uint64, offset=0):
        out = np.empty(shape, dtype=dtype)
        assert offset + out.nbytes <= self.nbytes
        check(self.L.vdb_memcpy_d2h(_p(out), ctypes.c_void_p(self.ptr.value + offset), _sz(out.nbytes)))
        return out

    def at(self, offset):
        return ctypes.c_void_p(self.ptr.value + int(offset))

    def free(self):
        if self.ptr is not None and self.ptr.value:
            check(self.L.vdb_free(self.ptr))
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class DeviceView(DeviceBuffer):
    """`nbytes` of another DeviceBuffer's allocation from `offset` on: taken wherever a DeviceBuffer is read, owns nothing (free() is a
    no-op; the view is valid as long as its owner's allocation)"""

    def __init__(self, owner, offset, nbytes):
        assert 0 <= int(offset) and int(offset) + int(nbytes) <= owner.nbytes
        self.L, self.owner, self.nbytes, self.ptr = owner.L, owner, int(nbytes), owner.at(offset)

    def free(self):
        self.ptr = None


def mem_info():
    """(free, total) bytes of HBM on this device"""
    f, t = ctypes.c_size_t(), ctypes.c_size_t()
    check(_lib.init().vdb_mem_info(ctypes.byref(f), ctypes.byref(t)))
    return f.value, t.value


def scratch_held():
    """bytes the library's cached work buffers hold (what vdb_scratch_release would give back)"""
    b = ctypes.c_size_t()
    check(_lib.init().vdb_scratch_held(ctypes.byref(b)))
    return b.value


def alloc_stats(reset=False):
    """(seconds, bytes, calls) of the device allocations made through the library since start / the last reset (vdb_alloc_stats)"""
    sec, b, n = ctypes.c_double(), ctypes.c_uint64(), ctypes.c_uint64()
    _lib.load().vdb_alloc_stats(ctypes.byref(sec), ctypes.byref(b), ctypes.byref(n), 1 if reset else 0)
    return sec.value, b.value, n.value


KEYGEN_SCRATCH_CAP = 16 << 30      # bound of the MSM's work space while setup / keygen allocate the proving key (vdb_msm_set_scratch_cap)


def msm_scratch_cap(nbytes):
    check(_lib.init().vdb_msm_set_scratch_cap(_sz(nbytes)))


def sync():
    check(_lib.init().vdb_sync())


def timer_start():
    check(_lib.init().vdb_timer_start())


def timer_stop():
    ms = ctypes.c_float(0)
    check(_lib.init().vdb_timer_stop(ctypes.byref(ms)))
    return ms.value


def profile_begin(deferred=False):
    """deferred: do not wait for each launch; the events are read in profile_end (kernels run as in the untimed path)"""
    check(_lib.init().vdb_profile_begin_deferred() if deferred else _lib.init().vdb_profile_begin())


def profile_end():
    import json
    buf = ctypes.create_string_buffer(1 << 16)
    check(_lib.init().vdb_profile_end(buf, _sz(len(buf))))
    return json.loads(buf.value.decode())
