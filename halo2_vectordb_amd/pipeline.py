"""HBM-resident driver of the proving hot path for one circuit (plumbing above the C ABI).

Mirrors what the reference's `Prove` arm does up to the committed / extended advice columns
(/root/reference/src/scaffold/mod.rs:284-298 -> create_proof):

    closure (witness gen)  ->  assign_threads_in (stream -> columns)  ->  commit_lagrange per column
    ->  lagrange_to_coeff  ->  coeff_to_extended

`setup()` plays the Keygen arm's role for the layout (src/scaffold/mod.rs:267-283): one run with gate
selectors recorded, from which the break points ("pinning") are derived.  Everything stays in HBM;
only commitments (64 B per column) come back to the host.
"""
import contextlib
import ctypes
import functools
import math

import numpy as np

from . import api
from ._lib import check
from .circuit_sym import FP_UNARY_OPS
from .protocol import MINIMUM_ROWS, N_BLIND, constraint_degree, fr_from_int

B = 32      # bytes per field element


def sift_like_vectors(seed, n, dim, k_distinct=0):
    """integers uniform in [0, 218] stored as f64; rows non-zero; first K rows distinct."""
    while True:
        rng = np.random.default_rng(seed)
        v = rng.integers(0, 219, size=(n, dim)).astype(np.float64)
        ok = (v.sum(axis=1) > 0).all()
        if k_distinct:
            ok = ok and len({tuple(r) for r in v[:k_distinct]}) == k_distinct
        if ok:
            return v, seed
        seed += 1


def shard_range(n_cols, rank, world):
    """Contiguous block [lo, hi) of a list of `n_cols` columns owned by `rank`."""
    return n_cols * rank // world, n_cols * (rank + 1) // world


def column_shards(n_adv, n_lk, world):
    """Per rank: (advice block, lookup block).  Advice and lookup columns are split separately so that every rank's
    blocks cover about the same stretch of the witness stream (lookup cells are emitted alongside the advice cells
    that are range-checked), which is what lets each rank generate only its part of the witness."""
    return [(shard_range(n_adv, r, world), shard_range(n_lk, r, world)) for r in range(world)]


def balanced_ranges(cost, world):
    """Contiguous blocks of a column list with (nearly) equal summed cost: block r ends at the first column where the
    running cost reaches (r + 1) / world of the total."""
    cost = np.asarray(cost, dtype=np.float64)
    n = len(cost)
    if n == 0:
        return [(0, 0)] * world
    cum = np.cumsum(cost)
    cuts = [0]
    for r in range(1, world):
        cuts.append(max(cuts[-1], min(n, int(np.searchsorted(cum, cum[-1] * r / world, side="left")) + 1)))
    cuts.append(n)
    return [(cuts[r], max(cuts[r], cuts[r + 1])) for r in range(world)]


def balanced_column_shards(var_adv, var_lk, world, msm_share=0.22):
    """Like column_shards, but the blocks equalise estimated time instead of column count: every column costs one unit
    (NTT, layout, bucket reduction) plus `msm_share` units per mean-column's worth of MSM entries (the non-zero signed
    window digits of its non-constant cells: what its commitment sorts and accumulates; the share is the measured ratio
    of those two groups of kernels: ~9 us of accumulate / combine per mean column against ~33 us of NTT, sort and
    bucket reduction).  Witness columns differ a lot here (input and indicator columns are
    nearly empty, fixed-point columns hold 100-bit values), which is what skews equal-count blocks."""
    var_adv = np.asarray(var_adv, dtype=np.float64)
    var_lk = np.asarray(var_lk, dtype=np.float64)
    mean = max(1.0, (var_adv.sum() + var_lk.sum()) / max(1, len(var_adv) + len(var_lk)))
    adv = balanced_ranges(1.0 + msm_share * var_adv / mean, world)
    lk = balanced_ranges(1.0 + msm_share * var_lk / mean, world)
    return list(zip(adv, lk))


def set_cols(n_lk_cols):
    """columns per product polynomial of the permutation argument, halo2's chunk_len = cs.degree() - 2 (protocol.constraint_degree: 4 for a
    circuit with lookup columns, 3 without): block boundaries of a sharded job fall on sets"""
    return constraint_degree(n_lk_cols) - 2


SET_COLS = 2


def align_column_shards(shards, n_adv, n_lk, chunk=SET_COLS):
    """The same blocks with their inner boundaries moved (by at most chunk - 1 columns) onto the boundaries of the permutation
    argument's column sets: the permutation runs over [advice | lookup | constants | instance] in sets of `chunk` consecutive
    columns, so an advice cut a must have a % chunk == 0 and a lookup cut l must have (n_adv + l) % chunk == 0.  Then every
    product polynomial's columns lie on one rank — except the one set that spans the advice / lookup junction — and the prover
    rounds shard by the same blocks as the hot path (rounds.ShardMap)."""
    world = len(shards)

    def snap(cuts, offset, n):
        out = [0]
        for c in cuts[1:-1]:
            down = c - (c + offset) % chunk
            up = down + chunk
            c2 = down if (c - down <= up - c or up > n) else up
            out.append(min(n, max(out[-1], c2, 0)))
        out.append(n)
        return out
    a_cuts = snap([0] + [shards[r][0][1] for r in range(world)], 0, n_adv)
    l_cuts = snap([0] + [shards[r][1][1] for r in range(world)], n_adv, n_lk)
    # a lookup cut below the first set that starts inside the lookup columns would split the junction set's columns over three ranks
    first = (-n_adv) % chunk
    l_cuts = [0] + [min(n_lk, max(c, first)) if c > 0 else 0 for c in l_cuts[1:-1]] + [n_lk]
    return [((a_cuts[r], a_cuts[r + 1]), (l_cuts[r], l_cuts[r + 1])) for r in range(world)]


def gather_commitments(dist, local, shards, device):
    """The one real exchange step of the path: all_gather of the 64-byte commitments of every rank's column
    shard (RCCL on GPUs, gloo in the CPU test).  `local`: (my_cols, 8) uint64, [advice block | lookup block];
    `shards`: the per-rank ((a_lo, a_hi), (l_lo, l_hi)) list every rank derived identically (column_shards /
    balanced_column_shards).  Returns (n_adv + n_lk, 8) in the unsharded order [all advice | all lookup]."""
    import torch
    world = len(shards)
    counts = [(a[1] - a[0]) + (l[1] - l[0]) for a, l in shards]
    mx = max(counts)
    mine = torch.zeros((mx, 8), dtype=torch.int64, device=device)
    if len(local):
        mine[: len(local)] = torch.from_numpy(np.ascontiguousarray(local).view(np.int64)).to(device)
    gathered = [torch.zeros_like(mine) for _ in range(world)]
    dist.all_gather(gathered, mine)
    parts = [g.cpu().numpy().view(np.uint64) for g in gathered]
    adv = [p[: a[1] - a[0]] for p, (a, l) in zip(parts, shards)]
    lk = [p[a[1] - a[0]: (a[1] - a[0]) + (l[1] - l[0])] for p, (a, l) in zip(parts, shards)]
    return np.concatenate(adv + lk)


# ---------------------------------------------------------------------------------------------------------------------------
# The alternative partition of SURVEY §8(e): ONE set of columns, the POINTS (rows) split over the ranks.  Only of use when
# there are fewer columns than GPUs (never at the BASELINE configs, where columns are sharded instead); it is what
# BASELINE.json's "all-reduce only for the final bucket reduction" describes.  RCCL has no curve reduction operator: the
# exchange is an all_gather of the per-rank partial commitments (64 B per column and rank) followed by world - 1 group
# additions per column on every rank (vdb_g1_sum) — exact and order independent after the affine normalisation.
def point_shard(rows, rank, world):
    return rows * rank // world, rows * (rank + 1) // world


def point_sharded_partials(srs_shard, cols_dev, n_cols, rows, lo, hi):
    """Commitments of rows [lo, hi) of n_cols device-resident columns (stride `rows`) against an Srs that holds exactly the
    bases of those rows: (n_cols, 8)."""
    lib = srs_shard.L
    desc = np.zeros((n_cols, 3), dtype=np.uint64)                    # vdb_colsrc {src, len, blind}
    base = cols_dev.ptr.value if hasattr(cols_dev, "ptr") else int(cols_dev)
    desc[:, 0] = base + (np.arange(n_cols, dtype=np.uint64) * np.uint64(rows) + np.uint64(lo)) * np.uint64(32)
    desc[:, 1] = hi - lo
    d_src = api.DeviceBuffer(desc.nbytes)
    d_src.upload(desc)
    out = np.zeros((n_cols, 8), dtype=np.uint64)
    try:
        check(lib.vdb_msm_batch_src_dev_begin(srs_shard.h, 1, d_src.ptr, ctypes.c_size_t(n_cols), ctypes.c_size_t(hi - lo), 0, None, None))
        check(lib.vdb_msm_batch_end(api._p(out), ctypes.c_size_t(n_cols)))
    finally:
        d_src.free()
    return out


def combine_partials(parts):
    """(world, n_cols, 8) partial commitments -> (n_cols, 8): the group sum per column (on the device)."""
    parts = np.ascontiguousarray(parts, dtype=np.uint64)
    world, n_cols = parts.shape[0], parts.shape[1]
    out = np.zeros((n_cols, 8), dtype=np.uint64)
    check(api._lib.init().vdb_g1_sum(api._p(parts), ctypes.c_size_t(world), ctypes.c_size_t(n_cols), api._p(out)))
    return out


def allgather_partials(dist, local, device):
    """all_gather of every rank's (n_cols, 8) partial commitments -> (world, n_cols, 8) on the host"""
    import torch
    mine = torch.from_numpy(np.ascontiguousarray(local).view(np.int64)).to(device)
    gathered = [torch.zeros_like(mine) for _ in range(dist.get_world_size())]
    dist.all_gather(gathered, mine)
    return np.stack([g.cpu().numpy().view(np.uint64) for g in gathered])


def _end_to_end(codes, size):
    """Independent gadget calls laid end to end in the stream: `size(code, byref cells, byref lookup cells)` is the calls' size entry
    point.  -> ([(code, first cell, first lookup cell)] per call, cells of all, lookup cells of all)."""
    parts = []
    cells_total = lk_total = 0
    for code in codes:
        cells, lk = ctypes.c_uint64(), ctypes.c_uint64()
        check(size(code, ctypes.byref(cells), ctypes.byref(lk)))
        parts.append((code, cells_total, lk_total))
        cells_total, lk_total = cells_total + cells.value, lk_total + lk.value
    return parts, cells_total, lk_total


class HotPath:
    """The HBM-resident driver of one circuit on one GPU (or one rank's block of its columns): witness -> layout -> commit -> NTT.
    Circuit neutral: a circuit class states its inputs and sizes (_input_vectors, n_input_rows, _circuit_size), its outputs
    (_alloc_outputs, registered with _output), the gadget calls that emit its cells after the input rows (_emit), what it makes
    public (public_values_dev), what it returns (results) and its constraint map (constraint_map)."""

    def __init__(self, n, dim, k, P, L, seed=None, tau=None, col_shard=(0, 1), vectors=None, blind_seed=None, params=None):
        """`tau`: toxic-waste scalar of the "unsafe" SRS as a canonical integer; None = the scalar the reference's
        `gen_srs(k)` derives from its fixed ChaCha20 seed (srs.gen_srs_tau, src/scaffold/mod.rs:260).
        `params`: an SRS whose scalar nobody knows instead — an srs.ParamsKZG (downsized to k on the device when its k is larger)
        or the path of a halo2 params file (read at k), what gen_srs(k) loads from params/kzg_bn254_{k}.srs when that exists.
        Not together with `tau`; `self.tau` stays None and `self.tau_g2` / `self.g2` carry the SRS's G2 side.
        `vectors`: the f64 rows the circuit assigns first (the `--input` file of the reference's examples,
        src/scaffold/mod.rs:64-77); None = the circuit's seeded synthetic rows (SIFT-shaped).
        `blind_seed`: None = the blinding rows of every column are drawn afresh from the operating system's entropy for every
        proof (step), as halo2's create_proof does with its OsRng (reached from src/scaffold/mod.rs:296); an integer fixes
        them — a test hook for comparing commitments across runs, never for real proofs (two proofs that share blinds leak
        the difference of their witnesses)."""
        self.blind_seed = blind_seed
        self._entropy = None
        self.given_vectors = None if vectors is None else np.ascontiguousarray(vectors, dtype=np.float64)
        self.n, self.dim, self.k, self.P, self.L = n, dim, k, P, L
        self.rows = 1 << k
        self.lib = api.init()
        self.rank, self.world = col_shard
        self.seed = seed
        if params is not None and tau is not None:
            raise ValueError("give the SRS as tau or as params, not both")
        self.tau = tau
        self.params = params
        self.tau_g2 = self.g2 = None
        self._outputs = []
        self.factor_constants = True
        self.shard_witness = True   # generate only the witness cells this rank's columns hold (values are computed everywhere)
        self.balance_shards = True  # equalise estimated time per rank instead of column count
        self.virtual_layout = True  # commit and transform straight from the witness stream (no stream -> column copy)
        self.msm_window_bits = 0    # 0 = the library's default (11 bits for k > 8: most witness scalars are short)
        self.ext_block_cols = None  # columns of extended cosets held at a time; None = all if they fit, else what leaves ext_reserve_bytes free
        self.ext_reserve_bytes = 64 << 30

    # ------------------------------------------------------------------ keygen-like setup (untimed)
    def setup(self, pinning=None):
        """`pinning`: path of a configs/{name}.json written by an earlier keygen (io.write_pinning); when given, its break
        points are used as they are — the Prove arm of the reference (src/scaffold/mod.rs:285-287) — after checking that
        they describe this circuit; otherwise they are derived from the keygen-style run, like the Keygen arm."""
        # the MSMs of setup and keygen (constant points, fixed columns) work in a bounded work space: on a still empty card the default
        # (half of the free HBM) would map up to 96 GiB for a two-second MSM, and mapping fresh HBM costs ~30 ms / GiB; step() lifts it
        api.msm_scratch_cap(api.KEYGEN_SCRATCH_CAP)
        self._load_inputs()
        d_sel = self._plan_layout(pinning)
        self._load_srs()
        self._partition_columns(d_sel)
        self._column_sources()
        self._factor_constants(d_sel)
        self._size_cosets()
        return self

    def _load_inputs(self):
        """The input rows on the device, the witness streams and the circuit's outputs."""
        vec, self.seed = self._input_vectors() if self.given_vectors is None else (self.given_vectors, self.seed)
        assert vec.shape == (self.n_input_rows(), self.dim), "input rows do not match the circuit's shape"
        self.vectors_f64 = vec
        self.qvec = api.quantize(vec, self.P)
        self.n_in, n_gadget_cells, self.n_lookup = self._circuit_size()
        self.n_cells = self.n_in + n_gadget_cells
        self.d_vec = api.DeviceBuffer(self.qvec.nbytes)
        self.d_vec.upload(self.qvec)
        self.d_stream = api.DeviceBuffer(self.n_cells * B)
        self.d_lookup = api.DeviceBuffer(max(self.n_lookup, 1) * B)
        self._alloc_outputs()

    def _plan_layout(self, pinning):
        """Keygen-style run: record gate starts, derive the break points (the reference pins them in configs/*.json) and the column
        counts.  -> the gate-start flags (device), which the later steps read and _factor_constants frees."""
        lib = self.lib
        d_sel = api.DeviceBuffer(self.n_cells)
        check(lib.vdb_memset_dev(d_sel.ptr, 0, ctypes.c_size_t(self.n_cells)))
        self._witness(sel=d_sel)
        nbp = ctypes.c_uint64()
        check(lib.vdb_layout_plan_dev(d_sel.ptr, ctypes.c_uint64(self.n_cells), self.k, MINIMUM_ROWS, None, ctypes.c_uint64(0), ctypes.byref(nbp)))
        self.bp = np.zeros(max(nbp.value, 1), dtype=np.uint64)
        check(lib.vdb_layout_plan_dev(d_sel.ptr, ctypes.c_uint64(self.n_cells), self.k, MINIMUM_ROWS, api._p(self.bp), ctypes.c_uint64(self.bp.size),
                                      ctypes.byref(nbp)))
        self.bp = self.bp[:nbp.value]
        if pinning is not None:
            from .io import read_pinning
            params, bp = read_pinning(pinning)
            if params["degree"] != self.k or params["lookup_bits"] != self.L or not np.array_equal(bp, self.bp):
                raise ValueError("pinning file does not describe this circuit (degree, lookup_bits or break points differ)")
            self.bp = bp
        self.n_adv_cols = len(self.bp) + 1
        self.n_lk_cols = math.ceil(self.n_lookup / (self.rows - MINIMUM_ROWS))
        self.n_cols = self.n_adv_cols + self.n_lk_cols
        return d_sel

    def _load_srs(self):
        if self.params is not None:
            from .srs import ParamsKZG
            params = self.params if isinstance(self.params, ParamsKZG) else ParamsKZG.read(self.params, self.k)
            params = params.downsize(self.k)      # ValueError when the params hold fewer than 2^k points
            g, gl = params.g, params.g_lagrange
            self.g2, self.tau_g2 = params.g2, params.s_g2
        else:
            if self.tau is None:
                from .srs import gen_srs_tau
                self.tau = gen_srs_tau()
            g, gl = api.srs_setup_unsafe(self.k, fr_from_int(self.tau))
        self.g_lagrange = gl
        self.g_monomial = g
        self.srs = api.Srs(self.k, None, gl, window_bits=self.msm_window_bits)

    def _partition_columns(self, d_sel):
        """Column sharding over ranks: a block of the advice columns and a block of the lookup columns each, and the stretches of the
        witness streams they hold (the rank window of _window)."""
        lib = self.lib
        self.shards = column_shards(self.n_adv_cols, self.n_lk_cols, self.world)
        if self.world > 1 and self.balance_shards:
            # keygen-time statistics of the layout just produced (every rank computes the same numbers)
            n_el = self.n_adv_cols * self.rows
            d_tmpm = api.DeviceBuffer(n_el)
            check(lib.vdb_layout_const_mask_dev(d_sel.ptr, ctypes.c_uint64(self.n_cells), api._p(self.bp), ctypes.c_uint64(len(self.bp)), self.k, d_tmpm.ptr))
            d_tmpc = api.DeviceBuffer(max(self.n_adv_cols, self.n_lk_cols, 1) * self.rows * B)
            check(lib.vdb_layout_columns_dev(self.d_stream.ptr, ctypes.c_uint64(self.n_cells), api._p(self.bp), ctypes.c_uint64(len(self.bp)), self.k,
                                             d_tmpc.ptr, None, 0))
            var_adv = np.zeros(self.n_adv_cols, dtype=np.uint64)
            check(lib.vdb_msm_count_entries_dev(self.srs.h, d_tmpc.ptr, ctypes.c_size_t(self.n_adv_cols), ctypes.c_size_t(self.rows), d_tmpm.ptr,
                                                api._p(var_adv)))
            var_lk = np.zeros(max(self.n_lk_cols, 1), dtype=np.uint64)
            if self.n_lk_cols:
                check(lib.vdb_layout_lookup_dev(self.d_lookup.ptr, ctypes.c_uint64(self.n_lookup), self.k, MINIMUM_ROWS, d_tmpc.ptr,
                                                ctypes.c_uint64(self.n_lk_cols), None, 0))
                check(lib.vdb_msm_count_entries_dev(self.srs.h, d_tmpc.ptr, ctypes.c_size_t(self.n_lk_cols), ctypes.c_size_t(self.rows), None,
                                                    api._p(var_lk)))
            d_tmpm.free()
            d_tmpc.free()
            self.msm_entries = (var_adv, var_lk[: self.n_lk_cols])
            self.shards = balanced_column_shards(var_adv, var_lk[: self.n_lk_cols], self.world)
        if self.world > 1:
            self.shards = align_column_shards(self.shards, self.n_adv_cols, self.n_lk_cols, set_cols(self.n_lk_cols))
        (self.a_lo, self.a_hi), (self.l_lo, self.l_hi) = self.shards[self.rank]
        self.my_adv, self.my_lk = self.a_hi - self.a_lo, self.l_hi - self.l_lo
        self.my_cols = self.my_adv + self.my_lk
        # the stretch of the flat stream / lookup stream those columns hold (column c = stream[starts[c] : starts[c] + bp[c] + 1])
        starts = np.concatenate([[0], np.cumsum(self.bp, dtype=np.uint64)]).astype(np.uint64)
        if self.my_adv:
            s_hi = int(starts[self.a_hi - 1]) + int(self.bp[self.a_hi - 1]) + 1 if self.a_hi - 1 < len(self.bp) else self.n_cells
            self.win_adv = (int(starts[self.a_lo]), s_hi)
        else:
            self.win_adv = (0, 0)
        max_rows = self.rows - MINIMUM_ROWS
        self.win_lk = (self.l_lo * max_rows, min(self.l_hi * max_rows, self.n_lookup)) if self.my_lk else (0, 0)

    def _column_sources(self):
        """The blinding scalars, the column buffer and the descriptors of where each of my columns lies in the streams."""
        lib = self.lib
        # N_BLIND blinding scalars per column, uniform in Fr: 64 bytes of entropy each, reduced on the device
        self.d_blind = api.DeviceBuffer(self.n_cols * N_BLIND * B)
        self.d_wide = api.DeviceBuffer(self.n_cols * N_BLIND * 64)
        self.refresh_blinds()
        self.d_cols = api.DeviceBuffer(max(self.my_cols, 1) * self.rows * B)
        # column descriptors of my [advice block | lookup block]: where each column lies in the streams (data independent)
        self.d_src = api.DeviceBuffer(max(self.my_cols, 1) * 24)
        if self.my_adv:
            check(lib.vdb_colsrc_build_dev(self.d_stream.ptr, ctypes.c_uint64(self.n_cells), api._p(self.bp), ctypes.c_uint64(len(self.bp)), self.k,
                                           ctypes.c_uint64(self.a_lo), ctypes.c_uint64(self.a_hi), self.d_blind.ptr, N_BLIND, self.d_src.ptr))
        if self.my_lk:
            check(lib.vdb_colsrc_build_lookup_dev(self.d_lookup.ptr, ctypes.c_uint64(self.n_lookup), self.k, MINIMUM_ROWS, ctypes.c_uint64(self.l_lo),
                                                  ctypes.c_uint64(self.l_hi), self.d_blind.at(self.n_adv_cols * N_BLIND * B), N_BLIND,
                                                  self.d_src.at(self.my_adv * 24)))

    def _factor_constants(self, d_sel):
        """Keygen-time factoring of the constant cells: column-layout mask of the QuantumCell::Constant cells and the per-column MSM of
        exactly those cells (data independent, so computed once like the rest of the proving key).  Frees `d_sel`."""
        lib = self.lib
        # (lookup columns hold no constants: their mask stays zero and their constant point is the identity).
        # Only this rank's advice columns, laid out in the column buffer the step overwrites anyway: no second buffer of the
        # columns' size (33.7 GiB at C4') is allocated and handed back.
        n_el = self.n_adv_cols * self.rows
        d_fmask = api.DeviceBuffer(n_el)                    # one byte per cell of ALL advice columns (1.1 GiB at C4')
        check(lib.vdb_layout_const_mask_dev(d_sel.ptr, ctypes.c_uint64(self.n_cells), api._p(self.bp), ctypes.c_uint64(len(self.bp)), self.k, d_fmask.ptr))
        d_sel.free()
        self.d_mask = api.DeviceBuffer(max(self.my_cols, 1) * self.rows)
        check(lib.vdb_memset_dev(self.d_mask.ptr, 0, ctypes.c_size_t(max(self.my_cols, 1) * self.rows)))
        const_mine = np.zeros((self.my_cols, 8), dtype=np.uint64)
        if self.my_adv:
            check(lib.vdb_memcpy_d2d(self.d_mask.ptr, d_fmask.at(self.a_lo * self.rows), ctypes.c_size_t(self.my_adv * self.rows)))
            check(lib.vdb_layout_columns_range_dev(self.d_stream.ptr, ctypes.c_uint64(self.n_cells), api._p(self.bp), ctypes.c_uint64(len(self.bp)), self.k,
                                                   ctypes.c_uint64(self.a_lo), ctypes.c_uint64(self.a_hi), self.d_cols.ptr, None, 0))
            check(lib.vdb_mask_select_dev(self.d_cols.ptr, self.d_mask.ptr, ctypes.c_uint64(self.my_adv * self.rows), 1, self.d_cols.ptr))
            pts = np.zeros((self.my_adv, 8), dtype=np.uint64)
            check(lib.vdb_msm_batch_dev(self.srs.h, 1, self.d_cols.ptr, ctypes.c_size_t(self.my_adv), ctypes.c_size_t(self.rows), api._p(pts)))
            const_mine[: self.my_adv] = pts
        self.const_points = const_mine                      # [my advice | my lookup] order, like d_cols
        self.d_cpts = api.DeviceBuffer(max(const_mine.nbytes, 64))
        if const_mine.nbytes:
            self.d_cpts.upload(np.ascontiguousarray(const_mine))
        self.const_cell_fraction = float(d_fmask.download((n_el,), dtype=np.uint8).mean()) if n_el <= (1 << 28) else None
        d_fmask.free()
        api.sync()

    def _size_cosets(self):
        """The extended cosets, last: all of them when they fit beside everything above and leave the MSM its work space (C4:
        68 GB), otherwise the largest block of columns that does — the cosets are then produced block after block into the
        same buffer (a circuit larger than HBM streams through: C4' cosine, 20.3 k columns = 170 GB of cosets; C5's Merkle).
        Two columns more than this rank holds: the prover rounds keep the cosets of the constants' fixed column and of the
        instance column behind the advice cosets, so that the permutation argument reads its columns from one contiguous
        block (rounds.py)."""
        per_col = self.rows * 4 * B
        want = max(self.my_cols, 1) + 2
        if self.ext_block_cols is None:
            free, _ = api.mem_info()
            free += api.scratch_held()       # (the bounded work space stays allocated: it is part of what ext_reserve_bytes leaves the MSM)
            fit = (free - self.ext_reserve_bytes) // per_col
            self.ext_cols = want if fit >= want else int(max(min(want, 256), fit // 256 * 256))
        else:
            self.ext_cols = min(want, int(self.ext_block_cols))
        self.d_ext = api.DeviceBuffer(self.ext_cols * per_col)

    # ------------------------------------------------------------------ blinding
    def _draw_entropy(self, seed):
        import os
        nbytes = self.n_cols * N_BLIND * 64
        return os.urandom(nbytes) if seed is None else np.random.default_rng(seed).bytes(nbytes)

    def refresh_blinds(self, seed=None):
        """New blinding rows for every column (halo2: Blind(Scalar::random(OsRng)) per committed polynomial).  The bytes for
        the next proof are drawn while the GPU is busy with this one (step()), so a refresh costs one small upload."""
        seed = self.blind_seed if seed is None else seed
        raw = self._entropy if (seed is None and self._entropy is not None) else self._draw_entropy(seed)
        self._entropy = None
        self.d_wide.upload(np.frombuffer(raw, dtype=np.uint8))
        check(self.lib.vdb_fr_from_wide_dev(self.d_wide.ptr, ctypes.c_size_t(self.n_cols * N_BLIND), self.d_blind.ptr))

    # ------------------------------------------------------------------ what a circuit states
    def _input_vectors(self):
        """(f64 rows that ctx.assign_witnesses puts at the head of the stream, seed actually used)"""
        raise NotImplementedError

    def n_input_rows(self):
        return self.n

    def _circuit_size(self):
        """(cells of ctx.assign_witnesses(quantize_vector(v)) for every input row, cells the gadgets emit, lookup cells)"""
        raise NotImplementedError

    def _alloc_outputs(self):
        """the circuit's output buffers, each made with _output"""
        raise NotImplementedError

    def _emit(self, sel):
        """the circuit's gadget calls, their cells from n_in on (sel: gate-start flag bytes of the stream, or None)"""
        raise NotImplementedError

    def public_values_dev(self):
        """(device pointer, count) of the values the reference's example of this circuit makes public, in make_public order.  Every
        rank computes them (value-only walk), whichever rank's columns hold the cells."""
        raise NotImplementedError

    def results(self):
        raise NotImplementedError

    def constraint_map(self, d_flags, on_device=True):
        """(the circuit's constraint map (circuit_sym.CopyMap over the stream cells), the cells its example makes public in make_public
        order, the stream cell of its Merkle root or None).  d_flags: the flags of a keygen-style run (keygen_flags); on_device: let the
        device place the map of a large circuit (circuit_dev.py) instead of the host."""
        raise NotImplementedError

    # ------------------------------------------------------------------ helpers of the circuits
    def _output(self, nbytes):
        """a device buffer for the circuit's outputs, freed by free()"""
        buf = api.DeviceBuffer(nbytes)
        self._outputs.append(buf)
        return buf

    @staticmethod
    def _sel_at(sel, at):
        """the flag bytes of a gadget call whose cells start `at` cells into the stream"""
        return ctypes.c_void_p(sel.ptr.value + at) if sel is not None else None

    def _window(self, sel, at, lookup=True):
        """The rank window of a gadget call whose cells start `at` cells into the stream: a rank that shards the witness stores only
        the cells its columns hold (the values are computed everywhere).  `lookup`: the call emits lookup cells (else the lookup
        window is empty)."""
        if not (sel is None and self.shard_witness and self.world > 1):
            return contextlib.nullcontext()
        return api.wit_window(adv=tuple(max(0, x - at) for x in self.win_adv), lookup=self.win_lk if lookup else (0, 0))

    def _fetch(self, lo, hi):
        """canonical integers of stream cells [lo, hi)"""
        c = api.fr_to_canonical(self.d_stream.download((hi - lo, 4), offset=lo * B))
        return [int(r[0]) | int(r[1]) << 64 | int(r[2]) << 128 | int(r[3]) << 192 for r in c]

    @staticmethod
    def _fetch_flags(d_flags, lo, hi):
        """flag bytes of stream cells [lo, hi)"""
        return d_flags.download((hi - lo,), dtype=np.uint8, offset=lo)

    # ------------------------------------------------------------------ the pinning file, the input, the layout, the witness
    def write_pinning(self, path):
        """configs/{name}.json of the Keygen arm (src/scaffold/mod.rs:272)."""
        from .io import write_pinning
        write_pinning(path, self.k, self.bp, self.n_lk_cols, self.L)

    def set_vectors(self, vectors_f64):
        """Prove for a different database of the same shape (the keygen-time data above stays untouched)."""
        self.vectors_f64 = np.asarray(vectors_f64, dtype=np.float64)
        self.qvec = api.quantize(self.vectors_f64, self.P)
        self.d_vec.upload(self.qvec)

    def _layout(self, dest=None):
        """My block of advice columns followed by my block of lookup columns, compact in d_cols (or `dest`)."""
        lib = self.lib
        d_cols = self.d_cols if dest is None else dest
        if self.my_adv:
            check(lib.vdb_layout_columns_range_dev(self.d_stream.ptr, ctypes.c_uint64(self.n_cells), api._p(self.bp), ctypes.c_uint64(len(self.bp)), self.k,
                                                   ctypes.c_uint64(self.a_lo), ctypes.c_uint64(self.a_hi), d_cols.ptr, self.d_blind.ptr, N_BLIND))
        if self.my_lk:
            check(lib.vdb_layout_lookup_range_dev(self.d_lookup.ptr, ctypes.c_uint64(self.n_lookup), self.k, MINIMUM_ROWS, ctypes.c_uint64(self.l_lo),
                                                  ctypes.c_uint64(self.l_hi), d_cols.at(self.my_adv * self.rows * B),
                                                  self.d_blind.at(self.n_adv_cols * N_BLIND * B), N_BLIND))

    def _witness(self, sel=None):
        """[assign_witnesses(input rows)] [the gadgets' cells]"""
        if self.n_in:
            check(self.lib.vdb_memcpy_d2d(self.d_stream.ptr, self.d_vec.ptr, ctypes.c_size_t(self.n_in * B)))
        self._emit(sel)

    # ------------------------------------------------------------------ one pass of the hot path
    def step(self, timings=None, blind_seed=None, with_ext=True, sync=True, after_witness=None):
        """`with_ext`: False leaves coeff_to_extended out (a caller that streams the cosets itself, block by block: rounds.py on
        circuits whose cosets do not fit HBM).  `sync`: False returns as soon as the commitments are on the host, the transforms
        still running on the library's stream (the caller absorbs the commitments into its transcript meanwhile; everything it
        queues next is ordered behind them).  `after_witness`: called once the witness kernels are queued and before the
        commitments are (the prover rounds read the public cells out of the stream there)."""
        lib = self.lib
        # the prover's MSM takes the work space its default policy gives it, whatever setup / keygen of any hot path bounded it to
        api.msm_scratch_cap(0)
        self.refresh_blinds(blind_seed)

        def stage(name, fn):
            if timings is not None:
                api.timer_start()
            fn()
            if timings is not None:
                timings[name] = timings.get(name, 0.0) + api.timer_stop()

        stage("witness", self._witness)
        if after_witness is not None:
            after_witness()

        virt = self.virtual_layout and self.k > 10
        if not virt:
            stage("layout", self._layout)
        my = self.d_cols.ptr
        self.commitments = np.zeros((self.my_cols, 8), dtype=np.uint64)

        def commit():
            # the MSM is queued without waiting; the bucket folding of its last batch runs on a second stream beside the NTTs
            mask = self.d_mask.ptr if self.factor_constants else None
            cpts = self.d_cpts.ptr if self.factor_constants else None
            if virt:
                check(lib.vdb_msm_batch_src_dev_begin(self.srs.h, 1, self.d_src.ptr, ctypes.c_size_t(self.my_cols), ctypes.c_size_t(self.rows), N_BLIND, mask, cpts))
            else:
                check(lib.vdb_msm_batch_masked_dev_begin(self.srs.h, 1, my, ctypes.c_size_t(self.my_cols), ctypes.c_size_t(self.rows), mask, cpts))

        def ntt():
            if virt:
                check(lib.vdb_lagrange_to_coeff_src_dev(self.d_src.ptr, my, ctypes.c_size_t(self.my_cols), self.k, N_BLIND))
            else:
                check(lib.vdb_lagrange_to_coeff_dev(my, ctypes.c_size_t(self.my_cols), self.k))
            # cosets of all columns when the buffer holds them, else block after block into the same buffer
            blk = min(self.ext_cols, max(self.my_cols, 1))
            for c0 in range(0, self.my_cols if with_ext else 0, blk):
                nb = min(blk, self.my_cols - c0)
                check(lib.vdb_coeff_to_extended_dev(self.d_cols.at(c0 * self.rows * B), self.d_ext.ptr, ctypes.c_size_t(nb), self.k, 2))
            if self.blind_seed is None and blind_seed is None:
                self._entropy = self._draw_entropy(None)      # the next proof's blinds, drawn while the GPU works on this one
            check(lib.vdb_msm_batch_end(api._p(self.commitments), ctypes.c_size_t(self.my_cols)))

        stage("commit_msm", commit)
        try:
            stage("ntt", ntt)
        except Exception:
            # a deferred MSM must always be collected, or every later MSM is refused ("deferred batch has not been collected")
            lib.vdb_msm_batch_end(None, ctypes.c_size_t(0))
            raise
        if sync:
            api.sync()
        return self.commitments

    # ------------------------------------------------------------------ the Mock stage (src/scaffold/mod.rs:263-266)
    def keygen_flags(self):
        """flag byte per advice cell from a keygen-style run (bit 0 gate start, bit 1 constant cell, bit 2 lookup source), on the device"""
        d_flags = api.DeviceBuffer(self.n_cells)
        check(self.lib.vdb_memset_dev(d_flags.ptr, 0, ctypes.c_size_t(self.n_cells)))
        self._witness(sel=d_flags)     # the flags are data independent; the cells written are those of the current input
        return d_flags

    def mock_check(self, copy_of=None, lookup_src=None, const_stream=None):
        """MockProver::run(..).assert_satisfied() of the reference's Mock arm on the witness as it lies in HBM after a
        step() / relayout(): every gate row, every lookup cell against the range table and — when the maps are given (device
        buffers or int64 arrays) — every copy constraint and every constant.  Returns api.MockReport (rank-unsharded runs)."""
        assert self.world == 1, "the mock check walks the whole witness"
        d_flags = self.keygen_flags()
        self._witness()           # the witness under test (the flag run above wrote the same cells)
        own = []

        def dev(a, dtype):
            if a is None or isinstance(a, (api.DeviceBuffer,)) or hasattr(a, "ptr"):
                return a
            a = np.ascontiguousarray(a, dtype=dtype)
            b = api.DeviceBuffer(max(a.nbytes, 32))
            b.upload(a)
            own.append(b)
            return b
        try:
            c, l, k = dev(copy_of, np.int64), dev(lookup_src, np.int64), dev(const_stream, np.uint64)
            return api.mock_check_dev(self.d_stream.ptr, self.n_cells, d_flags.ptr, self.d_lookup.ptr, self.n_lookup, self.L,
                                      None if c is None else c.ptr, None if l is None else l.ptr, None if k is None else k.ptr)
        finally:
            d_flags.free()
            for b in own:
                b.free()

    def local_index(self, col):
        """Position in this rank's compact column buffer of global column `col` ([all advice | all lookup] numbering)."""
        if col < self.n_adv_cols:
            assert self.a_lo <= col < self.a_hi, "column not held by this rank"
            return col - self.a_lo
        c = col - self.n_adv_cols
        assert self.l_lo <= c < self.l_hi, "column not held by this rank"
        return self.my_adv + c - self.l_lo

    def global_columns(self):
        """Global numbers of the columns this rank holds, in buffer order."""
        return list(range(self.a_lo, self.a_hi)) + [self.n_adv_cols + c for c in range(self.l_lo, self.l_hi)]

    def download_columns(self, col_indices):
        """Lagrange-basis columns as laid out (call right after `layout`, i.e. use relayout()); global column numbers."""
        out = np.zeros((len(col_indices), self.rows, 4), dtype=np.uint64)
        for j, c in enumerate(col_indices):
            out[j] = self.d_cols.download((self.rows, 4), offset=self.local_index(c) * self.rows * B)
        return out

    def relayout(self):
        """Re-run witness + layout only (columns are overwritten in place by the NTT stage)."""
        self._witness()
        self._layout()
        api.sync()

    def free(self):
        for name in ("d_vec", "d_stream", "d_lookup", "d_blind", "d_wide", "d_cols", "d_ext", "d_mask", "d_cpts", "d_src"):
            b = getattr(self, name, None)
            if b is not None:
                b.free()
        for b in self._outputs:
            b.free()
        self._outputs = []
        if getattr(self, "srs", None) is not None:
            self.srs.free()


def _merkle_cells(hp):
    """cells of merkle_commitment over the hot path's n vectors"""
    cells = ctypes.c_uint64()
    check(hp.lib.vdb_wit_merkle_size(hp.n, hp.dim, 0, ctypes.byref(cells)))
    return cells.value


def _merkle_trace(hp, d_vectors, at, sel):
    """merkle_commitment over the n vectors at `d_vectors`, its cells `at` cells into the stream, the root into hp.d_root.  Windowed:
    only the permutations whose cells fall into this rank's columns are traced; the digests are computed everywhere."""
    with hp._window(sel, at, lookup=False):
        check(hp.lib.vdb_wit_merkle_dev(d_vectors, hp.n, hp.dim, 0, hp.d_stream.at(at * B), hp._sel_at(sel, at), hp.d_root.ptr))


class KmeansHotPath(HotPath):
    """kmeans::<K, I> over N x D vectors at 2^k rows: witness -> layout -> commit -> NTT, one GPU."""

    def __init__(self, n=256, dim=128, K=4, I=8, k=16, P=48, L=15, metric="euclidean", seed=20260004, tau=None,
                 col_shard=(0, 1), vectors=None, blind_seed=None, params=None):
        super().__init__(n, dim, k, P, L, seed=seed, tau=tau, col_shard=col_shard, vectors=vectors, blind_seed=blind_seed, params=params)
        self.K, self.I = K, I
        self.metric = api.METRICS[metric]
        self.metric_name = metric

    def _input_vectors(self):
        return sift_like_vectors(self.seed, self.n, self.dim, self.K)

    def _circuit_size(self):
        cells, lk = ctypes.c_uint64(), ctypes.c_uint64()
        check(self.lib.vdb_wit_kmeans_size(self.metric, self.P, self.L, self.n, self.dim, self.K, self.I, 0, ctypes.byref(cells), ctypes.byref(lk)))
        return self.n * self.dim, cells.value, lk.value

    def _alloc_outputs(self):
        self.d_cent = self._output(self.K * self.dim * 32)
        self.d_ind = self._output(self.n * self.K * 32)

    def _emit(self, sel):
        at = self.n_in
        with self._window(sel, at):
            check(self.lib.vdb_wit_kmeans_dev(self.metric, self.P, self.L, self.d_vec.ptr, self.n, self.dim, self.K, self.I, 0, self.d_stream.at(at * B),
                                              self.d_lookup.ptr, self._sel_at(sel, at), self.d_cent.ptr, self.d_ind.ptr))

    def public_values_dev(self):
        return self.d_cent.ptr, self.K * self.dim              # examples/kmeans.rs:51-56: every centroid, word by word

    def results(self):
        cent = self.d_cent.download((self.K, self.dim, 4))
        ind = self.d_ind.download((self.n, self.K, 4))
        return cent, ind

    def constraint_map(self, d_flags, on_device=True):
        # the unit blocks are traced on the host (a few thousand cells each); their hundreds of thousands of instances are placed
        # by the device (circuit_dev.py): the map's 10^9-cell arrays never exist on the host
        from . import circuit_sym as CS
        from .circuit_dev import DeviceBuilder
        cm, (cent, _ind) = CS.build_kmeans(self.metric_name, self.n, self.dim, self.K, self.I, self.P, self.L, builder=DeviceBuilder if on_device else None)
        return cm, np.asarray(cent).reshape(-1), None


class PoseidonHotPath(HotPath):
    """What the circuits made of Poseidon permutations alone share (the commitment, path updates, openings): no lookup cells, and every
    column is dense (Poseidon states), so equal column counts per rank are balanced already."""

    def __init__(self, *args, **kw):
        super().__init__(*args, **kw)
        self.balance_shards = False
        self.msm_window_bits = 14   # nearly every scalar is a full-width Poseidon state: 19 windows instead of 24

    def _load_tree(self, d_out, lp, levels):
        """The resident tree over the n database vectors (api.merkle_tree_build's layout, 2 lp digests) into d_out: `levels` a
        DeviceBuffer (copied), a (2 lp, 4) array (uploaded), or None: built from self.database_f64."""
        if isinstance(levels, api.DeviceBuffer):
            check(self.lib.vdb_memcpy_d2d(d_out.ptr, levels.ptr, ctypes.c_size_t(2 * lp * B)))
        elif levels is not None:
            levels = np.ascontiguousarray(levels, dtype=np.uint64)
            assert levels.shape == (2 * lp, 4), "the tree does not belong to this shape"
            d_out.upload(levels)
        else:
            assert self.database_f64.shape == (self.n, self.dim), "database rows do not match the circuit's shape"
            qdb = api.quantize(self.database_f64, self.P)
            d_db = api.DeviceBuffer(qdb.nbytes)
            try:
                d_db.upload(qdb)
                check(self.lib.vdb_merkle_tree_build_dev(d_db.ptr, self.n, self.dim, d_out.ptr))
                api.sync()
            finally:
                d_db.free()


class MerkleHotPath(PoseidonHotPath):
    """merkle_commitment over N x D vectors (src/gadget/vectordb.rs:165-223; examples/merkle.rs) through the same hot
    path: Poseidon trace on the GPU -> commit -> NTT.  A rank that holds a block of columns traces only the permutations whose
    cells fall into it (the sponge states and the tree's digests are computed by every rank, value only)."""

    def __init__(self, n=1024, dim=128, k=15, P=32, seed=20260003, tau=None, col_shard=(0, 1), vectors=None, blind_seed=None, params=None):
        super().__init__(n, dim, k, P, 8, seed=seed, tau=tau, col_shard=col_shard, vectors=vectors, blind_seed=blind_seed, params=params)

    def _input_vectors(self):
        return sift_like_vectors(self.seed, self.n, self.dim)

    def _circuit_size(self):
        return self.n * self.dim, _merkle_cells(self), 0      # the vectors are assigned first (tests/vectordb/mod.rs:253-262 chip_merkle)

    def _alloc_outputs(self):
        self.d_root = self._output(32)

    def _emit(self, sel):
        _merkle_trace(self, self.d_vec.ptr, self.n_in, sel)

    def public_values_dev(self):
        return self.d_root.ptr, 1                  # examples/merkle.rs:47

    def results(self):
        return self.d_root.download((4,))

    def constraint_map(self, d_flags, on_device=True):
        from . import circuit_sym as CS
        from .circuit_dev import DeviceBuilder
        cm, root = CS.build_merkle(self.n, self.dim, functools.partial(self._fetch_flags, d_flags), self._fetch, builder=DeviceBuilder if on_device else None)
        assert cm.n_cells == self.n_cells
        return cm, [root], root                    # examples/merkle.rs:47 make_public.push(root)


class UpdateHotPath(PoseidonHotPath):
    """Inserts and replacements proved against the committed root: a batch of m Merkle path updates in one proof (include/vdb.h
    vdb_wit_merkle_update).  The reference has no such gadget: this is the closure a user of its chips writes.  Assigned witnesses:
    the m new vectors, per update the old leaf, the index bits and the siblings; then per update the leaf hash of the new vector, both
    paths level by level (assert_bit, four selects, two node hashes), the index as inner_product(bits, 2^l), and the top of the old path
    tied to the top of the update before.  Public: [old root | idx, old leaf, new leaf per update | new root]; an insert shows as old
    leaf 0.  The tree stays on the device: `d_levels` holds it after the batch (`d_levels0` before it), and `levels=` starts a batch
    from the tree another batch left.  No lookup cells; sharded like MerkleHotPath.
    `kinds` makes updates deletes (the new leaf is the constant 0) and `grow` doubles the padded leaf count that many times before the
    first update (include/vdb.h vdb_wit_merkle_update_ops, vdb_merkle_tree_grow_dev): both are circuit shape, the public values keep
    their form — the old root is the root before the growth, a delete shows new leaf 0."""

    def __init__(self, n=1024, dim=128, m=8, k=15, L=8, P=32, seed=20260005, tau=None, col_shard=(0, 1), vectors=None, updates=None, levels=None,
                 blind_seed=None, params=None, kinds=None, grow=0):
        """`vectors`: the (n, dim) f64 database the tree is built from (None: seeded synthetic rows), or `levels`: a tree already on
        the device or host (api.merkle_tree_build's layout over n vectors, not yet grown; a DeviceBuffer or a (2 lp, 4) array).
        `updates`: (indices, (w, dim) f64 rows of the writes), applied in order (None: m seeded replacements and, where the padding has
        room, inserts).  `kinds`: per update 0 (write) or 1 (delete), None: all writes.  `lp` and `depth` are the grown tree's."""
        if m < 1:
            raise ValueError("a batch holds at least one update")
        self.kinds = np.zeros(m, dtype=np.uint8) if kinds is None else np.ascontiguousarray(kinds, dtype=np.uint8)
        if self.kinds.shape != (m,) or (self.kinds > 1).any() or grow < 0:
            raise ValueError("one kind (0 write, 1 delete) per update and a non-negative number of doublings")
        self.grow, self.w = int(grow), int((self.kinds == 0).sum())
        self.lp0, depth0 = api.merkle_levels(n)
        self.lp, self.depth = self.lp0 << self.grow, depth0 + self.grow
        if self.depth < 1:
            raise ValueError("a tree of one leaf has no path")
        if self.depth > 30:
            raise ValueError("a tree of at most 30 levels")
        super().__init__(n, dim, k, P, L, seed=seed, tau=tau, col_shard=col_shard, vectors=None, blind_seed=blind_seed, params=params)
        self.m = m
        self.database_f64 = None if vectors is None else np.ascontiguousarray(vectors, dtype=np.float64)
        self.given_levels, self.given_updates = levels, updates

    def n_input_rows(self):
        return self.w

    def _input_vectors(self):
        """the new vectors of the writes (the rows ctx.assign_witnesses puts first) and self.indices"""
        if self.given_updates is not None:
            idx, rows = self.given_updates
            rows = np.ascontiguousarray(rows, dtype=np.float64).reshape(-1, self.dim)
        else:
            rows, _ = sift_like_vectors(self.seed + 2000, self.m, self.dim)
            rows = rows[: self.w]
            rng = np.random.default_rng(self.seed)
            idx = rng.integers(0, self.n, size=self.m)
            free = min(self.lp - self.n, self.m // 2)
            if free:
                idx[self.m - free:] = self.n + np.arange(free)      # the batch ends with inserts into the padding
        self.indices = np.ascontiguousarray(idx, dtype=np.uint64)
        if self.indices.shape != (self.m,) or (self.indices >= self.lp).any():
            raise ValueError("an update needs an index below the padded leaf count for every new vector")
        return rows, self.seed

    def _load_inputs(self):
        super()._load_inputs()
        self.d_levels0 = self._output(2 * self.lp * B)
        self.d_levels = self._output(2 * self.lp * B)
        # the tree before the growth: straight into d_levels0 when it is not grown, else into d_levels, which every run overwrites
        d_small = self.d_levels if self.grow else self.d_levels0
        if self.given_levels is None and self.database_f64 is None:
            self.database_f64, _ = sift_like_vectors(self.seed, self.n, self.dim)
        self._load_tree(d_small, self.lp0, self.given_levels)
        if self.grow:
            check(self.lib.vdb_merkle_tree_grow_dev(d_small.ptr, self.n, self.grow, self.d_levels0.ptr))
            api.sync()

    def _circuit_size(self):
        cells, n_in = ctypes.c_uint64(), ctypes.c_uint64()
        check(self.lib.vdb_wit_merkle_update_ops_size(self.n, self.dim, self.m, api._p(self.kinds), self.grow, ctypes.byref(cells), ctypes.byref(n_in)))
        return n_in.value, cells.value - n_in.value, 0

    def _alloc_outputs(self):
        self.d_pub = self._output((3 * self.m + 2) * B)

    def _witness(self, sel=None):
        # the call writes the assigned witnesses too (old leaves and siblings come out of its value pass); every run starts from the
        # tree before the batch, so that the keygen-style runs and the proof state the same update
        check(self.lib.vdb_memcpy_d2d(self.d_levels.ptr, self.d_levels0.ptr, ctypes.c_size_t(2 * self.lp * B)))
        with self._window(sel, 0, lookup=False):
            check(self.lib.vdb_wit_merkle_update_ops_dev(self.d_levels.ptr, self.n, self.dim, self.grow, self.d_vec.ptr if self.w else None,
                                                         api._p(self.indices), api._p(self.kinds), self.m, self.d_stream.ptr, self._sel_at(sel, 0),
                                                         self.d_pub.ptr))

    def public_values_dev(self):
        return self.d_pub.ptr, 3 * self.m + 2

    def results(self):
        """(old root (4,), indices (m, 4), old leaves (m, 4), new leaves (m, 4), new root (4,))"""
        pub = self.d_pub.download((3 * self.m + 2, 4))
        per = pub[1:-1].reshape(self.m, 3, 4)
        return pub[0], per[:, 0], per[:, 1], per[:, 2], pub[-1]

    def constraint_map(self, d_flags, on_device=True):
        from . import circuit_sym as CS
        from .circuit_dev import DeviceBuilder
        cm, pub = CS.build_merkle_update(self.m, self.dim, self.depth, functools.partial(self._fetch_flags, d_flags), self._fetch,
                                         builder=DeviceBuilder if on_device else None, kinds=self.kinds.tolist(), grow=self.grow)
        assert cm.n_cells == self.n_cells
        return cm, pub, None


class ReadHotPath(PoseidonHotPath):
    """Reads proved against the committed root: m openings of the resident tree in one proof (include/vdb.h vdb_wit_merkle_open).  The
    reference has no such gadget: this is the closure a user of its chips writes.  reveal="vector": the m vectors read are assigned,
    hashed (merkle_commitment's leaf hash) and public, "slot i holds vector v"; reveal="leaf": the leaf digest is assigned and
    public, and a padding slot shows leaf 0, "slot i is empty".  Then per read the path level by level (assert_bit, two selects, one
    node hash), the index as inner_product(bits, 2^l), and the top of every read tied to the top of read 0.  Public: [root | idx, leaf
    per read | the vectors word by word (vector mode)].  Reads do not see each other and leave the tree (`d_levels`) as it is.  No
    lookup cells; sharded like MerkleHotPath."""

    def __init__(self, n=1024, dim=128, m=8, k=15, L=8, P=32, seed=20260006, tau=None, col_shard=(0, 1), vectors=None, levels=None, reads=None,
                 reveal="vector", blind_seed=None, params=None):
        """`vectors`: the current (n, dim) f64 database (None: seeded synthetic rows, when the tree is built here too); `levels`: the
        tree as it stands (api.merkle_tree_build's layout: a DeviceBuffer, for instance an UpdateHotPath's d_levels, or a (2 lp, 4)
        array; None: built from `vectors`).  `reads`: the m slots (None: m seeded slots, in leaf mode the last one a padding slot where
        the tree has one)"""
        if m < 1:
            raise ValueError("a call opens at least one slot")
        if reveal not in ("vector", "leaf"):
            raise ValueError("reveal is 'vector' or 'leaf'")
        self.lp, self.depth = api.merkle_levels(n)
        if self.depth < 1:
            raise ValueError("a tree of one leaf has no path")
        super().__init__(n, dim, k, P, L, seed=seed, tau=tau, col_shard=col_shard, vectors=None, blind_seed=blind_seed, params=params)
        self.m, self.with_vectors = m, reveal == "vector"
        self.database_f64 = None if vectors is None else np.ascontiguousarray(vectors, dtype=np.float64)
        if self.database_f64 is None and (levels is None or self.with_vectors):
            if levels is not None:
                raise ValueError("a read that reveals vectors needs the database the tree was built from")
            self.database_f64, _ = sift_like_vectors(self.seed, self.n, self.dim)
        if self.database_f64 is not None and self.database_f64.shape != (self.n, self.dim):
            raise ValueError("database rows do not match the circuit's shape")
        self.given_levels, self.given_reads = levels, reads

    def n_input_rows(self):
        return self.m if self.with_vectors else 0

    def _input_vectors(self):
        """the m rows read, gathered from the database (vector mode; none in leaf mode), and self.indices"""
        if self.given_reads is not None:
            idx = np.asarray(self.given_reads)
        else:
            idx = np.random.default_rng(self.seed).integers(0, self.n, size=self.m)
            if not self.with_vectors and self.lp > self.n:
                idx[-1] = self.n                                  # "this slot is empty"
        self.indices = np.ascontiguousarray(idx, dtype=np.uint64)
        if self.indices.shape != (self.m,) or (self.indices >= (self.n if self.with_vectors else self.lp)).any():
            raise ValueError("a read needs a slot that holds a vector (vector mode) or lies in the padded tree (leaf mode)")
        rows = self.database_f64[self.indices.astype(np.int64)] if self.with_vectors else np.zeros((0, self.dim))
        return rows, self.seed

    def _load_inputs(self):
        super()._load_inputs()
        self.d_levels = self._output(2 * self.lp * B)
        self._load_tree(self.d_levels, self.lp, self.given_levels)

    def _circuit_size(self):
        cells, n_in = ctypes.c_uint64(), ctypes.c_uint64()
        check(self.lib.vdb_wit_merkle_open_size(self.n, self.dim, self.m, int(self.with_vectors), ctypes.byref(cells), ctypes.byref(n_in)))
        return n_in.value, cells.value - n_in.value, 0

    def _alloc_outputs(self):
        self.n_pub = 1 + 2 * self.m + (self.m * self.dim if self.with_vectors else 0)
        self.d_pub = self._output(self.n_pub * B)

    def _witness(self, sel=None):
        # the call writes the assigned witnesses too (bits from the indices, siblings and leaves out of the tree)
        with self._window(sel, 0, lookup=False):
            check(self.lib.vdb_wit_merkle_open_dev(self.d_levels.ptr, self.n, self.dim, self.d_vec.ptr if self.with_vectors else None, api._p(self.indices),
                                                   self.m, self.d_stream.ptr, self._sel_at(sel, 0), self.d_pub.ptr))

    def public_values_dev(self):
        return self.d_pub.ptr, self.n_pub

    def results(self):
        """(root (4,), indices (m, 4), leaves (m, 4)[, vectors (m, dim, 4) in vector mode])"""
        pub = self.d_pub.download((self.n_pub, 4))
        per = pub[1:1 + 2 * self.m].reshape(self.m, 2, 4)
        out = (pub[0], per[:, 0], per[:, 1])
        return out + (pub[1 + 2 * self.m:].reshape(self.m, self.dim, 4),) if self.with_vectors else out

    def constraint_map(self, d_flags, on_device=True):
        from . import circuit_sym as CS
        from .circuit_dev import DeviceBuilder
        cm, pub = CS.build_merkle_open(self.m, self.dim, self.depth, self.with_vectors, functools.partial(self._fetch_flags, d_flags), self._fetch,
                                       builder=DeviceBuilder if on_device else None)
        assert cm.n_cells == self.n_cells
        return cm, pub, None


class TopKQueryHotPath(HotPath):
    """Top-k queries against ONE committed database in one proof: assign the q queries, assign the n database vectors, per query the
    `topk` rounds of include/vdb.h's vdb_wit_nearest_topk (nearest_vector's distances once, its qmin chain / is_equal /
    select_by_indicator per round, the winners replaced by Constant(2^(2P) - 1) through gate.select before the next round), then
    merkle_commitment(database) once.  The reference has no top-k gadget: this is the closure a user of its chips writes.  Stream:
    [queries | vectors | block of query 0 | ... | merkle_commitment]; the lookup cells are the queries' blocks in query order; public,
    in make_public order: per query the topk result vectors, nearest first, then the root (the queries stay private).  With topk = 1
    the circuit is BatchQueryHotPath's, with q = 1 too QueryHotPath's: those classes are this one at these values.  Ties are
    nearest_vector's: every vector at the round's minimum distance gets its indicator set, the round's result is the last of them and
    all of them leave together; when fewer than topk distinct distances exist, the later rounds set every indicator and return the
    last vector.  (PoseidonChip::new's three load_constant cells are not emitted, as in MerkleHotPath: the sponge's initial state is
    pinned as constants of the circuit.)  All blocks come from one call whose launch count depends on neither q nor topk.  Sharded
    (SURVEY §8e): every rank computes the distances' values and the short minimum chains (value-only walk), and stores the cells of
    its own block of columns only — the distance blocks, N-way parallel and nearly all of the cells, are skipped outside the rank's
    window."""

    commit = True        # merkle_commitment(database) follows in the same circuit, its root public (NearestHotPath: not)

    def __init__(self, topk=10, q=1, n=64, dim=128, k=16, P=48, L=13, metric="euclidean", seed=20260002, tau=None, col_shard=(0, 1), vectors=None,
                 blind_seed=None, params=None):
        """`vectors`: (q + n, dim) f64 rows, the queries first"""
        if q < 1:
            raise ValueError("a batch holds at least one query")
        if not 1 <= topk <= n:
            raise ValueError("topk must be at least 1 and at most n")
        super().__init__(n, dim, k, P, L, seed=seed, tau=tau, col_shard=col_shard, vectors=vectors, blind_seed=blind_seed, params=params)
        self.q, self.topk = q, topk
        self.n_results = q * topk * dim            # cells of the result vectors
        self.metric = api.METRICS[metric]
        self.metric_name = metric

    def n_input_rows(self):
        return self.q + self.n

    def _input_vectors(self):
        vec, seed = sift_like_vectors(self.seed, self.n, self.dim)
        queries, _ = sift_like_vectors(seed + 1000, self.q, self.dim)
        return np.concatenate([queries, vec]), seed

    def _circuit_size(self):
        cells, lk = ctypes.c_uint64(), ctypes.c_uint64()
        check(self.lib.vdb_wit_nearest_topk_size(self.metric, self.P, self.L, self.q, self.n, self.dim, self.topk, ctypes.byref(cells), ctypes.byref(lk)))
        self.nearest_cells, self.merkle_cells = cells.value, _merkle_cells(self) if self.commit else 0
        return (self.q + self.n) * self.dim, self.nearest_cells + self.merkle_cells, lk.value

    def _alloc_outputs(self):
        self.d_ind = self._output(self.q * self.topk * self.n * 32)
        # [result vectors | root]: the public statement, in make_public order (examples/query.rs:58 make_public.extend(result), :69 push(root))
        self.d_pub = self.d_res = self._output((self.n_results + self.commit) * 32)
        if self.commit:
            self.d_root = self._output(32)

    def _emit(self, sel):
        at, d_db = self.n_in, self.d_vec.at(self.q * self.dim * 32)
        with self._window(sel, at):
            check(self.lib.vdb_wit_nearest_topk_dev(self.metric, self.P, self.L, self.d_vec.ptr, d_db, self.q, self.n, self.dim, self.topk,
                                                    self.d_stream.at(at * B), self.d_lookup.ptr, self._sel_at(sel, at), self.d_ind.ptr, self.d_pub.ptr))
        if self.commit:
            _merkle_trace(self, d_db, at + self.nearest_cells, sel)
            check(self.lib.vdb_memcpy_d2d(self.d_pub.at(self.n_results * 32), self.d_root.ptr, ctypes.c_size_t(32)))

    def public_values_dev(self):
        return self.d_pub.ptr, self.n_results + self.commit

    def _result_axes(self):
        return self.q, self.topk

    def results(self):
        axes = self._result_axes()
        out = self.d_ind.download(axes + (self.n, 4)), self.d_pub.download(axes + (self.dim, 4))
        return out + (self.d_root.download((4,)),) if self.commit else out

    def constraint_map(self, d_flags, on_device=True):
        # the queries' blocks, then merkle_commitment over the same assigned vectors, in one map (examples/query.rs)
        from . import circuit_sym as CS
        from .circuit_dev import DeviceBuilder
        bld, (_ind, res), used = CS.build_nearest_topk(self.metric_name, self.q, self.n, self.dim, self.topk, self.P, self.L,
                                                       builder=DeviceBuilder if on_device else None, extra_cells=self.merkle_cells, finish=False)
        assert used == self.n_in + self.nearest_cells
        public, root = [int(c) for c in np.asarray(res).reshape(-1)], None
        if self.commit:
            root, end = CS.place_merkle(bld, self.n, self.dim, used, self.q * self.dim, functools.partial(self._fetch_flags, d_flags), self._fetch)
            assert end == self.n_cells
            public.append(root)
        return bld.finish(), public, root


class BatchQueryHotPath(TopKQueryHotPath):
    """A batch of queries against ONE committed database in one proof: the closure a user of the reference's chips writes for it —
    assign the q queries, assign the n database vectors, nearest_vector(query, database) per query (src/gadget/vectordb.rs:122-163),
    merkle_commitment(database) once (:165-223) — i.e. examples/query.rs:32-73 with its nearest_vector repeated, so that q queries pay
    for the database commitment once.  TopKQueryHotPath at topk = 1, its results without the round axis."""

    def __init__(self, q=8, n=64, dim=128, k=16, P=48, L=13, metric="euclidean", seed=20260002, tau=None, col_shard=(0, 1), vectors=None,
                 blind_seed=None, params=None):
        """`vectors`: (q + n, dim) f64 rows, the queries first"""
        super().__init__(1, q, n, dim, k, P, L, metric, seed, tau, col_shard, vectors, blind_seed, params)

    def _result_axes(self):
        return (self.q,)


class QueryHotPath(TopKQueryHotPath):
    """The reference's `query` circuit — "exhaustively find the similar vector & commit to the database" (examples/query.rs:32-73;
    tests/vectordb/mod.rs:220-247 chip_nearest_vector): nearest_vector(query, database) and merkle_commitment(database) in ONE
    circuit over the same assigned vectors, the result vector and the Merkle root public.  TopKQueryHotPath at q = topk = 1, its
    results without the query and round axes."""

    def __init__(self, n=64, dim=128, k=14, P=48, L=13, metric="euclidean", seed=20260002, tau=None, col_shard=(0, 1), vectors=None, blind_seed=None,
                 params=None):
        """`vectors`: (n + 1, dim) f64 rows, the query first"""
        super().__init__(1, 1, n, dim, k, P, L, metric, seed, tau, col_shard, vectors, blind_seed, params)

    def _result_axes(self):
        return ()


class NearestHotPath(QueryHotPath):
    """nearest_vector(query, vectors) alone (src/gadget/vectordb.rs:122-163; tests/vectordb/mod.rs:220-247 assigns the query, then the
    vectors): QueryHotPath without the commitment, the result vector public (examples/query.rs:58)."""

    commit = False


class DistancesHotPath(HotPath):
    """The reference's two-vector circuits through the same hot path: examples/distances.rs:29-59 (assign a, assign b, then
    euclidean, manhattan, cosine and hamming distance of the same two vectors, each made public) and examples/euclid.rs:26-46 (ten Euclidean distances of one pair, nothing public:
    `metrics=("euclidean",) * 10, public=False`).  BASELINE configs[0] is this circuit with one Euclidean distance of two 4-dim
    vectors at k = 13, LOOKUP_BITS = 12.  Stream: [a | b | the cells of each distance in turn]; every rank emits every cell (a few
    columns: nothing to shard the witness by)."""

    def __init__(self, dim=4, metrics=("euclidean", "manhattan", "cosine", "hamming"), k=13, P=48, L=12, seed=20260001, tau=None, col_shard=(0, 1), vectors=None,
                 blind_seed=None, public=True, params=None):
        """`vectors`: (2, dim) f64 rows, a then b"""
        for m in metrics:
            if m not in api.METRICS:
                raise ValueError("unknown distance: " + str(m))
        super().__init__(2, dim, k, P, L, seed=seed, tau=tau, col_shard=col_shard, vectors=vectors, blind_seed=blind_seed, params=params)
        self.metrics = tuple(metrics)
        self.public = bool(public)
        self.shard_witness = False

    def _input_vectors(self):
        return sift_like_vectors(self.seed, 2, self.dim)

    def _circuit_size(self):
        self.parts, cells, lk = _end_to_end([api.METRICS[m] for m in self.metrics],
                                            lambda code, cells, lk: self.lib.vdb_wit_distance_size(code, self.P, self.L, 1, self.dim, cells, lk))
        return 2 * self.dim, cells, lk

    def _alloc_outputs(self):
        self.d_res = self._output(len(self.metrics) * 32)

    def _emit(self, sel):
        for i, (metric, off, lk_off) in enumerate(self.parts):
            at = self.n_in + off
            check(self.lib.vdb_wit_distance_dev(metric, self.P, self.L, self.d_vec.ptr, self.d_vec.at(self.dim * 32), 1, self.dim, self.d_stream.at(at * B),
                                                self.d_lookup.at(lk_off * B), self._sel_at(sel, at), self.d_res.at(i * 32)))

    def public_values_dev(self):
        return self.d_res.ptr, len(self.metrics) if self.public else 0      # examples/distances.rs:44-59: make_public.push(dist) after each

    def results(self):
        return self.d_res.download((len(self.metrics), 4))

    def constraint_map(self, d_flags, on_device=True):
        # two vectors, a handful of distances: the whole trace on the host (examples/distances.rs, examples/euclid.rs)
        from . import circuit_sym as CS
        cm, outs = CS.trace_distances(self.metrics, self.dim, self.P, self.L)
        return cm, outs if self.public else [], None      # examples/distances.rs:44-59 make_public.push(dist)


class FixedPointHotPath(HotPath):
    """examples/fixed_point.rs:38-112 through the hot path: FixedPointChip<32> on ONE value — x = ctx.load_witness(quantization(x)), then
    qexp2(x), qlog2(x) when x > 0, qsin(x), with x and every result public.  Stream: [x | the cells of each call in turn]
    (vdb_wit_fp_op_dev, one instance each).  `ops`: other unary FixedPointInstructions names instead of the example's."""

    def __init__(self, x=1.128, ops=None, k=13, P=32, L=12, tau=None, blind_seed=None, params=None):
        self.x = float(x)
        self.ops = tuple(ops) if ops is not None else ("qexp2",) + (("qlog2",) if self.x > 0.0 else ()) + ("qsin",)
        for name in self.ops:
            if name not in FP_UNARY_OPS:
                raise ValueError("not a unary FixedPointChip operation: " + str(name))
        super().__init__(1, 1, k, P, L, tau=tau, blind_seed=blind_seed, params=params)
        self.shard_witness = False

    def _input_vectors(self):
        return np.array([[self.x]], dtype=np.float64), None

    def _circuit_size(self):
        self.parts, cells, lk = _end_to_end([api.FP_OPS[name] for name in self.ops],
                                            lambda code, cells, lk: self.lib.vdb_wit_fp_op_size(code, self.P, self.L, 1, cells, lk))
        return 1, cells, lk

    def _alloc_outputs(self):
        self.d_res = self._output((1 + len(self.ops)) * 32)        # [x | results]: the public statement in make_public order

    def _emit(self, sel):
        check(self.lib.vdb_memcpy_d2d(self.d_res.ptr, self.d_vec.ptr, ctypes.c_size_t(32)))
        for i, (op, off, lk_off) in enumerate(self.parts):
            at = 1 + off
            check(self.lib.vdb_wit_fp_op_dev(op, self.P, self.L, self.d_vec.ptr, None, 1, self.d_stream.at(at * B), self.d_lookup.at(lk_off * B),
                                             self._sel_at(sel, at), self.d_res.at((1 + i) * 32)))

    def public_values_dev(self):
        return self.d_res.ptr, 1 + len(self.ops)           # examples/fixed_point.rs:64, :79, :94, :110: make_public.push after each

    def results(self):
        return self.d_res.download((1 + len(self.ops), 4))[1:]

    def constraint_map(self, d_flags, on_device=True):
        # one value, a handful of FixedPointChip calls (examples/fixed_point.rs): x and every result public
        from . import circuit_sym as CS
        cm, outs = CS.trace_fixed_point(self.ops, self.P, self.L)
        return cm, outs, None


class AnnIndex:
    """The committed index of approximate-nearest-neighbour queries, resident on the device (include/vdb.h vdb_ann_index_build_dev): the
    rows grouped by cluster, the forest of the K cluster trees and the centroids' tree, and the K + 2 root digests.  `vectors`: (n, dim)
    f64, or the (n, dim, 4) quantized rows; `cluster_ids`: (n,) integers, or KmeansHotPath.results()'s (n, K, 4) indicators; `centroids`: (K, dim) f64, or the (K, dim, 4)
    quantized centroids KmeansHotPath.results() returns."""

    def __init__(self, n, dim, K, vectors, cluster_ids, centroids, P=48, L=13, metric="euclidean"):
        self.lib = api.init()
        self.n, self.dim, self.K, self.P, self.L, self.metric_name = n, dim, K, P, L, metric
        ids = np.asarray(cluster_ids)
        if ids.ndim == 3:
            ids = np.argmax(ids.any(axis=2), axis=1)
        self.cluster_ids = np.ascontiguousarray(ids, dtype=np.uint32)
        cent = np.asarray(centroids)
        self.qcent = np.ascontiguousarray(cent, dtype=np.uint64) if cent.ndim == 3 else api.quantize(np.ascontiguousarray(cent, dtype=np.float64), P)
        vec = np.asarray(vectors)
        self.qvec = np.ascontiguousarray(vec, dtype=np.uint64) if vec.ndim == 3 else api.quantize(np.ascontiguousarray(vec, dtype=np.float64), P)
        if self.qvec.shape != (n, dim, 4) or self.qcent.shape != (K, dim, 4) or self.cluster_ids.shape != (n,):
            raise ValueError("vectors, cluster ids and centroids do not match (n, dim, K)")
        self.n_digests, self.segments = api.ann_forest_layout(self.cluster_ids, K)     # refuses an empty cluster, an id >= K, K = 0
        self.sizes = np.bincount(self.cluster_ids, minlength=K).astype(np.int64)
        self.offsets = np.concatenate([[0], np.cumsum(self.sizes)]).astype(np.int64)
        self._bufs = []
        self.d_vec, self.d_cent = self._buf(self.qvec.nbytes), self._buf(self.qcent.nbytes)
        self.d_grouped, self.d_slots, self.d_offsets = self._buf(self.qvec.nbytes), self._buf(n * 4), self._buf((K + 1) * 8)
        self.d_forest, self.d_roots = self._buf(self.n_digests * B), self._buf((K + 2) * B)
        self.d_vec.upload(self.qvec)
        self.d_cent.upload(self.qcent)
        check(self.lib.vdb_ann_index_build_dev(self.d_vec.ptr, api._p(self.cluster_ids), self.d_cent.ptr, n, K, dim, self.d_grouped.ptr, self.d_slots.ptr,
                                               self.d_offsets.ptr, self.d_forest.ptr, self.d_roots.ptr))

    @classmethod
    def from_resident(cls, dim, K, sizes, n_digests, segments, qcent, qvec, cluster_ids, P=48, L=13, metric="euclidean"):
        """an index over buffers that are filled on the device (vdb_ann_index_apply_dev) instead of built here: the host-side shape
        (`sizes` of the K clusters, the forest's `n_digests` and `segments`), the quantized centroids and database, and fresh device
        buffers of that shape, which the caller fills; d_vec is not kept resident"""
        ix = cls.__new__(cls)
        ix.lib = api.init()
        ix.sizes = np.ascontiguousarray(sizes, dtype=np.int64)
        ix.n, ix.dim, ix.K, ix.P, ix.L, ix.metric_name = int(ix.sizes.sum()), dim, K, P, L, metric
        ix.cluster_ids, ix.qcent, ix.qvec = np.ascontiguousarray(cluster_ids, dtype=np.uint32), qcent, qvec
        ix.n_digests, ix.segments = int(n_digests), np.ascontiguousarray(segments, dtype=np.uint64)
        ix.offsets = np.concatenate([[0], np.cumsum(ix.sizes)]).astype(np.int64)
        ix._bufs = []
        ix.d_vec, ix.d_cent = None, ix._buf(qcent.nbytes)
        ix.d_grouped, ix.d_slots, ix.d_offsets = ix._buf(ix.n * dim * B), ix._buf(ix.n * 4), ix._buf((K + 1) * 8)
        ix.d_forest, ix.d_roots = ix._buf(ix.n_digests * B), ix._buf((K + 2) * B)
        ix.d_cent.upload(qcent)
        return ix

    def _after_writes(self, hp, db_slots):
        """the shape and the host view of the index after the writes of `hp` (AnnUpdateHotPath or AnnWriteHotPath) with its appends at
        the database slots `db_slots`: replaced rows where the cluster's slots say, appended rows at db_slots -> (sizes before the batch
        as uint64, the new AnnIndex on fresh, unfilled buffers)"""
        c, m, app = hp.cluster, hp.m, hp.appends
        if db_slots.shape != (app,):
            raise ValueError("one database slot per append")
        sizes64 = np.ascontiguousarray(self.sizes, dtype=np.uint64)
        _, digests, seg = api.ann_index_apply_layout(sizes64, c, hp.grow, hp.indices)
        old_slots = self.d_slots.download((int(self.sizes[c]),), dtype=np.uint32, offset=int(self.offsets[c]) * 4)
        place = np.concatenate([old_slots, db_slots]).astype(np.int64)
        n2 = max(self.n, int(place.max()) + 1)
        qvec, ids = np.zeros((n2, self.dim, 4), dtype=np.uint64), np.zeros(n2, dtype=np.uint32)
        qvec[:self.n], ids[:self.n] = self.qvec, self.cluster_ids
        for j in range(m):
            qvec[place[int(hp.indices[j])]], ids[place[int(hp.indices[j])]] = hp.qvec[j], c
        sizes = self.sizes.copy()
        sizes[c] += app
        return sizes64, AnnIndex.from_resident(self.dim, self.K, sizes, digests, seg, self.qcent, qvec, ids, P=self.P, L=self.L, metric=self.metric_name)

    def updated(self, hp, db_slots=None):
        """the index after the batch of AnnUpdateHotPath `hp` (its witness has run: hp.d_levels holds the cluster's tree after the
        batch), as a new AnnIndex on buffers of its own (vdb_ann_index_apply_dev); this index stays valid.  `db_slots`: the database slot
        of every append, in append order (None: n, n + 1, ..., which keeps the members in database order).  Queries, reads and further
        updates run on the result unchanged."""
        c, m, app = hp.cluster, hp.m, hp.appends
        db_slots = np.arange(self.n, self.n + app, dtype=np.uint32) if db_slots is None else np.ascontiguousarray(db_slots, dtype=np.uint32)
        sizes64, ix = self._after_writes(hp, db_slots)
        try:
            check(self.lib.vdb_ann_index_apply_dev(self.d_grouped.ptr, self.d_slots.ptr, self.d_forest.ptr, self.d_roots.ptr, api._p(sizes64), self.K, self.dim,
                                                   c, hp.grow, hp.d_levels.ptr, hp.d_vec.ptr, api._p(hp.indices), api._p(db_slots) if app else None, m,
                                                   ix.d_grouped.ptr, ix.d_slots.ptr, ix.d_offsets.ptr, ix.d_forest.ptr, ix.d_roots.ptr))
        except Exception:
            ix.free()
            raise
        return ix

    def written(self, hp):
        """the index after the linked write of AnnWriteHotPath `hp` (its witness has run: hp.d_levels and hp.d_levels_db hold the two
        trees after the batch), as a new AnnIndex on buffers of its own (vdb_ann_index_write_dev); this index stays valid.  The appends
        take the database slots n, n + 1, ...; the host view is updated()'s.  The result's database tree is the one the proof wrote:
        written(hp).database_tree() costs nothing and refuses nothing.  ValueError for a hot path built on another index or with one of
        AnnWriteHotPath's overrides (levels, levels_db, db_indices): its trees are not this index's."""
        if hp.index is not self or hp.given_levels is not None or hp.given_levels_db is not None or hp.given_db_indices is not None:
            raise ValueError("the hot path was built on this index, with the index's own trees and database slots")
        sizes64, ix = self._after_writes(hp, np.arange(self.n, self.n + hp.appends, dtype=np.uint32))
        try:
            ix.d_db_tree = ix._buf(2 * hp.lp_db * B)
            check(self.lib.vdb_ann_index_write_dev(self.d_grouped.ptr, self.d_slots.ptr, self.d_forest.ptr, self.d_roots.ptr, api._p(sizes64), self.K, self.dim,
                                                   hp.cluster, hp.grow, hp.grow_db, hp.d_levels.ptr, hp.d_levels_db.ptr, hp.d_vec.ptr, api._p(hp.indices), hp.m,
                                                   ix.d_grouped.ptr, ix.d_slots.ptr, ix.d_offsets.ptr, ix.d_forest.ptr, ix.d_roots.ptr, ix.d_db_tree.ptr))
        except Exception:
            ix.free()
            raise
        return ix

    def removed(self, hp):
        """the index after the batch of AnnDeleteHotPath `hp` (its witness has run: hp.d_levels holds the cluster's tree after the
        batch), as a new AnnIndex on buffers of its own (vdb_ann_index_remove_dev); this index stays valid.  A removal compacts the
        database: the result's host view (qvec, cluster_ids) is its own grouped rows in order, database slot = grouped place.  Queries,
        reads, updates and further deletes run on the result unchanged."""
        c, m = hp.cluster, hp.m
        sizes64 = np.ascontiguousarray(self.sizes, dtype=np.uint64)
        _, digests, seg = api.ann_index_remove_layout(sizes64, c, hp.slots)
        sizes = self.sizes.copy()
        sizes[c] -= m
        # the host's view: the grouped rows before the batch, cluster c's rearranged as the batch leaves them (hp.origin)
        old_slots = self.d_slots.download((self.n,), dtype=np.uint32).astype(np.int64)
        lo = int(self.offsets[c])
        keep = np.concatenate([np.arange(lo), lo + np.asarray(hp.origin, dtype=np.int64), np.arange(lo + int(self.sizes[c]), self.n)]).astype(np.int64)
        qvec = np.ascontiguousarray(self.qvec[old_slots[keep]])
        ids = np.repeat(np.arange(self.K, dtype=np.uint32), sizes)
        ix = AnnIndex.from_resident(self.dim, self.K, sizes, digests, seg, self.qcent, qvec, ids, P=self.P, L=self.L, metric=self.metric_name)
        try:
            check(self.lib.vdb_ann_index_remove_dev(self.d_grouped.ptr, self.d_forest.ptr, self.d_roots.ptr, api._p(sizes64), self.K, self.dim, c,
                                                    hp.d_levels.ptr, api._p(hp.slots), m, ix.d_grouped.ptr, ix.d_slots.ptr, ix.d_offsets.ptr,
                                                    ix.d_forest.ptr, ix.d_roots.ptr))
        except Exception:
            ix.free()
            raise
        return ix

    def moved(self, hp):
        """the index after the batch of AnnMoveHotPath `hp` (its witness has run: hp.d_levels_a and hp.d_levels_b hold the two trees
        after the batch), as a new AnnIndex on buffers of its own (vdb_ann_index_move_dev); this index stays valid.  The database is not
        renumbered: the result's host view is the same qvec with the moved rows' cluster_ids set to b, and its database tree is this
        index's bit for bit.  Queries, reads, updates, deletes, audits and further moves run on the result unchanged."""
        a, b, m = hp.src, hp.dst, hp.m
        sizes64 = np.ascontiguousarray(self.sizes, dtype=np.uint64)
        _, g, digests, seg = api.ann_index_move_layout(sizes64, a, b, hp.slots)
        sizes = self.sizes.copy()
        sizes[a] -= m
        sizes[b] += m
        old_slots = self.d_slots.download((int(self.sizes[a]),), dtype=np.uint32, offset=int(self.offsets[a]) * 4).astype(np.int64)
        ids = self.cluster_ids.copy()
        ids[old_slots[np.asarray(hp.moved_from, dtype=np.int64)]] = b
        ix = AnnIndex.from_resident(self.dim, self.K, sizes, digests, seg, self.qcent, self.qvec, ids, P=self.P, L=self.L, metric=self.metric_name)
        try:
            check(self.lib.vdb_ann_index_move_dev(self.d_grouped.ptr, self.d_slots.ptr, self.d_forest.ptr, self.d_roots.ptr, api._p(sizes64), self.K, self.dim,
                                                  a, b, g, hp.d_levels_a.ptr, hp.d_levels_b.ptr, api._p(hp.slots), m, ix.d_grouped.ptr, ix.d_slots.ptr,
                                                  ix.d_offsets.ptr, ix.d_forest.ptr, ix.d_roots.ptr))
        except Exception:
            ix.free()
            raise
        return ix

    def _buf(self, nbytes):
        b = api.DeviceBuffer(max(int(nbytes), 32))
        self._bufs.append(b)
        return b

    def roots(self):
        """(K + 2, 4): [centroids' root | cluster roots | index root]"""
        return self.d_roots.download((self.K + 2, 4))

    def levels_ptr(self, c):
        """device pointer of segment c of the forest (c = K: the centroids' tree)"""
        return self.d_forest.at(int(self.segments[c]) * B)

    def levels(self, c):
        """cluster c's tree as a `levels=` of ReadHotPath / UpdateHotPath over its sizes[c] members: a view of the 2 lp_c digests of
        segment c where the forest holds them (the hot path copies them device to device); .download((2 lp_c, 4)) brings them to the host"""
        lo, hi = int(self.segments[c]), int(self.segments[c + 1])
        return api.DeviceView(self.d_forest, lo * B, (hi - lo) * B)

    def members_ptr(self, c):
        return self.d_grouped.at(int(self.offsets[c]) * self.dim * B)

    def members(self, c):
        return self.d_grouped.download((int(self.sizes[c]), self.dim, 4), offset=int(self.offsets[c]) * self.dim * B)

    def probe(self, query):
        """the id of the centroid nearest to `query` ((dim,) f64): nearest_vector's indicator (the last centroid at the minimum)"""
        q = api.quantize(np.ascontiguousarray(query, dtype=np.float64).reshape(1, self.dim), self.P)[0]
        ind = api.wit_nearest(self.metric_name, q, self.qcent, self.P, self.L)["indicator"]
        return int(np.flatnonzero(ind.any(axis=1))[-1])

    def probe_many(self, query, p):
        """the clusters p rounds of top-k over the centroids state for `query` ((dim,) f64), in round order, (p,) int64: round r's entry
        is the last centroid at the minimum of what the earlier rounds left — probe's rule round by round, so probe_many(q, 1)[0] ==
        probe(q) — in one values-only call against the resident centroids (vdb_nearest_topk_values_dev).  Centroids at equal distance
        leave in one round, which states the last of them: with fewer than p distance classes the entries are not pairwise distinct."""
        d_q, d_idx = api.DeviceBuffer(self.dim * B), api.DeviceBuffer(max(int(p), 1) * 4)
        try:
            d_q.upload(api.quantize(np.ascontiguousarray(query, dtype=np.float64).reshape(1, self.dim), self.P))
            check(self.lib.vdb_nearest_topk_values_dev(self.P, self.L, api.METRICS[self.metric_name], d_q.ptr, self.d_cent.ptr, 1, self.K, self.dim, int(p),
                                                       d_idx.ptr, None))
            return d_idx.download((int(p),), dtype=np.uint32).astype(np.int64)
        finally:
            d_q.free()
            d_idx.free()

    def assign(self, rows, distances=False):
        """the cluster of every row of `rows` ((m, dim) f64): probe's answer for each — the last centroid at the minimum of the
        circuit's fixed-point distance — in one values-only call against the resident centroids (vdb_nearest_values_dev: nothing is
        emitted, the centroids are not uploaded).  (m,) int64; with `distances` also the (m, 4) minimum distances."""
        rows = np.ascontiguousarray(rows, dtype=np.float64).reshape(-1, self.dim)
        m = rows.shape[0]
        if m == 0:
            return (np.zeros(0, dtype=np.int64), np.zeros((0, 4), dtype=np.uint64)) if distances else np.zeros(0, dtype=np.int64)
        d_rows, d_idx, d_dist = api.DeviceBuffer(m * self.dim * B), api.DeviceBuffer(m * 4), api.DeviceBuffer(m * B)
        try:
            d_rows.upload(api.quantize(rows, self.P))
            check(self.lib.vdb_nearest_values_dev(self.P, self.L, api.METRICS[self.metric_name], d_rows.ptr, self.d_cent.ptr, m, self.K, self.dim,
                                                  d_idx.ptr, d_dist.ptr))
            idx = d_idx.download((m,), dtype=np.uint32).astype(np.int64)
            return (idx, d_dist.download((m, 4))) if distances else idx
        finally:
            for b in (d_rows, d_idx, d_dist):
                b.free()

    def means(self):
        """(K, dim, 4): the mean of every cluster's members in the circuit's fixed-point arithmetic, qdiv(sum of the members' words,
        quantization(n_k)), in one values-only call over the resident grouped rows (vdb_ann_cluster_means_dev: nothing is emitted or
        uploaded) — bit for bit the centroid AnnMeanHotPath accepts for the cluster"""
        d = api.DeviceBuffer(self.K * self.dim * B)
        try:
            check(self.lib.vdb_ann_cluster_means_dev(self.P, self.L, self.d_grouped.ptr, self.d_offsets.ptr, self.n, self.K, self.dim, d.ptr))
            return d.download((self.K, self.dim, 4))
        finally:
            d.free()

    def recentred(self):
        """a new AnnIndex over the same rows and cluster ids whose centroids are means(): built from scratch by the index build, on
        buffers of its own; this index stays valid.  After writes and deletes have moved the members, the mean audit of every cluster
        of the result is clean.  This call proves nothing; that the result's root descends from this index's is proved one centroid at a
        time: K proofs of AnnRecentreHotPath, c = 0 .. K - 1, each on recentred_with of the one before, move this index's root to the
        result's root bit for bit."""
        if self.qvec.shape[0] != self.n:
            raise ValueError("the database has slots no cluster holds: recentre an index whose rows are dense")
        return AnnIndex(self.n, self.dim, self.K, self.qvec, self.cluster_ids, self.means(), P=self.P, L=self.L, metric=self.metric_name)

    def recentred_with(self, hp):
        """the index after the recentre of AnnRecentreHotPath `hp` (its witness has run: hp.d_levels holds the centroids' tree after the
        write, hp.d_new the new centroid), as a new AnnIndex on buffers of its own (vdb_ann_index_recentre_dev: copies and one sponge, no
        rebuild); this index stays valid.  Its index root is the proof's index_root_new."""
        if hp.index is not self:
            raise ValueError("the proof is of another index")
        c, sizes64 = hp.cluster, np.ascontiguousarray(self.sizes, dtype=np.uint64)
        qcent = self.qcent.copy()
        qcent[c] = hp.d_new.download((self.dim, 4))
        ix = AnnIndex.from_resident(self.dim, self.K, self.sizes, self.n_digests, self.segments, qcent, self.qvec, self.cluster_ids, P=self.P, L=self.L,
                                    metric=self.metric_name)
        try:
            check(self.lib.vdb_ann_index_recentre_dev(self.d_grouped.ptr, self.d_slots.ptr, self.d_offsets.ptr, self.d_forest.ptr, self.d_roots.ptr,
                                                      self.d_cent.ptr, api._p(sizes64), self.K, self.dim, c,
                                                      hp.d_levels.ptr, hp.d_new.ptr, ix.d_grouped.ptr, ix.d_slots.ptr, ix.d_offsets.ptr, ix.d_forest.ptr,
                                                      ix.d_roots.ptr, ix.d_cent.ptr))
        except Exception:
            ix.free()
            raise
        return ix

    def database_tree(self):
        """the merkle_commitment tree over the database rows in slot order (2 lp digests, api.merkle_tree_build's layout) as a device
        buffer this index owns, made once (vdb_ann_index_db_tree_dev): every leaf digest is copied from the forest to its row's slot,
        no vector is hashed again.  Its root is the root QueryHotPath / MerkleHotPath publish for the same rows, and the database_root
        of AnnCoverHotPath.  An index whose slots are no permutation of 0 .. n - 1 (a database with slots no cluster holds) is refused."""
        if getattr(self, "d_db_tree", None) is None:
            lp, _ = api.merkle_levels(self.n)
            buf = api.DeviceBuffer(2 * lp * B)
            try:
                check(self.lib.vdb_ann_index_db_tree_dev(self.d_forest.ptr, api._p(np.ascontiguousarray(self.sizes, dtype=np.uint64)), self.d_slots.ptr, self.K,
                                                         self.n, buf.ptr))
            except Exception:
                buf.free()
                raise
            self._bufs.append(buf)
            self.d_db_tree = buf
        return self.d_db_tree

    def free(self):
        for b in self._bufs:
            b.free()
        self._bufs = []
        self.d_db_tree = None


def _bind_cluster(hp, index, cluster):
    """binds hot path `hp` to cluster c of the index -> n_c"""
    hp.index, hp.K, hp.cluster = index, index.K, int(cluster)
    if not 0 <= hp.cluster < hp.K:
        raise ValueError("cluster outside the index")
    return int(index.sizes[hp.cluster])


def _given_ptr(hp, given, shape, resident_ptr):
    """where a call reads what the index holds: `resident_ptr`, or the quantized override `given`, uploaded"""
    if given is None:
        return resident_ptr
    a = np.ascontiguousarray(given, dtype=np.uint64)
    assert a.shape == shape
    d = hp._output(a.nbytes)
    d.upload(a)
    return d.ptr


class AnnProbeQueryHotPath(HotPath):
    """The approximate-nearest-neighbour query with the two knobs of an IVF-style index, in ONE proof (include/vdb.h vdb_wit_ann_probe):
    the `topk` nearest candidates over the members of the `probes` clusters whose centroids `probes` rounds of top-k over the committed
    centroids state.  Assigned: the query, the centroids, the candidates (the probed clusters' members end to end in round order), the
    K cluster roots; then nearest_topk(query, centroids, probes), merkle_commitment(centroids), nearest_topk(query, candidates, topk),
    one merkle_commitment per probed cluster, one select_by_indicator(cluster roots, centroid indicators of round r) per round, tied
    to that cluster's root, and the sponge over [centroids' root | cluster roots].  Public: the topk results nearest first, then the
    index root; the query, the clusters probed and their sizes stay private (the sizes shape the proving key).  Not proved: that no
    vector outside the probed clusters is nearer — that is what approximate means here.  `clusters`: the clusters probed, in round
    order (None: index.probe_many(query, probes)); a list other than the rounds' breaks a copy constraint.  Centroids at equal distance
    leave in one round, which states the last of them: a query with fewer than `probes` distance classes among the centroids probes
    some cluster twice and is refused (ValueError).  `cluster_roots` / `centroids`: quantized overrides of what the index holds (tests
    of the binding); with them the trees are hashed by the call instead of read from the forest."""

    def __init__(self, index, query, probes=1, topk=1, clusters=None, k=13, P=48, L=12, metric="euclidean", tau=None, col_shard=(0, 1), blind_seed=None,
                 params=None, cluster_roots=None, centroids=None):
        query = np.ascontiguousarray(query, dtype=np.float64).reshape(1, index.dim)
        self.index, self.K, self.probes, self.topk = index, index.K, int(probes), int(topk)
        if not 1 <= self.probes <= self.K:
            raise ValueError("probes: at least 1 and at most K")
        self.clusters = [int(c) for c in (index.probe_many(query[0], self.probes) if clusters is None else clusters)]
        if len(self.clusters) != self.probes or not all(0 <= c < self.K for c in self.clusters):
            raise ValueError("one cluster of the index per probe")
        if len(set(self.clusters)) != self.probes:
            raise ValueError("the clusters probed are not pairwise distinct: fewer than `probes` distance classes among the centroids")
        self.sizes = np.ascontiguousarray([index.sizes[c] for c in self.clusters], dtype=np.uint64)
        self.cand_offsets = np.concatenate([[0], np.cumsum(self.sizes.astype(np.int64))])
        super().__init__(int(self.sizes.sum()), index.dim, k, P, L, seed=None, tau=tau, col_shard=col_shard, vectors=query, blind_seed=blind_seed,
                         params=params)
        self.metric, self.metric_name = api.METRICS[metric], metric
        self.given_roots, self.given_cent = cluster_roots, centroids

    def n_input_rows(self):
        return 1

    def _load_inputs(self):
        super()._load_inputs()
        ix, self.resident = self.index, self.given_roots is None and self.given_cent is None
        self.p_roots = _given_ptr(self, self.given_roots, (self.K, 4), ix.d_roots.at(B))
        self.p_cent = _given_ptr(self, self.given_cent, (self.K, self.dim, 4), ix.d_cent.ptr)
        as_ptrs = lambda ptrs: (ctypes.c_void_p * self.probes)(*[p.value for p in ptrs])
        self.p_members = as_ptrs([ix.members_ptr(c) for c in self.clusters])
        self.p_levels = as_ptrs([ix.levels_ptr(c) for c in self.clusters]) if self.resident else None

    def _circuit_size(self):
        cells, lk, n_in = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
        check(self.lib.vdb_wit_ann_probe_size(self.metric, self.P, self.L, self.K, self.dim, self.probes, api._p(self.sizes), self.topk, ctypes.byref(cells),
                                              ctypes.byref(lk), ctypes.byref(n_in)))
        return n_in.value, cells.value - n_in.value, lk.value

    def _alloc_outputs(self):
        self.d_ind_c, self.d_ind_m = self._output(self.probes * self.K * B), self._output(self.topk * self.n * B)
        self.d_pub = self._output((self.topk * self.dim + 1) * B)

    def _witness(self, sel=None):
        # the call writes the assigned witnesses too (centroids, candidates and roots where the index holds them)
        ix = self.index
        with self._window(sel, 0):
            check(self.lib.vdb_wit_ann_probe_dev(self.metric, self.P, self.L, self.d_vec.ptr, self.p_cent, self.p_members, self.p_roots,
                                                 ix.levels_ptr(self.K) if self.resident else None, self.p_levels, self.K, self.dim, self.probes,
                                                 api._p(self.sizes), self.topk, self.d_stream.ptr, self.d_lookup.ptr, self._sel_at(sel, 0),
                                                 self.d_ind_c.ptr, self.d_ind_m.ptr, self.d_pub.ptr))

    def public_values_dev(self):
        return self.d_pub.ptr, self.topk * self.dim + 1

    def results(self):
        """(centroid indicators (p, K, 4), candidate indicators (t, N, 4), results (t, dim, 4) nearest first, index root (4,))"""
        t, pub = self.topk, self.d_pub.download((self.topk * self.dim + 1, 4))
        return (self.d_ind_c.download((self.probes, self.K, 4)), self.d_ind_m.download((t, self.n, 4)), pub[:t * self.dim].reshape(t, self.dim, 4),
                pub[t * self.dim])

    def neighbours(self):
        """(t,) int64: the database slots of the results, nearest first — the last set indicator of every round of the candidate
        search, through the candidates' place in their cluster's grouped rows, to index.d_slots"""
        ind = self.d_ind_m.download((self.topk, self.n, 4)).any(axis=2)
        cand = np.asarray([int(np.flatnonzero(row)[-1]) for row in ind], dtype=np.int64)
        r = np.searchsorted(self.cand_offsets, cand, side="right") - 1
        grouped = np.asarray([self.index.offsets[self.clusters[j]] for j in r], dtype=np.int64) + cand - self.cand_offsets[r]
        slots = self.index.d_slots.download((self.index.n,), dtype=np.uint32).astype(np.int64)
        return slots[grouped]

    def constraint_map(self, d_flags, on_device=True):
        from . import circuit_sym as CS
        from .circuit_dev import DeviceBuilder
        cm, public, _ = CS.build_ann_probe(self.metric_name, self.K, [int(x) for x in self.sizes], self.dim, self.probes, self.topk, self.P, self.L,
                                           functools.partial(self._fetch_flags, d_flags), self._fetch, builder=DeviceBuilder if on_device else None)
        assert cm.n_cells == self.n_cells
        return cm, public, None


class AnnQueryHotPath(AnnProbeQueryHotPath):
    """The query of the nearest cluster alone (include/vdb.h vdb_wit_ann_query): nearest_vector(query, centroids), then
    nearest_vector(query, members of the winning centroid's cluster), both trees and the index root in ONE proof.  The reference runs the
    two searches in two circuits and compares roots outside them (tests/demo/mod.rs:52 "FIXME: these should be done in the same
    circuit"): this is that one circuit.  Public: the result vector, then the index root.  The circuit's shape depends on (K, n_c, dim,
    metric): one proving key per cluster size.  `cluster`: the cluster searched (None: index.probe(query)); a cluster other than the
    winning centroid's breaks the copy constraint.  AnnProbeQueryHotPath at probes = topk = 1, its results without the round axes."""

    def __init__(self, index, query, cluster=None, k=13, P=48, L=12, metric="euclidean", tau=None, col_shard=(0, 1), blind_seed=None, params=None,
                 cluster_roots=None, centroids=None):
        super().__init__(index, query, 1, 1, None if cluster is None else [cluster], k, P, L, metric, tau, col_shard, blind_seed, params, cluster_roots,
                         centroids)
        self.cluster = self.clusters[0]

    def results(self):
        """(centroid indicator (K, 4), member indicator (n_c, 4), result (dim, 4), index root (4,))"""
        ind_c, ind_m, res, root = super().results()
        return ind_c[0], ind_m[0], res[0], root


class _AnnBatchHotPath(PoseidonHotPath):
    """What the proofs of a batch against the committed index root share (AnnUpdateHotPath, AnnDeleteHotPath): the cluster c of an
    AnnIndex, its tree before the batch (`d_levels0`) and the copy every witness run works on (`d_levels`), the public row `d_pub` of
    `n_public` values, the map.  A subclass sets lp, depth, m, n_public and given_levels, and gives _circuit_size, _call(sel): the
    library's witness call on these buffers -> its return code, and _builder(CS): (circuit_sym's build function, its own keywords)."""

    def _load_inputs(self, grow=0):
        super()._load_inputs()
        self.d_levels0 = self._output(2 * self.lp * B)
        self.d_levels = self._output(2 * self.lp * B)
        d_given = self.d_levels if grow else self.d_levels0      # a tree that has yet to be grown into d_levels0 waits in d_levels
        self._load_tree(d_given, self.lp >> grow, self.index.levels(self.cluster) if self.given_levels is None else self.given_levels)

    def _alloc_outputs(self):
        self.d_pub = self._output(self.n_public * B)

    def _witness(self, sel=None):
        # the call writes the assigned header too; every run starts from the cluster's tree before the batch
        check(self.lib.vdb_memcpy_d2d(self.d_levels.ptr, self.d_levels0.ptr, ctypes.c_size_t(2 * self.lp * B)))
        with self._window(sel, 0, lookup=False):
            check(self._call(self._sel_at(sel, 0)))

    def public_values_dev(self):
        return self.d_pub.ptr, self.n_public

    def constraint_map(self, d_flags, on_device=True):
        from . import circuit_sym as CS
        from .circuit_dev import DeviceBuilder
        build, kw = self._builder(CS)
        cm, pub, _ = build(self.K, self.m, self.dim, self.depth, functools.partial(self._fetch_flags, d_flags), self._fetch,
                           builder=DeviceBuilder if on_device else None, **kw)
        assert cm.n_cells == self.n_cells
        return cm, pub, None


class AnnUpdateHotPath(_AnnBatchHotPath):
    """Inserts and replacements proved against the committed index root: m writes into ONE cluster c of an AnnIndex in one proof (include/vdb.h
    vdb_wit_ann_update).  Assigned: [c | centroids' root | cluster roots]; then idx_to_indicator(c, K), select_by_indicator(cluster roots,
    indicators) tied to the old root of the update block, the sponge over the roots (index_root_old), UpdateHotPath's whole circuit on the
    cluster's tree, out_j = select(new cluster root, cluster_root_j, indicator_j) and the sponge over [centroids' root | out_j]
    (index_root_new).  Public: [index_root_old | c | idx, old leaf, new leaf per write | index_root_new].  Writes only, and the members stay
    dense: slot s of the cluster is below its fill (a replacement) or equal to it (an append).  Cluster assignment is NOT proved: the caller
    chooses c (index.probe(v) is its tool).  K, m, grow and the depth are circuit shape, c is not.  `d_levels` holds the cluster's tree
    after the batch; AnnIndex.updated(hp) gives the next index."""

    def __init__(self, index, cluster, updates, grow=0, k=15, L=8, tau=None, col_shard=(0, 1), blind_seed=None, params=None, levels=None):
        """`updates`: (slots in the cluster (m,), (m, dim) f64 rows), applied in order.  `grow`: doublings of the cluster's tree before the
        first write; None: the smallest number that fits the appends.  `levels`: a tree to use in place of the index's segment c (a test of
        the binding: another cluster's tree breaks the picked copy)."""
        idx, rows = updates
        self.indices = np.ascontiguousarray(idx, dtype=np.uint64)
        m = self.indices.shape[0]
        if m < 1:
            raise ValueError("a batch holds at least one write")
        n_c = _bind_cluster(self, index, cluster)
        fill = n_c
        for s in self.indices.tolist():
            if s > fill:
                raise ValueError("a write above the cluster's fill: the members of a cluster stay dense")
            fill += s == fill
        self.appends = fill - n_c
        self.lp0, depth0 = api.merkle_levels(n_c)
        if grow is None:
            grow = 0
            while (self.lp0 << grow) < fill:
                grow += 1
        self.grow = int(grow)
        self.lp, self.depth = self.lp0 << self.grow, depth0 + self.grow
        if self.depth < 1:
            raise ValueError("a tree of one leaf has no path: grow it")
        super().__init__(n_c, index.dim, k, index.P, L, seed=None, tau=tau, col_shard=col_shard,
                         vectors=np.ascontiguousarray(rows, dtype=np.float64).reshape(m, index.dim), blind_seed=blind_seed, params=params)
        self.m, self.n_public, self.given_levels = m, 3 * m + 3, levels

    def n_input_rows(self):
        return self.m

    def _load_inputs(self):
        super()._load_inputs(self.grow)
        if self.grow:
            check(self.lib.vdb_merkle_tree_grow_dev(self.d_levels.ptr, self.n, self.grow, self.d_levels0.ptr))
            api.sync()

    def _circuit_size(self):
        cells, n_in, ub = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
        check(self.lib.vdb_wit_ann_update_size(self.K, self.n, self.dim, self.m, self.grow, ctypes.byref(cells), ctypes.byref(n_in), ctypes.byref(ub)))
        self.update_base = ub.value
        return n_in.value, cells.value - n_in.value, 0

    def _call(self, sel):
        return self.lib.vdb_wit_ann_update_dev(self.d_levels.ptr, self.index.d_roots.ptr, self.K, self.cluster, self.n, self.dim, self.grow, self.d_vec.ptr,
                                               api._p(self.indices), self.m, self.d_stream.ptr, sel, self.d_pub.ptr)

    def results(self):
        """(index_root_old (4,), c (4,), indices (m, 4), old leaves (m, 4), new leaves (m, 4), index_root_new (4,))"""
        pub = self.d_pub.download((3 * self.m + 3, 4))
        per = pub[2:-1].reshape(self.m, 3, 4)
        return pub[0], pub[1], per[:, 0], per[:, 1], per[:, 2], pub[-1]

    def _builder(self, CS):
        return CS.build_ann_update, dict(grow=self.grow)


class AnnWriteHotPath(AnnUpdateHotPath):
    """Linked writes: m inserts or replacements into ONE cluster c of an AnnIndex and the same m leaf changes in the database tree, in one
    proof (include/vdb.h vdb_wit_ann_write): (database_root_old, index_root_old) to (database_root_new, index_root_new).  The circuit is
    AnnUpdateHotPath's, cell for cell, with one more block E_db between E and F: the update block of the database tree at dim 1 whose new
    leaves are CARRIED: one witness cell each, tied to the digest E's leaf sponge squeezed, its old leaf tied to E's old leaf; every vector
    is hashed once.  So a cover of the old pair of roots (AnnCoverHotPath) and this proof cover the new pair.  Public: [database_root_old |
    index_root_old | c | idx, db_idx, old leaf, new leaf per write | database_root_new | index_root_new]; a verifier who tracks n_c and n
    checks for an append idx = the cluster's fill, db_idx = the database's fill and old leaf = 0.  (K, d_c, g_c, d_db, g_db, m, dim) are
    circuit shape; c, the slots and the values are not.  `d_levels` and `d_levels_db` hold the two trees after the batch;
    AnnIndex.written(hp) gives the next index with its database tree."""

    def __init__(self, index, cluster, updates, grow=None, k=15, L=8, tau=None, col_shard=(0, 1), blind_seed=None, params=None, levels=None, levels_db=None,
                 db_indices=None):
        """`updates`, `grow`, `levels`: as AnnUpdateHotPath (grow None: the smallest number that fits, which AnnIndex.written demands).
        The database slots come from the index's own slots of cluster c; `db_indices` (m,) overrides them and `levels_db` the index's
        database tree, not yet grown (tests of the binding)."""
        super().__init__(index, cluster, updates, grow=grow, k=k, L=L, tau=tau, col_shard=col_shard, blind_seed=blind_seed, params=params, levels=levels)
        slots = index.d_slots.download((self.n,), dtype=np.uint32, offset=int(index.offsets[self.cluster]) * 4)
        own, _ = api.ann_write_db_indices(slots, self.indices, index.n)
        self.db_indices = own if db_indices is None else np.ascontiguousarray(db_indices, dtype=np.uint64)
        self.n_db = index.n
        self.lp_db0, depth_db0 = api.merkle_levels(self.n_db)
        self.lp_db, self.depth_db = api.merkle_levels(self.n_db + self.appends)
        if self.depth_db < 1:
            raise ValueError("a database tree of one leaf has no path")
        self.grow_db = self.depth_db - depth_db0
        self.n_public, self.given_levels_db, self.given_db_indices = 4 * self.m + 5, levels_db, db_indices

    def _load_inputs(self):
        super()._load_inputs()
        self.d_levels_db0 = self._output(2 * self.lp_db * B)     # the grown database tree before the batch
        self.d_levels_db = self._output(2 * self.lp_db * B)
        given = self.index.database_tree() if self.given_levels_db is None else self.given_levels_db
        self._load_tree(self.d_levels_db if self.grow_db else self.d_levels_db0, self.lp_db0, given)
        if self.grow_db:
            check(self.lib.vdb_merkle_tree_grow_dev(self.d_levels_db.ptr, self.n_db, self.grow_db, self.d_levels_db0.ptr))
            api.sync()

    def _witness(self, sel=None):
        check(self.lib.vdb_memcpy_d2d(self.d_levels_db.ptr, self.d_levels_db0.ptr, ctypes.c_size_t(2 * self.lp_db * B)))
        super()._witness(sel)

    def _circuit_size(self):
        cells, n_in, ub, udb = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
        check(self.lib.vdb_wit_ann_write_size(self.K, self.n, self.n_db, self.dim, self.m, self.appends, ctypes.byref(cells), ctypes.byref(n_in), ctypes.byref(ub),
                                              ctypes.byref(udb), None, None))
        self.update_base, self.update_db_base = ub.value, udb.value
        return n_in.value, cells.value - n_in.value, 0

    def _call(self, sel):
        return self.lib.vdb_wit_ann_write_dev(self.d_levels.ptr, self.d_levels_db.ptr, self.index.d_roots.ptr, self.K, self.cluster, self.n, self.n_db, self.dim,
                                              self.grow, self.grow_db, self.d_vec.ptr, api._p(self.indices), api._p(self.db_indices), self.m, self.d_stream.ptr,
                                              sel, self.d_pub.ptr)

    def results(self):
        """(database_root_old (4,), index_root_old (4,), c (4,), indices (m, 4), database indices (m, 4), old leaves (m, 4), new leaves
        (m, 4), database_root_new (4,), index_root_new (4,))"""
        pub = self.d_pub.download((4 * self.m + 5, 4))
        per = pub[3:-2].reshape(self.m, 4, 4)
        return (pub[0], pub[1], pub[2]) + tuple(per[:, i] for i in range(4)) + (pub[-2], pub[-1])

    def _builder(self, CS):
        return CS.build_ann_write, dict(grow=self.grow, depth_db=self.depth_db, grow_db=self.grow_db)


class AnnDeleteHotPath(_AnnBatchHotPath):
    """Deletes proved against the committed index root: m deletes from ONE cluster c of an AnnIndex in one proof (include/vdb.h
    vdb_wit_ann_delete).  The members stay dense by swap-with-last: delete j moves the member at last_j = fill - 1 into slot_j and empties
    the last slot, two path updates of the cluster's tree (a carried leaf, then a delete); when the cluster drops to a power of two the
    tree halves, and the circuit proves that the dropped half is empty (block S).  Blocks A - D, F, G are AnnUpdateHotPath's.  Public:
    [index_root_old | c | slot, removed leaf, last, moved leaf per delete | index_root_new]; a verifier who tracks n_c checks
    last_j = n_c - 1 - j.  No input rows.  K, m, the depth and the halvings `s` are circuit shape, c and the slots are not.  `d_levels`
    holds the cluster's tree after the batch at its old size; AnnIndex.removed(hp) gives the next index (which cuts it).  `origin[p]`:
    the slot that held, before the batch, the member at surviving position p."""

    def __init__(self, index, cluster, slots, k=15, L=8, tau=None, col_shard=(0, 1), blind_seed=None, params=None, levels=None):
        """`slots`: (m,) slots of the cluster, each below the fill at its turn (n_c - j); repeats are legal.  `levels`: a tree to use in
        place of the index's segment c (tests of the binding)."""
        self.slots = np.ascontiguousarray(slots, dtype=np.uint64)
        m = self.slots.shape[0]
        n_c = _bind_cluster(self, index, cluster)
        if m < 1 or m >= n_c:
            raise ValueError("a batch holds at least one delete and leaves at least one member")
        origin = list(range(n_c))
        for j, s in enumerate(self.slots.tolist()):
            if s >= n_c - j:
                raise ValueError("a slot at or above the cluster's fill at its turn")
            origin[s] = origin[n_c - j - 1]
        self.origin = origin[:n_c - m]
        self.lp, self.depth = api.merkle_levels(n_c)
        super().__init__(n_c, index.dim, k, index.P, L, seed=None, tau=tau, col_shard=col_shard, vectors=np.zeros((0, index.dim)), blind_seed=blind_seed,
                         params=params)
        self.m, self.n_public, self.given_levels = m, 4 * m + 3, levels

    def n_input_rows(self):
        return 0

    def _circuit_size(self):
        cells, n_in, ub, sb, s = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint()
        check(self.lib.vdb_wit_ann_delete_size(self.K, self.n, self.dim, self.m, ctypes.byref(cells), ctypes.byref(n_in), ctypes.byref(ub), ctypes.byref(sb),
                                               ctypes.byref(s)))
        self.update_base, self.shrink_base, self.shrink = ub.value, sb.value, s.value
        return n_in.value, cells.value - n_in.value, 0

    def _call(self, sel):
        return self.lib.vdb_wit_ann_delete_dev(self.d_levels.ptr, self.index.d_roots.ptr, self.K, self.cluster, self.n, self.dim, api._p(self.slots), self.m,
                                               self.d_stream.ptr, sel, self.d_pub.ptr)

    def results(self):
        """(index_root_old (4,), c (4,), slots (m, 4), removed leaves (m, 4), last (m, 4), moved leaves (m, 4), index_root_new (4,))"""
        pub = self.d_pub.download((4 * self.m + 3, 4))
        per = pub[2:-1].reshape(self.m, 4, 4)
        return pub[0], pub[1], per[:, 0], per[:, 1], per[:, 2], per[:, 3], pub[-1]

    def _builder(self, CS):
        return CS.build_ann_delete, dict(shrink=self.shrink)


class AnnMoveHotPath(_AnnBatchHotPath):
    """Moves proved against the committed index root: m members pass from cluster a = `src` to cluster b = `dst` of an AnnIndex in one
    proof (include/vdb.h vdb_wit_ann_move), index_root_old to index_root_new.  Move j is delete j of a (AnnDeleteHotPath's blocks E' and S
    on a's tree) and an append to b at dest_j = n_b + j whose new leaf is CARRIED: one witness cell tied to the removed leaf, so no vector
    enters the circuit and the database, its slots and its root are untouched.  b's root is selected from the roots after the removal.
    Public: [index_root_old | a | b | slot, leaf, last, moved leaf, dest, dest old leaf per move | index_root_new]; a verifier who tracks
    n_a and n_b checks last_j = n_a - 1 - j, dest_j = n_b + j and dest old leaf = 0.  No input rows, no lookup cells.  (K, d_a, s, d_b, g,
    m) are circuit shape; a, b and the slots are not.  `d_levels_a` and `d_levels_b` hold the two trees after the batch (a's at its old
    size); AnnIndex.moved(hp) gives the next index.  `origin[p]`: the slot of a that held, before the batch, the member at surviving
    position p; `moved_from[j]`: the slot of a that held the member move j takes to b."""

    def __init__(self, index, src, dst, slots, grow=None, k=15, L=8, tau=None, col_shard=(0, 1), blind_seed=None, params=None, levels_src=None,
                 levels_dst=None):
        """`slots`: (m,) slots of cluster src, each below its fill at its turn (n_a - j); repeats are legal.  `grow`: doublings of b's
        tree before the first append: None, or the smallest number that fits.  `levels_src` / `levels_dst`: trees to use in place of the
        index's segments a and b, the latter not yet grown (tests of the binding)."""
        self.slots = np.ascontiguousarray(slots, dtype=np.uint64)
        m = self.slots.shape[0]
        n_a = _bind_cluster(self, index, src)
        self.src, self.dst = self.cluster, int(dst)
        if not 0 <= self.dst < self.K or self.dst == self.src:
            raise ValueError("the destination is another cluster of the index")
        n_b = int(index.sizes[self.dst])
        if m < 1 or m >= n_a:
            raise ValueError("a batch holds at least one move and leaves at least one member")
        origin, self.moved_from = list(range(n_a)), []
        for j, s in enumerate(self.slots.tolist()):
            if s >= n_a - j:
                raise ValueError("a slot at or above the source cluster's fill at its turn")
            self.moved_from.append(origin[s])
            origin[s] = origin[n_a - j - 1]
        self.origin = origin[:n_a - m]
        self.lp, self.depth = api.merkle_levels(n_a)
        self.lp_b0, depth_b0 = api.merkle_levels(n_b)
        self.lp_b, self.depth_b = api.merkle_levels(n_b + m)
        if grow is not None and int(grow) != self.depth_b - depth_b0:
            raise ValueError("grow is the smallest number of doublings after which the destination's tree holds its new members")
        self.grow = self.depth_b - depth_b0
        super().__init__(n_a, index.dim, k, index.P, L, seed=None, tau=tau, col_shard=col_shard, vectors=np.zeros((0, index.dim)), blind_seed=blind_seed,
                         params=params)
        self.n_b, self.m, self.n_public, self.given_levels, self.given_levels_b = n_b, m, 6 * m + 4, levels_src, levels_dst

    def n_input_rows(self):
        return 0

    def _load_inputs(self):
        super()._load_inputs()
        self.d_levels_a = self.d_levels
        self.d_levels_b0 = self._output(2 * self.lp_b * B)       # b's grown tree before the batch
        self.d_levels_b = self._output(2 * self.lp_b * B)
        given = self.index.levels(self.dst) if self.given_levels_b is None else self.given_levels_b
        self._load_tree(self.d_levels_b if self.grow else self.d_levels_b0, self.lp_b0, given)
        if self.grow:
            check(self.lib.vdb_merkle_tree_grow_dev(self.d_levels_b.ptr, self.n_b, self.grow, self.d_levels_b0.ptr))
            api.sync()

    def _witness(self, sel=None):
        check(self.lib.vdb_memcpy_d2d(self.d_levels_b.ptr, self.d_levels_b0.ptr, ctypes.c_size_t(2 * self.lp_b * B)))
        super()._witness(sel)

    def _circuit_size(self):
        cells, n_in, db, sb, ab = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
        s, g = ctypes.c_uint(), ctypes.c_uint()
        check(self.lib.vdb_wit_ann_move_size(self.K, self.n, self.n_b, self.m, ctypes.byref(cells), ctypes.byref(n_in), ctypes.byref(db), ctypes.byref(sb),
                                             ctypes.byref(ab), ctypes.byref(s), ctypes.byref(g)))
        assert g.value == self.grow
        self.delete_base, self.shrink_base, self.append_base, self.shrink = db.value, sb.value, ab.value, s.value
        return n_in.value, cells.value - n_in.value, 0

    def _call(self, sel):
        return self.lib.vdb_wit_ann_move_dev(self.d_levels.ptr, self.d_levels_b.ptr, self.index.d_roots.ptr, self.K, self.src, self.dst, self.n, self.n_b,
                                             self.grow, api._p(self.slots), self.m, self.d_stream.ptr, sel, self.d_pub.ptr)

    def results(self):
        """(index_root_old (4,), a (4,), b (4,), slots (m, 4), leaves (m, 4), last (m, 4), moved leaves (m, 4), dest (m, 4), dest old
        leaves (m, 4), index_root_new (4,))"""
        pub = self.d_pub.download((6 * self.m + 4, 4))
        per = pub[3:-1].reshape(self.m, 6, 4)
        return (pub[0], pub[1], pub[2]) + tuple(per[:, i] for i in range(6)) + (pub[-1],)

    def constraint_map(self, d_flags, on_device=True):
        from . import circuit_sym as CS
        from .circuit_dev import DeviceBuilder
        cm, pub, _ = CS.build_ann_move(self.K, self.m, self.depth, self.shrink, self.depth_b, self.grow, functools.partial(self._fetch_flags, d_flags),
                                       self._fetch, builder=DeviceBuilder if on_device else None)
        assert cm.n_cells == self.n_cells
        return cm, pub, None


class _AnnClusterHotPath(HotPath):
    """What the audits of one cluster c of a committed AnnIndex share (AnnAuditHotPath, AnnMeanHotPath): the binding to (index, cluster),
    where the call reads the centroids and the members (`p_cent`, `p_members`: the resident index, or the overrides given; `resident`),
    no input rows, the flag bytes and the public row [index_root | c] (`d_pub`), the map.  A subclass gives _size(*outputs) and
    _call(*shared arguments): the library's size and witness calls -> their return codes, _n_flags(): the length of its flag bytes, and
    _builder(CS): (circuit_sym's build function, the arguments ahead of K)."""

    def __init__(self, index, cluster, k=13, P=48, L=12, tau=None, col_shard=(0, 1), blind_seed=None, params=None, centroids=None, members=None):
        n_c = _bind_cluster(self, index, cluster)
        super().__init__(n_c, index.dim, k, P, L, seed=None, tau=tau, col_shard=col_shard, vectors=np.zeros((0, index.dim)), blind_seed=blind_seed,
                         params=params)
        self.given_cent, self.given_members = centroids, members

    def n_input_rows(self):
        return 0

    def _load_inputs(self):
        super()._load_inputs()
        ix, self.resident = self.index, self.given_cent is None and self.given_members is None
        self.p_cent = _given_ptr(self, self.given_cent, (self.K, self.dim, 4), ix.d_cent.ptr)
        self.p_members = _given_ptr(self, self.given_members, (self.n, self.dim, 4), ix.members_ptr(self.cluster))

    def _circuit_size(self):
        cells, lk, n_in = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
        check(self._size(ctypes.byref(cells), ctypes.byref(lk), ctypes.byref(n_in)))
        return n_in.value, cells.value - n_in.value, lk.value

    def _alloc_outputs(self):
        self.d_flag_bytes, self.d_pub = self._output(max(self._n_flags(), 32)), self._output(2 * B)

    def _witness(self, sel=None):
        # the call writes the assigned header, centroids and members too
        ix = self.index
        with self._window(sel, 0):
            check(self._call(self.p_cent, self.p_members, ix.d_roots.ptr, ix.levels_ptr(self.K) if self.resident else None,
                             ix.levels_ptr(self.cluster) if self.resident else None, self.K, self.cluster, self.n, self.dim, self.d_stream.ptr,
                             self.d_lookup.ptr, self._sel_at(sel, 0), self.d_flag_bytes.ptr, self.d_pub.ptr))

    def public_values_dev(self):
        return self.d_pub.ptr, 2

    def results(self):
        """(index_root (4,), c (4,), the flag bytes, uint8: the audit's routed (n_c,), member i's own centroid attains the minimum of its K
        distances; the mean's mean_ok (dim,), word j of centroid c is the mean of the members' words j)"""
        pub = self.d_pub.download((2, 4))
        return pub[0], pub[1], self.d_flag_bytes.download((self._n_flags(),), dtype=np.uint8)

    def constraint_map(self, d_flags, on_device=True):
        from . import circuit_sym as CS
        from .circuit_dev import DeviceBuilder
        build, ahead = self._builder(CS)
        cm, public, _ = build(*ahead, self.K, self.n, self.dim, self.P, self.L, functools.partial(self._fetch_flags, d_flags), self._fetch,
                              builder=DeviceBuilder if on_device else None)
        assert cm.n_cells == self.n_cells
        return cm, public, None


class AnnAuditHotPath(_AnnClusterHotPath):
    """The routing of ONE cluster c of a committed AnnIndex proved in one proof (include/vdb.h vdb_wit_ann_audit): every member committed
    under cluster_root_c is at least as close to centroid c as to any other committed centroid, in the circuit's fixed-point distance.
    Assigned: the header [c | centroids' root | cluster roots]; then idx_to_indicator(c, K), select_by_indicator(cluster roots, indicators)
    -> picked, the sponge over the roots (index_root), [centroids | members] assigned, per member its K distances, their qmin chain and
    select_by_indicator(distances, indicators) tied to the chain's minimum, merkle_commitment(centroids) tied to the header's centroids'
    root and merkle_commitment(members) tied to picked.  Public: [index_root | c].  It covers the build's cluster ids and the writes after
    them: audit cluster c of index.updated(hp) after a batch into c; K proofs cover an index.  That centroids are means is
    proved per cluster by a proof of its own (AnnMeanHotPath).  That the members are the database: AnnCoverHotPath.  A member equidistant from two centroids is accepted under either.  The shape depends on (K, n_c, dim,
    metric): one proving key per cluster size.  A misrouted member still gives a witness; results()[2] flags it and its copy fails in
    the Mock report.  `centroids` / `members`: quantized overrides of what the index holds (tests of the binding); with them the two
    trees are hashed by the call instead of read from the forest."""

    def __init__(self, index, cluster, k=13, P=48, L=12, metric="euclidean", tau=None, col_shard=(0, 1), blind_seed=None, params=None, centroids=None,
                 members=None):
        super().__init__(index, cluster, k, P, L, tau, col_shard, blind_seed, params, centroids, members)
        self.metric, self.metric_name = api.METRICS[metric], metric

    d_routed = property(lambda self: self.d_flag_bytes)

    def _n_flags(self):
        return self.n

    def _size(self, *out):
        return self.lib.vdb_wit_ann_audit_size(self.metric, self.P, self.L, self.K, self.n, self.dim, *out)

    def _call(self, *shared):
        return self.lib.vdb_wit_ann_audit_dev(self.metric, self.P, self.L, *shared)

    def _builder(self, CS):
        return CS.build_ann_audit, (self.metric_name,)


class AnnMeanHotPath(_AnnClusterHotPath):
    """That centroid c of a committed AnnIndex is the mean of its cluster, proved in one proof (include/vdb.h vdb_wit_ann_mean): word for
    word, centroid c equals qdiv(sum of the members committed under cluster_root_c, quantization(n_c)) in the circuit's fixed-point
    arithmetic.  Assigned: the header [c | centroids' root | cluster roots]; then idx_to_indicator(c, K), select_by_indicator(cluster
    roots, indicators) -> picked, the sponge over the roots (index_root), [centroids | members] assigned, select_by_indicator(centroids,
    indicators) -> own word by word, the constant quantization(n_c), the qadd chain over the members and one qdiv per word tied to own,
    merkle_commitment(centroids) tied to the header's centroids' root and merkle_commitment(members) tied to picked.  Public:
    [index_root | c].  K mean proofs and K routing audits (AnnAuditHotPath) state that the index is a fixed point of one Lloyd step over
    the committed members.  That the members are the database: AnnCoverHotPath.  That a recentred index descends from its predecessor is a
    proof of its own, one centroid at a time (AnnRecentreHotPath).  The shape depends on (K, n_c, dim): one proving key per cluster size.  A centroid that is not the mean still gives a
    witness; results()[2] flags the words that differ and their copies fail in the Mock report.  `centroids` / `members`: quantized
    overrides of what the index holds (tests of the binding); with them the two trees are hashed by the call instead of read from the
    forest."""

    d_ok = property(lambda self: self.d_flag_bytes)

    def _n_flags(self):
        return self.dim

    def _size(self, *out):
        return self.lib.vdb_wit_ann_mean_size(self.P, self.L, self.K, self.n, self.dim, *out)

    def _call(self, *shared):
        return self.lib.vdb_wit_ann_mean_dev(self.P, self.L, *shared)

    def _builder(self, CS):
        return CS.build_ann_mean, ()


class AnnRecentreHotPath(HotPath):
    """The recentre of ONE cluster c of a committed AnnIndex proved from the old index root to the new one (include/vdb.h
    vdb_wit_ann_recentre): the index under index_root_new has the K cluster roots of the index under index_root_old, and its centroids'
    tree is the old one with leaf c replaced by the leaf of qdiv(sum of the members committed under cluster_root_c, quantization(n_c)),
    word for word the quotient AnnMeanHotPath accepts.  Assigned: the header [c | centroids' root | cluster roots]; then
    idx_to_indicator(c, K), select_by_indicator(cluster roots, indicators) -> picked, the sponge over the roots (index_root_old), the
    members assigned, the constant quantization(n_c), the qadd chain over the members and one qdiv per word, merkle_commitment(members)
    tied to picked, UpdateHotPath's circuit with one write on the centroids' tree — its old root tied to the header's centroids' root,
    its index to c, its new vector to the quotients — and the sponge over [the new centroids' root | cluster roots] (index_root_new).
    Public: [index_root_old | c | index_root_new].  K such proofs, one per cluster, recentre an index: the memberships do not change
    between them, so the chain ends on the root of AnnIndex.recentred().  The old centroid is never assigned.  Not proved: that
    the members are still routed to their cluster after the recentre (the routing audits of the new root say which are not; a delete
    from one cluster and a write into another moves them).  That the members are the database: AnnCoverHotPath.  The shape depends on (K, n_c, dim): one proving key
    per cluster size.  `d_levels` holds the centroids' tree after the write and `d_new` the new centroid; AnnIndex.recentred_with(hp)
    gives the next index.  `members` / `levels`: quantized overrides of the cluster's members and of the centroids' tree (tests of the
    binding); with `members` the cluster's tree is hashed by the call instead of read from the forest."""

    def __init__(self, index, cluster, k=13, P=48, L=12, tau=None, col_shard=(0, 1), blind_seed=None, params=None, members=None, levels=None):
        n_c = _bind_cluster(self, index, cluster)
        if self.K < 2:
            raise ValueError("a tree of one leaf has no path: an index of one cluster has no centroid to open")
        super().__init__(n_c, index.dim, k, P, L, seed=None, tau=tau, col_shard=col_shard, vectors=np.zeros((0, index.dim)), blind_seed=blind_seed,
                         params=params)
        self.lp, self.depth = api.merkle_levels(self.K)
        self.given_members, self.given_levels = members, levels

    def n_input_rows(self):
        return 0

    def _load_inputs(self):
        super()._load_inputs()
        ix, self.resident = self.index, self.given_members is None
        self.p_members = _given_ptr(self, self.given_members, (self.n, self.dim, 4), ix.members_ptr(self.cluster))
        self.d_levels0, self.d_levels = self._output(2 * self.lp * B), self._output(2 * self.lp * B)
        if self.given_levels is None:
            check(self.lib.vdb_memcpy_d2d(self.d_levels0.ptr, ix.levels_ptr(self.K), ctypes.c_size_t(2 * self.lp * B)))
        else:
            lv = np.ascontiguousarray(self.given_levels, dtype=np.uint64)
            assert lv.shape == (2 * self.lp, 4), "the tree does not belong to this shape"
            self.d_levels0.upload(lv)

    def _circuit_size(self):
        cells, lk, n_in, ub = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
        check(self.lib.vdb_wit_ann_recentre_size(self.P, self.L, self.K, self.n, self.dim, ctypes.byref(cells), ctypes.byref(lk), ctypes.byref(n_in),
                                                 ctypes.byref(ub)))
        self.update_base = ub.value
        return n_in.value, cells.value - n_in.value, lk.value

    def _alloc_outputs(self):
        self.d_new, self.d_pub = self._output(max(self.dim * B, 32)), self._output(3 * B)

    def _witness(self, sel=None):
        # the call writes the assigned header and members too; every run starts from the centroids' tree before the write
        ix = self.index
        check(self.lib.vdb_memcpy_d2d(self.d_levels.ptr, self.d_levels0.ptr, ctypes.c_size_t(2 * self.lp * B)))
        with self._window(sel, 0):
            check(self.lib.vdb_wit_ann_recentre_dev(self.P, self.L, self.d_levels.ptr, self.p_members, ix.d_roots.ptr,
                                                    ix.levels_ptr(self.cluster) if self.resident else None, self.K, self.cluster, self.n, self.dim,
                                                    self.d_stream.ptr, self.d_lookup.ptr, self._sel_at(sel, 0), self.d_new.ptr, self.d_pub.ptr))

    def public_values_dev(self):
        return self.d_pub.ptr, 3

    def results(self):
        """(index_root_old (4,), c (4,), index_root_new (4,), the new centroid (dim, 4))"""
        pub = self.d_pub.download((3, 4))
        return pub[0], pub[1], pub[2], self.d_new.download((self.dim, 4))

    def constraint_map(self, d_flags, on_device=True):
        from . import circuit_sym as CS
        from .circuit_dev import DeviceBuilder
        cm, public, _ = CS.build_ann_recentre(self.K, self.n, self.dim, self.P, self.L, functools.partial(self._fetch_flags, d_flags), self._fetch,
                                              builder=DeviceBuilder if on_device else None)
        assert cm.n_cells == self.n_cells
        return cm, public, None


class AnnCoverHotPath(PoseidonHotPath):
    """The index holds exactly the committed database (include/vdb.h vdb_wit_ann_cover): public [database_root | index_root], where
    database_root is the merkle_commitment root QueryHotPath / MerkleHotPath / UpdateHotPath / ReadHotPath publish for the rows in slot
    order and index_root the root every index proof is bound to.  Assigned: the header [centroids' root | cluster roots] and the 2 n leaf
    digests, the database's in slot order and the clusters' in grouped order; then the database tree and the K cluster trees over them
    (every root tied to the header), the sponge over the header (index_root), gamma = sponge([database_root, index_root]) and the two
    products prod (gamma - a_i), prod (gamma - b_j), tied: the two multisets of leaf digests are equal, so the members of the index are
    the database's vectors with their multiplicities (gamma is the circuit's own hash of the two roots, the one step argued in the model of an ideal hash).  No vector is hashed: the statement is on
    leaf digests, which both commitments share.  The shape — and the verifying key — depends on n, K and the K cluster sizes, which are
    therefore public.  Not covered: a database with emptied slots (after UpdateHotPath deletes; AnnIndex's own deletes compact).
    `leaves`: (database leaf digests (n, 4), cluster leaf digests (n, 4)) in place of what the index holds (tests of the binding); the
    K + 1 trees are then hashed by the call instead of read where they lie."""

    def __init__(self, index, k=15, L=8, tau=None, col_shard=(0, 1), blind_seed=None, params=None, leaves=None):
        self.index, self.K = index, index.K
        self.sizes64 = np.ascontiguousarray(index.sizes, dtype=np.uint64)
        super().__init__(index.n, index.dim, k, index.P, L, seed=None, tau=tau, col_shard=col_shard, vectors=np.zeros((0, index.dim)), blind_seed=blind_seed,
                         params=params)
        self.given_leaves = leaves

    def n_input_rows(self):
        return 0

    def _load_inputs(self):
        super()._load_inputs()
        self.resident = self.given_leaves is None
        if self.resident:
            self.p_tree, self.p_a, self.p_b = self.index.database_tree().ptr, None, None
        else:
            a, b = (np.ascontiguousarray(x, dtype=np.uint64) for x in self.given_leaves)
            assert a.shape == (self.n, 4) and b.shape == (self.n, 4), "n leaf digests a side"
            self.p_tree = None
            self.p_a, self.p_b = _given_ptr(self, a, a.shape, None), _given_ptr(self, b, b.shape, None)

    def _circuit_size(self):
        cells, n_in = ctypes.c_uint64(), ctypes.c_uint64()
        check(self.lib.vdb_wit_ann_cover_size(api._p(self.sizes64), self.K, self.n, ctypes.byref(cells), ctypes.byref(n_in)))
        return n_in.value, cells.value - n_in.value, 0

    def _alloc_outputs(self):
        self.d_pub = self._output(2 * B)

    def _witness(self, sel=None):
        # the call writes the assigned header and digests too; the centroids' root is word 0 of the index's roots
        ix = self.index
        with self._window(sel, 0, lookup=False):
            check(self.lib.vdb_wit_ann_cover_dev(self.p_a, self.p_b, ix.d_roots.ptr, api._p(self.sizes64), self.K, self.n, self.p_tree,
                                                 ix.d_forest.ptr if self.resident else None, self.d_stream.ptr, self._sel_at(sel, 0), self.d_pub.ptr))

    def public_values_dev(self):
        return self.d_pub.ptr, 2

    def results(self):
        """(database_root (4,), index_root (4,))"""
        pub = self.d_pub.download((2, 4))
        return pub[0], pub[1]

    def constraint_map(self, d_flags, on_device=True):
        from . import circuit_sym as CS
        from .circuit_dev import DeviceBuilder
        cm, public, _ = CS.build_ann_cover(self.index.sizes, functools.partial(self._fetch_flags, d_flags), self._fetch,
                                           builder=DeviceBuilder if on_device else None)
        assert cm.n_cells == self.n_cells
        return cm, public, None
