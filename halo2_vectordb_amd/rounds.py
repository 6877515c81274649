"""The prover's rounds after the advice commitments, composed from the device bricks on the buffers the
k-means hot path leaves resident: lookup permutation -> products -> quotient -> evaluations -> openings, every polynomial
step on the GPU, nothing but commitments, evaluations and challenges crossing the C ABI.

The circuit proved is the reference's circuit: the vertical gate on every gate row, every lookup cell in the range table,
and the permutation argument over the advice columns, the lookup columns, ONE fixed column of constants and ONE instance
column, with every copy halo2-base records while the closure runs — `Existing` cells, `Constant` cells (tied to the fixed
column), constrain_equal / assert_is_const, the lookup cells (copies of advice cells), the overlap cell the column layout
duplicates — taken from the circuit's symbolic map (circuit_sym.py for the fixed-point gadgets, copymap.py for the Merkle
circuit), and every cell the closure pushes into `make_public` tied to its row of the instance column
(RangeWithInstanceCircuitBuilder, /root/reference/src/scaffold/mod.rs:400; the values are circuit.instances(), :265): the
centroids for k-means (examples/kmeans.rs:51-56), the result vector for nearest_vector (examples/query.rs:58), the root for
the Merkle circuit (examples/merkle.rs:47).  The instance polynomial is not committed: prover and verifier both make it from
the public values, which enter the transcript first (halo2's KZG provers: QUERY_INSTANCE = false, [UPSTREAM-RECALL]).
What this is not: halo2's exact proof layout (the order of terms and challenges is recalled, [UPSTREAM-RECALL]; the
Fiat–Shamir transcript is the library's own, vdb_transcript_*; the multi-open is SHPLONK, or one quotient per rotation point
with multiopen="gwc"); the order of the quotient's terms follows plonk/evaluation.rs as recalled ([UPSTREAM-RECALL]; parity
unpinned).  What the tests hold it to instead is what a verifier checks: the quotient identity at a random point recombined
from the returned evaluations, and every opening against its commitments in the exponent (tests/test_gpu_rounds.py).
"""
import contextlib
import ctypes
from collections.abc import Mapping

import os
import time

import numpy as np

from . import api, protocol
from ._lib import check
from .protocol import DERIVED, FIXED, MINIMUM_ROWS, N_BLIND, R_MOD, constraint_degree
from .protocol import fr_from_int as _fr_from_int, fr_to_int as _fr_to_int

B = 32
# The quotient has n_h = degree - 1 pieces (protocol.constraint_degree).
# halo2 evaluates the numerator on every point of the extended domain; the quotient has degree below n_h n, so its values on n_h of the
# cosets of the 2^k-th roots of unity determine it, and the gates' share (degree 3: below 2 n) on two.  The rounds work coset by coset
# ("slots", vdb_coeff_to_cosets_dev: arrays [column][slot][row]) on n_slots = n_h of them and never make the rest: with degree 4 a
# quarter of every extended transform and of every evaluation kernel is not run, and the quotient that comes out is the same polynomial.
GATE_SLOTS = 2               # cosets the gate terms are evaluated on (slots 0, 1 = the coset of 2 n points)
BLOCK_COLS = 510 # fixed-polynomial cosets are produced this many columns at a time (a multiple of every chunk_len; 3.2 GB at 2^16 rows)


def _sz(v):
    return ctypes.c_size_t(int(v))


def _position(ranges, i):
    """position of global index i in a buffer that holds the stretches `ranges` one after the other (this rank's sets in its
    product buffers, its permutation columns in its sigma buffers)"""
    off = 0
    for lo, hi in ranges:
        if lo <= i < hi:
            return off + i - lo
        off += hi - lo
    raise KeyError(i)


def _consts_table(consts):
    """a circuit's distinct constants (Python integers) as Montgomery field elements, (n, 4): the fixed column's first rows"""
    if not len(consts):
        return np.zeros((0, 4), dtype=np.uint64)
    return api.fr_from_canonical(np.array([[(int(v) >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)] for v in consts], dtype=np.uint64))


class _View:
    """a stretch of a pooled device allocation (same surface as api.DeviceBuffer; freeing it is a no-op)"""

    def __init__(self, buf, offset, nbytes):
        self.ptr, self.nbytes = ctypes.c_void_p(buf.ptr.value + int(offset)), int(nbytes)

    def at(self, offset):
        return ctypes.c_void_p(self.ptr.value + int(offset))

    def download(self, shape, dtype=np.uint64, offset=0):
        out = np.empty(shape, dtype=dtype)
        assert offset + out.nbytes <= self.nbytes
        check(api.init().vdb_memcpy_d2h(api._p(out), self.at(offset), _sz(out.nbytes)))
        return out

    def free(self):
        pass


class _Evals(Mapping):
    """evaluations as returned by prove(): (name, rotation) -> list of canonical Python integers, converted from the
    Montgomery arrays the device returned when first asked for (a proof of 2 x 10^4 columns carries ~2 x 10^5 of them)"""

    def __init__(self, raw):
        self.raw, self._ints = raw, {}

    def __getitem__(self, key):
        if key not in self._ints:
            a = np.ascontiguousarray(self.raw[key], dtype=np.uint64).reshape(-1, 4)
            self._ints[key] = [int(r[0]) | int(r[1]) << 64 | int(r[2]) << 128 | int(r[3]) << 192 for r in api.fr_to_canonical(a)] if len(a) else []
        return self._ints[key]

    def __iter__(self):
        return iter(self.raw)

    def __len__(self):
        return len(self.raw)


class _Poly:
    """a set of polynomials in the three forms the rounds use; any of them may be absent.  In a sharded proof the buffers hold
    this rank's part only: `ranges` = the [lo, hi) stretches of the set's global numbering that lie in the buffers one after the
    other (n_cols polynomials in all), `n_total` = the size of the whole set; `commits` is always the whole set's (gathered).
    `replicated`: every rank holds the whole set (the small fixed polynomials, the quotient's pieces)."""

    def __init__(self, name, n_cols, lag=None, coeff=None, ext=None, commits=None, ranges=None, n_total=None, replicated=False):
        self.name, self.n_cols, self.lag, self.coeff, self.ext, self.commits = name, n_cols, lag, coeff, ext, commits
        self.ranges = [(0, n_cols)] if ranges is None else [(int(a), int(b)) for a, b in ranges if b > a]
        self.n_total = n_cols if n_total is None else int(n_total)
        self.replicated = replicated
        assert sum(b - a for a, b in self.ranges) == n_cols

    def free(self):
        for b in (self.lag, self.coeff, self.ext):
            if b is not None:
                b.free()
        self.lag = self.coeff = self.ext = None


class _Proof:
    """What one run of ProverRounds.prove carries from round to round: the transcript (None when the challenges are handed
    in), the challenges `ch` and their pointers `p`, the host's transcript time `host`, the device `timings` (None: untimed),
    the blinding seed, the polynomials made so far and the public values."""

    def __init__(self, challenges, seed, timings):
        self.tr = api.Transcript() if challenges is None else None
        self.ch = {} if challenges is None else {name: np.ascontiguousarray(v, dtype=np.uint64) for name, v in challenges.items()}
        self.p = {name: api._p(v) for name, v in self.ch.items()}
        self.host = {"transcript": 0.0}
        self.timings = timings
        self._seed = seed
        self.polys = {}
        self.instances = []
        self.resident = False           # every advice coset in the hot path's coset buffer (set by the advice round)

    def seed(self, i):
        """the blinding seed of slot i, None when the proof is not seeded.  Slots: 0 the advice columns (the hot path), 1 the
        permuted inputs, 2 the permuted tables, 3 the permutation products, 4 the lookup products, 5 the random polynomial."""
        return None if self._seed is None else [int(self._seed), i]

    @contextlib.contextmanager
    def host_transcript(self):
        """wall-clock time of the host's transcript work inside, added to host["transcript"]"""
        t0 = time.perf_counter()
        yield
        self.host["transcript"] += (time.perf_counter() - t0) * 1e3

    @contextlib.contextmanager
    def stage(self, name):
        """device time of the work inside, added to timings[name] — only when timings were asked for: the timer waits for the
        device, and an untimed proof lets the host's transcript work run beside whatever the device still has queued"""
        if self.timings is None:
            yield
            return
        api.timer_start()
        yield
        self.timings[name] = self.timings.get(name, 0.0) + api.timer_stop()

    def squeeze(self, *names):
        if self.tr is not None:
            with self.host_transcript():
                for name in names:
                    self.ch[name] = self.tr.squeeze()
                    self.p[name] = api._p(self.ch[name])

    def write_points(self, points):
        if self.tr is not None and len(points):
            with self.host_transcript():
                self.tr.write_points(np.stack([np.asarray(pt) for pt in points]) if isinstance(points, list) else points)

    def power(self, name, e):
        """challenge^e as a Montgomery element (a fold that skips e terms another rank holds multiplies by it)"""
        return _fr_from_int(pow(_fr_to_int(self.ch[name]), int(e), R_MOD))


class _Fold:
    """position in a sum  sum_i t_i c^(N-1-i)  (c = challenge `challenge` of the proof `pf`, N = n_terms) that this rank folds
    its own terms of, in increasing i, into `acc` (n_elems field elements): `skip_to(i, count)` before terms i .. i + count - 1
    are folded in (acc <- acc c + t_i) multiplies the accumulator by c for every term in between that another rank holds;
    `finish()` for the terms after its last.  On one rank nothing is ever skipped."""

    def __init__(self, lib, pf, challenge, acc, n_elems, n_terms):
        self.lib, self.pf, self.challenge, self.acc, self.n_elems, self.n_terms = lib, pf, challenge, acc, n_elems, n_terms
        self.pos, self.live = 0, False

    def skip_to(self, i, count):
        if self.live and i > self.pos:
            check(self.lib.vdb_poly_scale_dev(self.acc.ptr, api._p(self.pf.power(self.challenge, i - self.pos)), _sz(self.n_elems)))
        assert i >= self.pos or not self.live, "terms are folded in increasing order"
        self.pos, self.live = i + count, True

    def finish(self):
        if self.live and self.n_terms > self.pos:
            check(self.lib.vdb_poly_scale_dev(self.acc.ptr, api._p(self.pf.power(self.challenge, self.n_terms - self.pos)), _sz(self.n_elems)))
        self.pos = self.n_terms


class ProverRounds:
    """`comm`: the exchange steps of a sharded proof (dist.Comm over torch.distributed: RCCL on a multi-GPU node, gloo in the
    tests) when the hot path `hp` holds one rank's column blocks (col_shard = (rank, world)); None for a proof on one GPU.
    Every rank runs the same rounds on its own columns and its own sets of the permutation argument (shardmap.ShardMap) and
    keeps a transcript of its own: commitments and evaluations are exchanged in the global order before they are absorbed, so
    every rank derives the same challenges and ends with the same proof bytes — the bytes a single GPU writes with the same
    blinding scalars.
    Three switches, set on the object before keygen():
    `map_on_device` (True): the device places the constraint map; False = the host builds the maps the device would place.
    `keep_circuit` (False): keep the device's constraint map of a circuit of 2^28 cells or more, which keygen otherwise releases.
    `keep_mapping` (False): keep the permutation's 64-bit mapping in `d_map` after keygen (the tests compare it with the host's)."""

    def __init__(self, hp, block_cols=BLOCK_COLS, comm=None):
        from .dist import LocalComm
        from .shardmap import ShardMap
        self.degree = constraint_degree(hp.n_lk_cols)
        self.chunk_len, self.n_h = self.degree - 2, self.degree - 1
        self.n_slots = self.n_h
        assert block_cols % self.chunk_len == 0
        self.block_cols = block_cols
        self.hp, self.lib = hp, hp.lib
        self.comm = comm if comm is not None else LocalComm()
        self.rank, self.world = hp.rank, hp.world
        assert (self.comm.rank, self.comm.world) == (self.rank, self.world), "the hot path's shard and the communicator disagree"
        self.k, self.rows, self.ne = hp.k, hp.rows, hp.rows * self.n_slots      # ne: points per column of a coset array
        self.usable = hp.rows - N_BLIND
        self.n_adv, self.n_lk, self.n_cols = hp.n_adv_cols, hp.n_lk_cols, hp.n_cols
        self.n_perm = self.n_cols + 2                # the permutation argument's columns: advice, lookup, the constants' fixed column, the instance column
        self.n_sets = -(-self.n_perm // self.chunk_len)
        self.map = ShardMap(hp.shards, self.n_adv, self.n_lk, self.chunk_len)
        (self.a_lo, self.a_hi), (self.l_lo, self.l_hi) = hp.shards[self.rank]
        self.my_adv, self.my_lk = self.a_hi - self.a_lo, self.l_hi - self.l_lo
        self.set_ranges = self.map.set_ranges(self.rank)                       # the sets whose running products this rank computes
        self.sig_ranges = self.map.set_col_ranges(self.rank)                   # their columns: the sigma columns this rank keeps
        self.my_sets = sum(hi - lo for lo, hi in self.set_ranges)
        self.my_sig = sum(hi - lo for lo, hi in self.sig_ranges)
        self.adv_ranges = [(self.a_lo, self.a_hi), (self.n_adv + self.l_lo, self.n_adv + self.l_hi)]      # my columns among all advice + lookup columns
        self.lk_ranges = [(self.l_lo, self.l_hi)]                               # my lookup columns among all lookup columns
        self.foreign = self.map.foreign_cols(self.rank)                        # columns of my sets that another rank holds
        self.stray = self.map.stray_cols(self.rank)                            # my columns that lie in another rank's set
        self.delta = api.fr_delta()
        self.fixed = {}
        self._vk_digest = None
        self.map_on_device, self.keep_circuit, self.keep_mapping = True, False, False
        self.circuit = None             # the constraint map of the last keygen
        # d_key: the key's big buffer [sigma columns of my sets | selectors of my advice columns]; d_map / d_map32: the permutation's
        # mapping in 64 bits per cell (only under keep_mapping) and packed in 32
        self.d_key = self.d_map = self.d_map32 = self.d_inst_cells = None
        self.public_cells = []        # the circuit's default public cells (circuit_map); a key loaded from a file brings its own
        self.instance_cells = []

    # ------------------------------------------------------------------ local positions of global things
    def _col_local(self, p):
        """position of advice / lookup column p (permutation numbering) in the hot path's column buffer [my advice | my lookup]; None: not mine"""
        if self.a_lo <= p < self.a_hi:
            return p - self.a_lo
        if self.l_lo <= p - self.n_adv < self.l_hi:
            return self.my_adv + p - self.n_adv - self.l_lo
        return None

    def _globalize(self, local, ranges, n_total):
        """rows this rank made, placed at `ranges` of an array of n_total rows; the other ranks' rows come with the exchange"""
        local = np.ascontiguousarray(local, dtype=np.uint64)
        if self.world == 1:
            return local
        out = np.zeros((n_total,) + local.shape[1:], dtype=np.uint64)
        off = 0
        for lo, hi in ranges:
            out[lo:hi] = local[off: off + hi - lo]
            off += hi - lo
        return self.comm.sum_disjoint(out)

    # ------------------------------------------------------------------ helpers on device-resident columns
    def _to_coeff(self, lag_buf, n_cols):
        """copy of Lagrange-form columns turned into coefficients"""
        c = api.DeviceBuffer(max(n_cols, 1) * self.rows * B)
        check(self.lib.vdb_memcpy_d2d(c.ptr, lag_buf.ptr, _sz(n_cols * self.rows * B)))
        check(self.lib.vdb_lagrange_to_coeff_dev(c.ptr, _sz(n_cols), self.k))
        return c

    def _to_ext(self, coeff_buf, n_cols):
        e = api.DeviceBuffer(max(n_cols, 1) * self.ne * B)
        check(self.lib.vdb_coeff_to_cosets_dev(coeff_buf.ptr, e.ptr, _sz(n_cols), self.k, self.n_slots, None))
        return e

    def _srs_for(self, n_cols, basis, dense):
        return self.hp.srs if basis == 1 and not dense else (self.srs_few if basis == 0 and n_cols <= 8 else self.srs_m)

    def _commit(self, buf, n_cols, basis, dense=True):
        out = np.zeros((n_cols, 8), dtype=np.uint64)
        if n_cols:
            check(self.lib.vdb_msm_batch_dev(self._srs_for(n_cols, basis, dense).h, basis, buf.ptr, _sz(n_cols), _sz(self.rows), api._p(out)))
        return out

    def _commit_begin(self, buf, n_cols, basis, dense=True):
        """queue the commitment of n_cols columns and return (vdb_msm_batch_masked_dev_begin); _commit_end collects the points"""
        if n_cols:
            check(self.lib.vdb_msm_batch_masked_dev_begin(self._srs_for(n_cols, basis, dense).h, basis, buf.ptr, _sz(n_cols), _sz(self.rows), None, None))

    def _commit_end(self, n_cols):
        out = np.zeros((n_cols, 8), dtype=np.uint64)
        if n_cols:
            check(self.lib.vdb_msm_batch_end(api._p(out), _sz(n_cols)))
        return out

    def _blind(self, buf, n_cols, from_row, seed, ranges=None, n_total=None):
        """uniform field elements into the rows from `from_row` on of every column (halo2 fills them with Scalar::random(rng)
        from OsRng): 64 bytes of entropy each, reduced on the device; `seed` = None draws from the operating system.
        `ranges` / `n_total`: the n_cols columns are those stretches of a set of n_total columns; a seeded stream (test hook) is
        then drawn for the whole set and this rank's part taken, so that a sharded proof blinds as the unsharded one does."""
        cnt = self.rows - from_row
        if n_cols * cnt == 0:
            return
        if seed is None or ranges is None or n_total == n_cols:
            ranges, n_total = [(0, n_cols)], n_cols
        d = api.DeviceBuffer(n_total * cnt * B)
        api.random_scalars_dev(d.ptr, n_total * cnt, seed=seed)
        off = 0
        for lo, hi in ranges:
            if hi > lo:
                check(self.lib.vdb_fill_rows_dev(buf.at(off * self.rows * B), _sz(hi - lo), _sz(self.rows), _sz(from_row), d.at(lo * cnt * B)))
            off += hi - lo
        api.sync()
        d.free()

    def vk_digest(self):
        """The verifying key's entry into the transcript: ONE scalar, as halo2 absorbs vk.transcript_repr (a hash of the key made
        at keygen) — here the squeeze of a sponge of its own over every fixed commitment in FIXED order, computed once per key (the
        38 k points of the k = 16 cosine circuit would otherwise cost every proof 19 k permutations on the host)."""
        if self._vk_digest is None:
            self._vk_digest = protocol.vk_digest({name: self.fixed[name].commits for name in FIXED})
        return self._vk_digest

    def _fixed_poly(self, name, lag_buf, n_cols, keep_lag=True, keep_ext=True, ranges=None, n_total=None):
        """commitment and coefficient form of a fixed polynomial; its extended coset only when it is small (the selector and
        sigma cosets — 4x the columns — are produced block by block inside the quotient instead of being held).  With `ranges`
        the buffer holds this rank's part of a set of n_total polynomials: every rank commits its part, the commitments of the
        whole set are exchanged (they make the verifying key's digest); without, every rank holds the (small) whole."""
        commits = self._commit(lag_buf, n_cols, 1)
        if ranges is not None:
            commits = self._globalize(commits, ranges, n_total)
        if keep_lag:
            coeff = self._to_coeff(lag_buf, n_cols)
        else:                      # transformed where it lies: no second buffer of tens of GB for the sigma columns and the selectors
            check(self.lib.vdb_lagrange_to_coeff_dev(lag_buf.ptr, _sz(n_cols), self.k))
            coeff, lag_buf = lag_buf, None
        p = _Poly(name, n_cols, lag=lag_buf, coeff=coeff, ext=self._to_ext(coeff, n_cols) if keep_ext else None, commits=commits,
                  ranges=ranges, n_total=n_total, replicated=ranges is None)
        self.fixed[name] = p
        return p

    # ------------------------------------------------------------------ keygen side (untimed): the fixed polynomials
    def circuit_map(self, d_flags):
        """The circuit's constraint map (circuit_sym.CopyMap) for the gadget this hot path runs (hp.constraint_map); sets the cells its
        example makes public and the Merkle root's cell (None for a circuit without one).  `map_on_device` = False: the host builds
        the maps the device would place."""
        cm, public, self.root_cell = self.hp.constraint_map(d_flags, self.map_on_device)
        self.public_cells = [int(c) for c in public]
        return cm

    def keygen(self, circuit=None, instance_cells=None, check=True):
        """The Keygen arm's work for the rounds (src/scaffold/mod.rs:267-283 -> keygen_vk / keygen_pk): gate selectors, the
        permutation (sigma columns) from the circuit's constraint map, the constants' fixed column, the range table.
        `circuit`: a circuit_sym.CopyMap over the stream cells; None = the map of the gadget this hot path runs (circuit_map).
        `instance_cells`: the stream cells the closure makes public, in `make_public` order; cell i is tied to row i of the
        instance column by a copy constraint (src/scaffold/mod.rs:400).  None = what the reference's example of this gadget
        exposes (circuit_map: centroids / result vector / root) when the map is the gadget's own, nothing for a map handed in.
        `check`: run the device-side MockProver on the keygen witness with the whole map (vdb_mock_check_dev); the report is
        kept in self.keygen_report (a circuit the witness does not satisfy can still be set up — the proof will not verify)."""
        # the fixed columns' commitments work in the bounded MSM work space of setup (pipeline.HotPath.setup); every step() lifts the bound
        api.msm_scratch_cap(api.KEYGEN_SCRATCH_CAP)
        self._commit_srs()
        d_flags = self.hp.keygen_flags()        # gate selectors from a flag-recording witness run
        cm = self._keygen_circuit(circuit, instance_cells, d_flags)
        if check:
            self.keygen_report = self.mock_check(d_flags)
        d_map = self._build_mapping(cm, *self._permutation_parents(cm))
        self._sigma_columns(d_map)
        self._selector_columns(d_flags)
        self._small_fixed()
        api.sync()
        return self._alloc_working_set()

    def _commit_srs(self):
        """the SRS handles of the commitments the hot path's own does not serve"""
        # the derived columns (products, quotient, opening quotients) and the fixed sigma columns hold full-width scalars
        hp, k = self.hp, self.k
        self.srs_m = api.Srs(k, hp.g_monomial, hp.g_lagrange, window_bits=14)
        self.srs_few = api.Srs(k, hp.g_monomial, None)     # a handful of columns: the bucket folding dominates, fewer buckets win

    def _keygen_circuit(self, circuit, instance_cells, d_flags):
        """the constraint map and the public cells of this keygen (the arguments, or the gadget's own), checked against the hot
        path's circuit; sets self.circuit, self.instance_cells, self.consts"""
        hp = self.hp
        self.public_cells = []
        cm = circuit if circuit is not None else self.circuit_map(d_flags)
        if instance_cells is None:
            instance_cells = self.public_cells
        self.instance_cells = [int(c) for c in instance_cells]
        if len(self.instance_cells) > self.usable or any(not 0 <= c < hp.n_cells for c in self.instance_cells):
            raise ValueError("public cells outside the stream, or more of them than usable rows of the instance column")
        n_src = cm.n_lookup if hasattr(cm, "d_copy_of") else (None if cm.lookup_src is None else len(cm.lookup_src))
        if cm.n_cells != hp.n_cells or (n_src is not None and n_src != hp.n_lookup):
            raise ValueError("the constraint map does not describe this circuit (cell counts differ)")
        self.circuit = cm
        self.consts = [int(v) for v in cm.consts]
        if len(self.consts) > self.usable:
            raise ValueError("more distinct constants than usable rows of the fixed column")
        return cm

    def _permutation_parents(self, cm):
        """The copy forest the permutation is built from: (d_parent, lsrc_ptr, d_lsrc, tie_lookups) — every cell's parent (a cell
        tied to a constant points at the constant's slot behind the cells), the lookup cells' sources (d_lsrc: the upload of a
        host map's, which the caller frees; None for the device's map, which owns them) and whether the lookup columns are tied
        at all.  A map without lookup sources leaves them untied: only the tests' negative cases want that."""
        hp, lib = self.hp, self.lib
        d_parent = api.DeviceBuffer(hp.n_cells * 8)
        if hasattr(cm, "d_copy_of"):
            bad, nosrc = ctypes.c_uint64(), ctypes.c_uint64()
            check(lib.vdb_copymap_finish_dev(cm.d_copy_of.ptr, cm.d_const_idx.ptr, ctypes.c_uint64(hp.n_cells), cm.d_lookup_src.ptr, ctypes.c_uint64(hp.n_lookup),
                                             d_parent.ptr, ctypes.byref(bad), ctypes.byref(nosrc)))
            if bad.value:
                raise ValueError("a cell tied to a constant must be the root of its copies")
            return d_parent, cm.d_lookup_src.ptr, None, bool(hp.n_lookup)
        parent = cm.copy_of.astype(np.int64, copy=True)
        tied = cm.const_idx >= 0
        if (parent[tied] != np.flatnonzero(tied)).any():
            raise ValueError("a cell tied to a constant must be the root of its copies")
        parent[tied] = hp.n_cells + cm.const_idx[tied]
        d_parent.upload(parent)
        del parent
        tie_lookups = bool(hp.n_lookup) and cm.lookup_src is not None
        d_lsrc = None
        if tie_lookups:
            d_lsrc = api.DeviceBuffer(hp.n_lookup * 8)
            d_lsrc.upload(np.ascontiguousarray(cm.lookup_src, dtype=np.int64))
        return d_parent, d_lsrc.ptr if tie_lookups else None, d_lsrc, tie_lookups

    def _build_mapping(self, cm, d_parent, lsrc_ptr, d_lsrc, tie_lookups):
        """The permutation over [advice | lookup | constants | instance]: the cycles of the copy classes, built on the device
        (vdb_permutation_mapping_dev: pointer jumping, one radix sort; copymap.mapping_from_copy_of is the host restatement the
        tests compare it with).  Allocates the key's buffer d_key, frees the parents, releases a large device map, and leaves the
        mapping packed in self.d_map32.  Returns the 64-bit mapping d_map, which the sigma columns are made from."""
        hp, lib, rows, k = self.hp, self.lib, self.rows, self.k
        d_map = api.DeviceBuffer(self.n_perm * rows * 8)
        bp64 = np.ascontiguousarray(hp.bp, dtype=np.uint64)
        self._upload_instance_cells()
        # The key's two big buffers — the sigma columns of my sets, the selectors of my advice columns — are ONE allocation, made
        # before the permutation is built and lent to it for its sort records (51 GiB at C4'): HBM that is mapped once and never handed
        # back (mapping or clearing HBM costs this driver ~30 ms / GiB, vdb_alloc_stats).
        if self.d_key is not None:
            self.d_key.free()
        self.d_key = api.DeviceBuffer(max(self.my_sig + self.my_adv, 1) * rows * B)
        check(lib.vdb_permutation_mapping_ws_dev(d_parent.ptr, ctypes.c_uint64(hp.n_cells), ctypes.c_uint64(len(self.consts)), api._p(bp64), ctypes.c_uint64(len(bp64)), k,
                                                 lsrc_ptr if tie_lookups else None, ctypes.c_uint64(hp.n_lookup if tie_lookups else 0),
                                                 ctypes.c_uint64(rows - MINIMUM_ROWS), ctypes.c_uint64(self.n_cols),
                                                 self.d_inst_cells.ptr, ctypes.c_uint64(len(self.instance_cells)), d_map.ptr,
                                                 self.d_key.ptr, _sz(self.d_key.nbytes)))
        d_parent.free()
        if d_lsrc is not None:
            d_lsrc.free()
        if hasattr(cm, "d_copy_of") and hp.n_cells >= (1 << 28) and not self.keep_circuit:
            cm.free()                    # tens of GB at BASELINE sizes: the proof needs the room; small circuits keep their map (tests, mock_check)
        self.d_map = d_map if self.keep_mapping else None
        # the mapping stays with the key in 32 bits per cell when column and row fit: the product round makes the sigma columns'
        # Lagrange form from it (one product per cell) instead of transforming their coefficient form back
        self.d_map32 = None
        if (self.n_perm - 1).bit_length() + k <= 32:
            self.d_map32 = api.DeviceBuffer(self.n_perm * rows * 4)
            check(lib.vdb_permutation_mapping_pack_dev(d_map.ptr, _sz(self.n_perm), k, self.d_map32.ptr))
            api.sync()
        if self.world > 1 and self.d_map32 is None:
            raise ValueError("a sharded key keeps the packed mapping: column and row of a cell must fit 32 bits")
        return d_map

    def _sigma_columns(self, d_map):
        """the sigma columns of my sets, into the front of d_key: every rank builds the cycles of the whole circuit (the copy
        classes cross all columns) and keeps the columns of its own sets; frees d_map unless keep_mapping holds it"""
        lib, rows, k = self.lib, self.rows, self.k
        d_sigma = _View(self.d_key, 0, self.my_sig * rows * B)
        off = 0
        for lo, hi in self.sig_ranges:
            check(lib.vdb_permutation_sigma_dev(d_map.at(lo * rows * 8), _sz(hi - lo), k, api._p(self.delta), d_sigma.at(off * rows * B))
                  if self.world == 1 else
                  lib.vdb_permutation_sigma_packed_dev(self.d_map32.at(lo * rows * 4), _sz(hi - lo), _sz(self.n_perm), k, api._p(self.delta), d_sigma.at(off * rows * B)))
            off += hi - lo
        if self.d_map is None:
            d_map.free()
        self._fixed_poly("sigma", d_sigma, self.my_sig, keep_lag=False, keep_ext=False, ranges=self.sig_ranges, n_total=self.n_perm)

    def _selector_columns(self, d_flags):
        """the gate selectors of my advice columns, behind the sigma columns in d_key (after the permutation's work space is
        gone: both are tens of GB at BASELINE sizes); frees d_flags"""
        hp, lib, rows = self.hp, self.lib, self.rows
        d_mine = _View(self.d_key, self.my_sig * rows * B, self.my_adv * rows * B)
        # a rank of a sharded run lays out every column's selectors and keeps its own
        d_all = d_mine if self.my_adv == self.n_adv else api.DeviceBuffer(self.n_adv * rows * B)
        check(lib.vdb_layout_selectors_dev(d_flags.ptr, ctypes.c_uint64(hp.n_cells), api._p(hp.bp), ctypes.c_uint64(len(hp.bp)), self.k, d_all.ptr))
        d_flags.free()
        if d_all is not d_mine:
            check(lib.vdb_memcpy_d2d(d_mine.ptr, d_all.at(self.a_lo * rows * B), _sz(self.my_adv * rows * B)))
            api.sync()
            d_all.free()
        self._fixed_poly("sel", d_mine, self.my_adv, keep_lag=False, keep_ext=False, ranges=[(self.a_lo, self.a_hi)], n_total=self.n_adv)

    def _small_fixed(self):
        """the three small fixed polynomials every rank holds whole: the constants' column, the range table, the Lagrange selectors"""
        hp, rows = self.hp, self.rows
        # the constants' fixed column: constant r at row r (halo2-base assigns the distinct constants of a circuit to fixed cells
        # and ties every Constant advice cell to its fixed cell through the permutation)
        cst = np.zeros((rows, 4), dtype=np.uint64)
        cst[: len(self.consts)] = _consts_table(self.consts)
        d_cst = api.DeviceBuffer(rows * B)
        d_cst.upload(cst)
        self._fixed_poly("cst", d_cst, 1)
        self._place_cst_coset()
        # range table 0 .. 2^L - 1, zero below
        tab = np.arange(rows, dtype=np.uint64)
        tab[tab >= (1 << hp.L)] = 0
        d_tab = api.DeviceBuffer(rows * B)
        d_tab.upload(api.fr_from_canonical(np.stack([tab, np.zeros_like(tab), np.zeros_like(tab), np.zeros_like(tab)], axis=1)))
        self._fixed_poly("table", d_tab, 1)
        lag = self._lagrange_selectors()
        d_l = api.DeviceBuffer(lag.nbytes)
        d_l.upload(lag)
        self._fixed_poly("lag", d_l, 3)

    def _lagrange_selectors(self):
        """l0, l_last, l_active in Lagrange form (3, rows, 4): one at row 0, at the first unusable row, on every usable row"""
        lag = np.zeros((3, self.rows, 4), dtype=np.uint64)
        one = _fr_from_int(1)
        lag[0, 0], lag[1, self.usable], lag[2, : self.usable] = one, one, one
        return lag

    def _place_cst_coset(self):
        """the constants' coset sits behind the advice cosets, the instance column's behind it (the permutation term of the quotient
        reads one contiguous block of columns)"""
        hp = self.hp
        if hp.ext_cols >= self.my_adv + self.my_lk + 2:
            check(self.lib.vdb_memcpy_d2d(hp.d_ext.at((self.my_adv + self.my_lk) * self.ne * B), self.fixed["cst"].ext.ptr, _sz(self.ne * B)))

    def _upload_instance_cells(self):
        cells = np.asarray(self.instance_cells, dtype=np.int64)
        if self.d_inst_cells is not None:      # a second keygen / key load on the same object
            self.d_inst_cells.free()
        self.d_inst_cells = api.DeviceBuffer(max(cells.nbytes, 32))
        if cells.nbytes:
            self.d_inst_cells.upload(cells)

    def _instance_values(self, instances):
        """`instances` (canonical integers, one per public cell of keygen) as Montgomery field elements, (max(n, 1), 4)"""
        if len(instances) != len(self.instance_cells):
            raise ValueError("one value per public cell")
        vals = np.zeros((max(len(instances), 1), 4), dtype=np.uint64)
        if len(instances):
            vals[: len(instances)] = np.stack([_fr_from_int(int(v)) for v in instances])
        return vals

    def mock_check(self, d_flags=None, instances=None):
        """The Mock stage on the witness in HBM with this circuit's whole constraint map (vdb_mock_check_dev): gate rows, the
        range table, every copy, every lookup source, every constant and asserted constant — and, with `instances` (canonical
        integers, one per public cell: MockProver::run's third argument), every public cell against the value claimed for it.
        api.MockReport."""
        hp = self.hp
        cm = self.circuit
        own = d_flags is None
        if own:
            d_flags = hp.keygen_flags()
            shard, hp.shard_witness = hp.shard_witness, False      # the check walks the whole witness, whatever this rank's columns
            try:
                hp._witness()
            finally:
                hp.shard_witness = shard
        bufs = []

        def dev(a, dtype):
            a = np.ascontiguousarray(a, dtype=dtype)
            b = api.DeviceBuffer(max(a.nbytes, 32))
            if a.nbytes:
                b.upload(a)
            bufs.append(b)
            return b
        try:
            if hasattr(cm, "d_copy_of"):
                if cm.d_copy_of is None:
                    raise RuntimeError("the circuit's constraint map was released after keygen (set keep_circuit = True before keygen to keep it)")
                d_copy, d_cidx, d_lsrc = cm.d_copy_of, cm.d_const_idx, cm.d_lookup_src if hp.n_lookup else None
            else:
                d_copy = dev(cm.copy_of, np.int64)
                d_lsrc = dev(cm.lookup_src, np.int64) if hp.n_lookup and cm.lookup_src is not None else None
                d_cidx = dev(cm.const_idx, np.int64)
            tab = np.zeros((max(len(cm.consts), 1), 4), dtype=np.uint64)
            tab[: len(cm.consts)] = _consts_table(cm.consts)
            d_tab = dev(tab, np.uint64)
            rep = api.mock_check_dev(hp.d_stream.ptr, hp.n_cells, d_flags.ptr, hp.d_lookup.ptr, hp.n_lookup, hp.L, d_copy.ptr,
                                     None if d_lsrc is None else d_lsrc.ptr, None, d_cidx.ptr, d_tab.ptr, len(cm.consts))
            if instances is not None:
                vals = self._instance_values(instances)
                api.mock_check_instances_dev(rep, hp.d_stream.ptr, hp.n_cells, dev(self.instance_cells, np.int64).ptr, dev(vals, np.uint64).ptr, len(instances))
            return rep
        finally:
            for b in bufs:
                b.free()
            if own:
                d_flags.free()

    def mock_check_instances(self, instances):
        """The `instances` argument of MockProver::run alone, on the witness in HBM (vdb_mock_check_instances_dev): public cell i of
        keygen must hold instances[i] (canonical integers).  Needs no constraint map, so it also serves after keygen released the
        map of a BASELINE-size circuit.  api.MockReport with only the instance fields filled."""
        vals = self._instance_values(instances)
        rep = api.MockReport()
        if not len(instances):
            return rep
        d_vals = api.DeviceBuffer(vals.nbytes)
        try:
            d_vals.upload(vals)
            api.mock_check_instances_dev(rep, self.hp.d_stream.ptr, self.hp.n_cells, self.d_inst_cells.ptr, d_vals.ptr, len(instances))
        finally:
            d_vals.free()
        return rep

    def _alloc_working_set(self):
        lib, rows, CHUNK_LEN = self.lib, self.rows, self.chunk_len
        # The working set of prove(), allocated once (device allocations of tens of GB take seconds): the derived columns
        # [pa | ps | zp | zl] (Lagrange, then coefficient form in place), the lookup columns laid out, and block buffers of
        # `block_cols` columns — two in Lagrange form (the permutation's columns and their sigma columns), two of extended
        # cosets, one of product cosets — through which every per-column stage streams.  The library's MSM scratch is released
        # first so that it is re-sized to what is left.
        if api.scratch_held() > 2 * api.KEYGEN_SCRATCH_CAP:      # a hot path that has proved already holds the prover's big work space
            check(lib.vdb_scratch_release())
        n_der = 3 * self.my_lk + self.my_sets
        blk = max(2 * CHUNK_LEN, min(self.block_cols, -(-max(self.my_sig, 1) // (2 * CHUNK_LEN)) * (2 * CHUNK_LEN)) // (2 * CHUNK_LEN) * (2 * CHUNK_LEN))
        self.blk_alloc = blk
        self.pool_der = api.DeviceBuffer(max(n_der, 1) * rows * B)
        self.d_pa, self.d_ps, self.d_zp, self.d_zl = (_View(self.pool_der, lo * rows * B, m * rows * B) for lo, m in
                                                      ((0, self.my_lk), (self.my_lk, self.my_lk), (2 * self.my_lk, self.my_sets), (2 * self.my_lk + self.my_sets, self.my_lk)))
        self.d_lklag = api.DeviceBuffer(max(self.my_lk, 1) * rows * B)
        # what a sharded proof receives from other ranks: the columns that complete the set spanning the advice / lookup junction
        # (Lagrange and coefficient form), one boundary product polynomial per requested set
        self.z_req = self.map.z_requests(self.rank)
        self.foreign_slot = {c: i for i, c in enumerate(self.foreign)}          # positions in d_foreign_lag / d_foreign_coeff
        self.z_slot = {i: j for j, i in enumerate(self.z_req)}                  # positions in d_zhalo
        self.all_foreign = self.map.all_foreign_cols() if self.world > 1 else []     # what the ranks send each other
        self.all_z = self.map.all_z_requests() if self.world > 1 else []
        self.l_cosets = tuple(self.fixed["lag"].ext.at(i * self.ne * B) for i in range(3))     # l0, l_last, l_active
        self.d_foreign_lag = api.DeviceBuffer(max(len(self.foreign), 1) * rows * B)
        self.d_foreign_coeff = api.DeviceBuffer(max(len(self.foreign), 1) * rows * B)
        self.d_zhalo = api.DeviceBuffer(max(len(self.z_req), 1) * rows * B)
        self.d_lag_a, self.d_lag_s = api.DeviceBuffer(blk * rows * B), api.DeviceBuffer(blk * rows * B)
        self.d_ea, self.d_eb = api.DeviceBuffer(blk * self.ne * B), api.DeviceBuffer(blk * self.ne * B)
        self.d_ez = api.DeviceBuffer((blk // CHUNK_LEN + 1) * self.ne * B)
        self.d_zf, self.d_zlast = api.DeviceBuffer(self.ne * B), api.DeviceBuffer(self.ne * B)
        self.d_h, self.d_h2, self.d_h3, self.d_h4 = (api.DeviceBuffer(self.ne * B) for _ in range(4))
        self.d_hg = api.DeviceBuffer(GATE_SLOTS * rows * B)         # the gates' accumulator, on the coset of 2 n points
        self.d_comb, self.d_quot = api.DeviceBuffer(rows * B), api.DeviceBuffer(rows * B)
        # the instance column: Lagrange form (the public values in rows 0 .. n_instances - 1, zero below), coefficients, coset —
        # made anew for every proof from the values of the statement
        self.d_inst_lag, self.d_inst_coeff, self.d_inst_ext = api.DeviceBuffer(rows * B), api.DeviceBuffer(rows * B), api.DeviceBuffer(self.ne * B)
        self.d_rand, self.d_hf = api.DeviceBuffer(rows * B), api.DeviceBuffer(rows * B)       # the vanishing argument's random polynomial, h folded at x
        check(lib.vdb_memset_dev(self.d_inst_lag.ptr, 0, _sz(rows * B)))
        self._vk_digest = None
        self.vk_digest()            # part of the key, made here so that no proof pays for it
        self._keep_fixed_cosets()
        return self

    def _keep_fixed_cosets(self):
        """The cosets of the fixed polynomials that every proof would otherwise transform again — the sigma columns (n_slots cosets
        each) and the selectors (two) — stay in HBM when they fit beside the working set with room to spare for the MSM's work space:
        halo2's ProvingKey holds them too (fixed_cosets, permutation cosets).  They fit on a rank of a multi-GPU job and for circuits
        up to a few thousand columns; BASELINE C4' on one card (20,969 columns: 126 + 36 GB) streams them block by block as before."""
        lib, rows = self.lib, self.rows
        self.fixed_cosets_resident = False
        need = (self.my_sig * self.ne + self.my_adv * GATE_SLOTS * rows) * B
        free, _total = api.mem_info()
        free += api.scratch_held()          # the work space already allocated counts towards the reserve kept for it
        reserve = int(os.environ.get("VDB_FIXED_COSETS_RESERVE_GB", "48")) << 30
        if os.environ.get("VDB_FIXED_COSETS", "1") != "0" and free - need >= reserve:
            sig, sel = self.fixed["sigma"], self.fixed["sel"]
            sig.ext = api.DeviceBuffer(max(self.my_sig * self.ne, 1) * B)
            check(lib.vdb_coeff_to_cosets_dev(sig.coeff.ptr, sig.ext.ptr, _sz(self.my_sig), self.k, self.n_slots, None))
            sel.ext = api.DeviceBuffer(max(self.my_adv * GATE_SLOTS * rows, 1) * B)
            check(lib.vdb_coeff_to_cosets_dev(sel.coeff.ptr, sel.ext.ptr, _sz(self.my_adv), self.k, GATE_SLOTS, None))
            api.sync()
            self.fixed_cosets_resident = True

    # ------------------------------------------------------------------ the proving key on disk
    def save_verifying_key(self, path, opened=None):
        """What the Keygen arm writes beside the proving key (src/scaffold/mod.rs:276-281: data/{name}.vk) in this build's own
        container (upstream's is SerdeFormat::RawBytes of halo2's VerifyingKey: parity unpinned): the circuit's shape, the commitments
        of the fixed polynomials in FIXED order, the transcript digest made of them, the SRS scalar of the deterministic "unsafe"
        setup the reference's gen_srs uses (a verifier derives [tau]_2 from it) — or, for an SRS from a params file, whose scalar nobody
        knows, its G2 points tau_g2 = [tau]_2 and g2 instead —, and — when a proof's `opened` map is given — which polynomial is opened
        at which rotation.  io.read_verifying_key reads it."""
        from .io import write_verifying_key
        meta = protocol.key_meta(self.k, self.n_adv, self.n_lk, len(self.instance_cells))
        meta["delta"] = str(meta["delta"])
        if self.hp.tau is not None:
            meta["tau"] = str(self.hp.tau)
        else:
            meta["tau_g2"] = [str(int(w)) for w in self.hp.tau_g2]
            meta["g2"] = [str(int(w)) for w in self.hp.g2]
        meta["vk_digest"] = str(_fr_to_int(self.vk_digest()))
        if opened is not None:
            meta["opened"] = {str(rot): list(names) for rot, names in opened.items()}
        write_verifying_key(path, meta, {name: self.fixed[name].commits for name in FIXED})

    def _key_header(self):
        """what a proving-key file must agree on with the run that loads it: the circuit's shape and, for a sharded key, this rank's
        place in the partition (rank, world, every rank's column blocks)"""
        shards = np.asarray([[a[0], a[1], l[0], l[1]] for a, l in self.hp.shards], dtype=np.int64)
        return (np.array([self.k, self.n_adv, self.n_lk, self.hp.L, self.chunk_len, N_BLIND, self.rank, self.world], dtype=np.uint64), shards)

    def save_proving_key(self, path):
        """What the reference's Keygen arm leaves for the Prove arm (src/scaffold/mod.rs:272-281: pinning + pk), in this
        build's own container: an .npz (numpy.load with allow_pickle=False reads it) holding the circuit's shape, the break
        points, and per fixed polynomial — gate selectors, sigma columns, constants, range table, Lagrange selectors — its coefficient
        form and its commitments.  Upstream's pk file format (SerdeFormat::RawBytes) is not reproduced: parity unpinned.
        Sharded (world > 1): every rank writes a file of its own (the caller names it per rank) with the selectors of its advice
        columns and the sigma columns of its sets, beside the whole set's commitments and the replicated small polynomials; the
        header records the partition, and load_proving_key refuses a file written for another rank or other column blocks."""
        api.sync()
        meta, shards = self._key_header()
        doc = {"meta": meta, "shards": shards, "break_points": np.asarray(self.hp.bp, dtype=np.uint64)}
        doc["instance_cells"] = np.asarray(self.instance_cells, dtype=np.int64)
        doc["instance_cells_are_the_default"] = np.array([int(self.instance_cells == [int(c) for c in self.public_cells])], dtype=np.int64)
        for name, q in self.fixed.items():
            doc[name + "_coeff"] = q.coeff.download((max(q.n_cols, 1), self.rows, 4))[: q.n_cols]
            doc[name + "_commits"] = q.commits
        np.savez(path, **doc)

    def load_proving_key(self, path):
        """The Prove arm's side: the fixed polynomials from a file written by save_proving_key instead of a keygen run (no
        flag-recording witness pass, no permutation construction).  The Lagrange forms the rounds read (sigma, table) are
        recovered with a forward transform; raises ValueError when the file describes another circuit, another rank or another
        partition of the columns."""
        with np.load(path, allow_pickle=False) as doc:
            meta, shards = self._key_header()
            if not np.array_equal(doc["meta"], meta) or not np.array_equal(doc["shards"], shards) \
                    or not np.array_equal(doc["break_points"], np.asarray(self.hp.bp, dtype=np.uint64)):
                raise ValueError("proving key does not describe this circuit (shape, break points, rank or column blocks differ)")
            return self._install_key(doc)

    def _install_key(self, doc):
        """doc[name + "_coeff"], doc[name + "_commits"] for every fixed polynomial, doc["instance_cells"]: the key's polynomials go
        to the device in the forms the rounds read"""
        lib, rows, k = self.lib, self.rows, self.k
        self._commit_srs()
        omega = api.root_of_unity(k)
        # (name, polynomials held here, their place in the whole set, size of the whole set, Lagrange form kept, cosets kept)
        plan = (("sel", self.my_adv, [(self.a_lo, self.a_hi)], self.n_adv, False, False), ("sigma", self.my_sig, self.sig_ranges, self.n_perm, False, False),
                ("cst", 1, None, 1, True, True), ("table", 1, None, 1, True, True), ("lag", 3, None, 3, False, True))
        for name, n_cols, ranges, n_total, need_lag, keep_ext in plan:
            coeff_h = np.ascontiguousarray(doc[name + "_coeff"])
            commits = np.ascontiguousarray(doc[name + "_commits"])
            if coeff_h.shape != (n_cols, rows, 4) or commits.shape != (n_total, 8):
                raise ValueError("proving key: wrong shape for " + name)
            coeff = api.DeviceBuffer(max(coeff_h.nbytes, 32))
            if coeff_h.nbytes:
                coeff.upload(coeff_h)
            lag = None
            if need_lag:
                lag = api.DeviceBuffer(coeff_h.nbytes)
                check(lib.vdb_memcpy_d2d(lag.ptr, coeff.ptr, _sz(coeff_h.nbytes)))
                check(lib.vdb_ntt_batch_dev(lag.ptr, _sz(n_cols), k, api._p(omega), 0))
            self.fixed[name] = _Poly(name, n_cols, lag=lag, coeff=coeff, ext=self._to_ext(coeff, n_cols) if keep_ext else None, commits=commits,
                                     ranges=ranges, n_total=n_total, replicated=ranges is None)
        self.instance_cells = [int(c) for c in doc["instance_cells"]]      # the public cells come with the key
        if int(doc["instance_cells_are_the_default"][0]):
            self.public_cells = list(self.instance_cells)
        self._upload_instance_cells()
        self._place_cst_coset()
        api.sync()
        return self._alloc_working_set()

    # upstream's own key files ------------------------------------------------------------------------------------------------
    RAW_FIXED = ("table", "cst", "sel")     # halo2-base creates the fixed columns in this order (io.py, [UPSTREAM-RECALL])
    RAW_BLOCK = 64                          # polynomials converted and written at a time

    @property
    def raw_ext_k(self):
        """halo2's extended domain has 2^(k + ceil(log2(degree - 1))) points: 4n for the circuits with lookups (degree 4), 2n without
        (the rounds here evaluate on degree - 1 cosets of size n instead, self.ne points per column)"""
        return int(self.chunk_len).bit_length()

    def _raw_blocks(self, names, form):
        """The polynomials of `names`, in order, as host blocks of at most RAW_BLOCK: form "coeff", "lagrange" (values over the
        2^k domain) or "extended" (values over the 4n coset, halo2's ExtendedLagrangeCoeff)"""
        omega = api.root_of_unity(self.k)
        for name in names:
            q = self.fixed[name]
            for lo in range(0, q.n_cols, self.RAW_BLOCK):
                m = min(self.RAW_BLOCK, q.n_cols - lo)
                coeff = q.coeff.download((m, self.rows, 4), offset=lo * self.rows * B)
                yield coeff if form == "coeff" else api.ntt_batch(coeff, omega) if form == "lagrange" else api.coeff_to_extended(coeff, self.raw_ext_k)

    def _write_vk_raw(self, f):
        from .io import write_vk_raw
        if self.world != 1:
            raise ValueError("upstream's key files describe the whole circuit: write them from a one-rank keygen (save_proving_key writes a rank's share)")
        api.sync()
        fixed = np.concatenate([self.fixed[name].commits for name in self.RAW_FIXED])
        write_vk_raw(f, self.k, fixed, self.fixed["sigma"].commits, (np.any(v != 0, axis=2) for v in self._raw_blocks(("sel",), "lagrange")))

    def save_verifying_key_raw(self, path):
        """data/{name}.vk as the reference's Keygen arm writes it (src/scaffold/mod.rs:276-281): halo2's
        `VerifyingKey::write(.., SerdeFormat::RawBytes)` layout (io.py restates it; [UPSTREAM-RECALL], parity unpinned) — k, the fixed
        columns' commitments (table, constants, one per gate selector), the sigma commitments, the selectors' bits.
        io.read_verifying_key_raw reads it back; tests/verify_file.py verifies a proof against it."""
        with open(path, "wb") as f:
            self._write_vk_raw(f)

    def save_proving_key_raw(self, path):
        """data/{name}.pk as snark-verifier-sdk's gen_pk leaves it for read_pk (src/scaffold/mod.rs:273, :325-331): halo2's
        `ProvingKey::write` layout — the verifying key; l_0, l_last, l_active_row over the extended domain; every fixed column as
        values, coefficients and extended coset; the sigma columns likewise.  Written a block of polynomials at a time (the cosets are
        made for the file only: 6 x 2^k x 32 bytes per column, which is why upstream's later versions dropped them from the key).
        The break points and the public cells are not part of it — they travel in the pinning file (io.write_pinning) and with the
        circuit, as upstream."""
        from .io import write_poly_raw, write_polys_raw
        with open(path, "wb") as f:
            self._write_vk_raw(f)
            for poly in next(self._raw_blocks(("lag",), "extended")):
                write_poly_raw(f, poly)
            n_fixed = sum(self.fixed[name].n_cols for name in self.RAW_FIXED)
            for form in ("lagrange", "coeff", "extended"):
                write_polys_raw(f, self._raw_blocks(self.RAW_FIXED, form), n_fixed)
            for form in ("lagrange", "coeff", "extended"):
                write_polys_raw(f, self._raw_blocks(("sigma",), form), self.n_perm)

    def load_proving_key_raw(self, path, instance_cells=None):
        """The Prove arm reading upstream's pk layout (custom_read_pk, src/scaffold/mod.rs:325-331): commitments and coefficient
        forms come from the file, the extended cosets are skipped over and re-derived on the device, l_0 / l_last / l_active are
        checked against this circuit's.  `instance_cells`: as in keygen (None = the gadget's own public cells, which a circuit map
        the circuit's constraint map names).  Raises ValueError when the file is not a key of this circuit."""
        from .io import read_vk_raw, read_poly_raw, read_polys_raw
        if self.world != 1:
            raise ValueError("upstream's key files describe the whole circuit: load them on one rank")
        rows, ne = self.rows, self.rows << self.raw_ext_k
        with open(path, "rb") as f:
            vk = read_vk_raw(f, self.n_perm, self.n_adv)
            if vk["k"] != self.k or len(vk["fixed_commitments"]) != self.n_adv + 2:
                raise ValueError("proving key does not describe this circuit (k or the number of fixed columns differ)")
            lag_ext = np.stack([read_poly_raw(f, ne) for _ in range(3)])
            read_polys_raw(f, self.n_adv + 2, rows, keep=False)
            fixed = read_polys_raw(f, self.n_adv + 2, rows)
            read_polys_raw(f, self.n_adv + 2, ne, keep=False)
            read_polys_raw(f, self.n_perm, rows, keep=False)
            sigma = read_polys_raw(f, self.n_perm, rows)
            read_polys_raw(f, self.n_perm, ne, keep=False)
            if f.read(1):
                raise ValueError("proving key: bytes after the permutation's cosets")
        lag_coeff = api.lagrange_to_coeff(self._lagrange_selectors())
        if not np.array_equal(api.coeff_to_extended(lag_coeff, self.raw_ext_k), lag_ext):
            raise ValueError("proving key: l_0, l_last, l_active_row are not this circuit's (another number of blinding rows?)")
        sel_bits = np.any(api.ntt_batch(fixed[2:], api.root_of_unity(self.k)) != 0, axis=2) if self.n_adv else np.zeros((0, rows), dtype=bool)
        if not np.array_equal(sel_bits, vk["selectors"]):
            raise ValueError("proving key: the selectors' bits are not where the selector columns are non-zero")
        if instance_cells is None:
            if not self.public_cells:
                d_flags = self.hp.keygen_flags()       # the circuit's own public cells: from its constraint map, as keygen takes them
                self.circuit_map(d_flags)
                d_flags.free()
            instance_cells = self.public_cells
        fc = vk["fixed_commitments"]
        doc = {"table_coeff": fixed[0:1], "cst_coeff": fixed[1:2], "sel_coeff": fixed[2:], "sigma_coeff": sigma, "lag_coeff": lag_coeff,
               "table_commits": fc[0:1], "cst_commits": fc[1:2], "sel_commits": fc[2:], "sigma_commits": vk["permutation_commitments"],
               "lag_commits": np.zeros((3, 8), dtype=np.uint64),
               "instance_cells": np.asarray(instance_cells, dtype=np.int64),
               "instance_cells_are_the_default": np.array([int(list(instance_cells) == list(self.public_cells))])}
        return self._install_key(doc)

    # ------------------------------------------------------------------ the rounds
    def prove(self, challenges=None, seed=None, timings=None, multiopen="shplonk", instances=None):
        """challenges: dict of Montgomery field elements beta, gamma, y, x, v, or None to derive them with the Fiat–Shamir
        transcript (api.Transcript; the proof bytes are then returned as `proof`).  Transcript order: the verifying key's
        digest (vk_digest: one scalar made of the fixed commitments at keygen); the public inputs; advice commitments -> theta (squeezed as halo2 does, unused: the lookups
        are single-column); permuted input / table commitments -> beta, gamma; product commitments, the vanishing argument's random
        polynomial -> y; the quotient's pieces -> x; all evaluations, rotation by rotation (not h's: h is folded at x and its value follows
        from the quotient identity, halo2's vanishing argument) -> then the multi-open: "gwc": v, one quotient per rotation
        point; "shplonk" (what the reference's gen_snark_shplonk runs, [UPSTREAM-RECALL] for the order of its challenges):
        yo, v; the quotient f of all rotation sets; u; the quotient of the linearisation polynomial.
        Each round is a method of its own on the proof's state (_Proof), called below in that order.
        `instances`: the public values, one per public cell of keygen (Montgomery field elements); None = read from the witness
        this proof commits to (the honest prover's statement: circuit.instances(), src/scaffold/mod.rs:265).  They fill rows
        0 .. of the instance column, which the permutation argument ties to the public cells.
        Returns dict(commitments, evals, openings, points, proof, challenges, opened, instances): commitments[name] (n, 8); evals[(name,
        rotation)] list of ints; openings: "gwc": list of dict(rotation, point, polys=[names in combination order], eval, W), or _shplonk's.
        `seed`: None = every blinding scalar of this proof (advice, lookup and product columns) comes fresh from the
        operating system's entropy, as in halo2's create_proof; an integer makes the proof reproducible (tests).
        Sharded (world > 1, SHPLONK only): every rank calls prove() with the same arguments; each works on its own columns and
        sets and all end with the same proof bytes (see the class docstring and shardmap.py)."""
        if self.world > 1 and multiopen != "shplonk":
            raise ValueError("the sharded rounds open with SHPLONK")
        pf = _Proof(challenges, seed, timings)
        self.host_ms = pf.host          # wall-clock ms the host spent in the sponge (read by the benches)
        if pf.tr is not None:
            pf.tr.common_scalar(self.vk_digest())
        self._advice(pf, instances)
        pf.omega = api.root_of_unity(self.k)        # (the products round's sigma columns of a key loaded from a file)
        self._lookup_permuted(pf)
        self._receive_foreign()
        self._products(pf)
        self._random_poly(pf)
        self._receive_boundary_products()
        self._quotient(pf)
        self._fold_h(pf)
        allp = {**pf.polys, **self.fixed}
        opened = protocol.opened(self.n_lk)
        points = protocol.rotation_points(_fr_to_int(pf.ch["x"]), self.k, opened)
        evals = self._evaluations(pf, allp, opened, points)
        if multiopen == "shplonk":
            openings = self._shplonk(pf, allp, opened, points, evals)
        else:
            openings = self._open_gwc(pf, allp, opened, points)
        proof = None
        if pf.tr is not None:
            proof = pf.tr.proof()
            pf.tr.free()
        api.sync()
        return dict(commitments={name: q.commits for name, q in allp.items()}, evals=_Evals(evals), openings=openings, points=points,
                    proof=proof, challenges={name: v.copy() for name, v in pf.ch.items()}, opened=opened,
                    instances=[_fr_to_int(v) for v in pf.instances])

    # ------------------------------------------------------------------ the permutation's columns, block by block
    @property
    def _blk(self):
        """columns per block of the streamed stages: `block_cols` (a caller may lower it after keygen) within the blocks allocated"""
        two = 2 * self.chunk_len
        return max(two, min(self.block_cols, self.blk_alloc) // two * two)

    def _runs(self, c0, nb):
        """the permutation's columns c0 .. c0 + nb cut into stretches of one kind: (kind, first column, count) with kind
        "adv" / "lk" (this rank's), "foreign" (another rank's, received), "cst", "inst" """
        out = []
        for c in range(c0, c0 + nb):
            kind = ("cst" if c == self.n_cols else "inst" if c == self.n_cols + 1 else "adv" if self.a_lo <= c < self.a_hi else
                    "lk" if self.l_lo <= c - self.n_adv < self.l_hi else "foreign")
            if kind == "foreign" and c not in self.foreign_slot:
                raise AssertionError("a column of this rank's sets that nobody sent")
            if out and out[-1][0] == kind and kind not in ("cst", "inst") and (kind != "foreign" or self.foreign_slot[c] == self.foreign_slot[c - 1] + 1):
                out[-1][2] += 1
            else:
                out.append([kind, c, 1])
        return out

    def _lagrange_block(self, c0, nb, dest):
        """the permutation's columns c0 .. c0 + nb in Lagrange form: advice from the stream, lookup from their laid-out copy, constants, instances"""
        hp, lib, rows = self.hp, self.lib, self.rows
        for kind, c, m in self._runs(c0, nb):
            to = dest.at((c - c0) * rows * B)
            if kind == "adv":
                check(lib.vdb_layout_columns_range_dev(hp.d_stream.ptr, ctypes.c_uint64(hp.n_cells), api._p(hp.bp), ctypes.c_uint64(len(hp.bp)), self.k,
                                                       ctypes.c_uint64(c), ctypes.c_uint64(c + m), to, hp.d_blind.ptr, N_BLIND))
            else:
                src = (self.d_lklag.at((c - self.n_adv - self.l_lo) * rows * B) if kind == "lk" else self.d_foreign_lag.at(self.foreign_slot[c] * rows * B)
                       if kind == "foreign" else self.fixed["cst"].lag.ptr if kind == "cst" else self.d_inst_lag.ptr)
                check(lib.vdb_memcpy_d2d(to, src, _sz(m * rows * B)))

    def _local_ext_index(self, c):
        """position of permutation column c in the hot path's coset buffer [my advice | my lookup | constants | instance], None: not there"""
        if c >= self.n_cols:
            return self.my_adv + self.my_lk + c - self.n_cols
        return self._col_local(c)

    def _adv_ext_block(self, pf, c0, nb):
        """(pointer, first column) of a buffer that holds the cosets of the permutation's columns c0 .. c0 + nb"""
        hp, ne = self.hp, self.ne
        if pf.resident:
            loc = [self._local_ext_index(c) for c in range(c0, c0 + nb)]
            if None not in loc and loc == list(range(loc[0], loc[0] + nb)):
                return hp.d_ext.ptr, c0 - loc[0]
        for kind, c, m in self._runs(c0, nb):
            to = self.d_ea.at((c - c0) * ne * B)
            if kind in ("adv", "lk"):
                if pf.resident:
                    check(self.lib.vdb_memcpy_d2d(to, hp.d_ext.at(self._col_local(c) * ne * B), _sz(m * ne * B)))
                else:
                    self._ext_into(hp.d_cols.at(self._col_local(c) * self.rows * B), to, m)
            elif kind == "foreign":
                self._ext_into(self.d_foreign_coeff.at(self.foreign_slot[c] * self.rows * B), to, m)
            else:
                check(self.lib.vdb_memcpy_d2d(to, (self.fixed["cst"].ext if kind == "cst" else self.d_inst_ext).ptr, _sz(ne * B)))
        return self.d_ea.ptr, c0

    def _col_ptr(self, base, col0, c):
        return ctypes.c_void_p(base.value + (c - col0) * self.ne * B)

    def _ext_into(self, coeff_ptr, dest_ptr, m):
        check(self.lib.vdb_coeff_to_cosets_dev(coeff_ptr, dest_ptr, _sz(m), self.k, self.n_slots, None))

    def _z_coeff(self, i):
        """coefficient form of product polynomial i: mine, or the copy its owner sent"""
        if i in self.z_slot:
            return self.d_zhalo.at(self.z_slot[i] * self.rows * B)
        return self.d_zp.at(_position(self.set_ranges, i) * self.rows * B)

    # ------------------------------------------------------------------ what the ranks of a sharded proof send each other
    def _exchange(self, keys, held, dest, slot):
        """Exchange the polynomials each rank owns: a host slab with one per entry of `keys`, filled from `held` ((position in keys,
        device pointer) of the ones this rank holds), summed over the ranks; the entries this rank receives (`slot`: key -> position
        in `dest`) are uploaded into dest.  `keys` is empty on one rank: nothing happens."""
        if not keys:
            return
        slab = np.zeros((len(keys), self.rows, 4), dtype=np.uint64)
        for j, ptr in held:
            check(self.lib.vdb_memcpy_d2h(api._p(slab[j]), ptr, _sz(self.rows * B)))
        slab = self.comm.sum_disjoint(slab)
        for j, key in enumerate(keys):
            if key in slot:
                dest.upload(slab[j], offset=slot[key] * self.rows * B)

    def _held_foreign(self):
        """(position, pointer) of the Lagrange form of each column of all_foreign this rank holds, laid out one at a time"""
        tmp = api.DeviceBuffer(self.rows * B)
        for i, c in enumerate(self.all_foreign):
            if self._col_local(c) is not None:
                self._lagrange_block(c, 1, tmp)
                yield i, tmp.ptr
        tmp.free()

    # ------------------------------------------------------------------ round 1: advice and instance columns
    def _advice(self, pf, instances):
        """the advice columns (the hot path of the bench: witness, commit, lagrange_to_coeff, coeff_to_extended), the instance
        column made from the public values -> theta"""
        hp, lib, rows, k, ne = self.hp, self.lib, self.rows, self.k, self.ne
        my_cols = self.my_adv + self.my_lk
        pf.resident = hp.ext_cols >= my_cols + 2      # every advice coset stays in HBM; otherwise they are recomputed block by block
        ni = len(self.instance_cells)
        given = None if instances is None else np.ascontiguousarray(np.stack([np.asarray(v, dtype=np.uint64) for v in instances]).reshape(-1, 4) if ni else np.zeros((0, 4), np.uint64))
        assert given is None or len(given) == ni, "one value per public cell"
        inst_host = np.zeros((max(ni, 1), 4), dtype=np.uint64)
        # (the transforms of the advice columns are still running when step returns: the commitments are absorbed meanwhile)
        adv_local = hp.step(pf.timings, blind_seed=pf.seed(0), with_ext=False, sync=False, after_witness=lambda: self._public_values(inst_host, given)).copy()
        if pf.resident:        # the cosets of all my columns at once, into the hot path's coset buffer (three of the four it is sized for)
            with pf.stage("ntt"):
                self._ext_into(hp.d_cols.ptr, hp.d_ext.ptr, my_cols)
        adv_commits = self._globalize(adv_local, self.adv_ranges, self.n_cols)
        pf.instances = [inst_host[i].copy() for i in range(ni)]
        # the instance polynomial in the forms the rounds read (one column: queued behind the advice transforms)
        check(lib.vdb_memcpy_d2d(self.d_inst_coeff.ptr, self.d_inst_lag.ptr, _sz(rows * B)))
        check(lib.vdb_lagrange_to_coeff_dev(self.d_inst_coeff.ptr, _sz(1), k))
        self._ext_into(self.d_inst_coeff.ptr, self.d_inst_ext.ptr, 1)
        if pf.resident:
            check(lib.vdb_memcpy_d2d(hp.d_ext.at((my_cols + 1) * ne * B), self.d_inst_ext.ptr, _sz(ne * B)))
        if pf.tr is not None and ni:
            with pf.host_transcript():
                pf.tr.common_scalars(inst_host[:ni])
        pf.write_points(adv_commits)
        pf.squeeze("theta")
        pf.polys["adv"] = _Poly("adv", my_cols, coeff=hp.d_cols, commits=adv_commits, ranges=self.adv_ranges, n_total=self.n_cols)
        # the gate columns once more as a group of their own: only they are read at rows 1..3 (halo2 opens a column at the rotations
        # its queries name — the lookup columns only at the current row)
        pf.polys["advg"] = _Poly("advg", self.my_adv, coeff=hp.d_cols, commits=adv_commits[: self.n_adv], ranges=[(self.a_lo, self.a_hi)], n_total=self.n_adv)

    def _public_values(self, inst_host, given):
        """rows 0 .. ni - 1 of the instance column <- the public cells of the witness just generated (or the values of the
        statement handed in); the values are needed on the host before the advice commitments enter the transcript, so they
        are read here, behind the witness kernels only, and not behind the transforms queued next"""
        hp, lib, ni = self.hp, self.lib, len(self.instance_cells)
        if not ni:
            return
        if given is None:
            if self.world == 1:
                check(lib.vdb_gather_fr_dev(hp.d_stream.ptr, self.d_inst_cells.ptr, _sz(ni), self.d_inst_lag.ptr))
            else:
                # a rank writes only the cells of its own columns; the values every rank computes are the gadget's results
                ptr, cnt = hp.public_values_dev()
                if cnt != ni or self.instance_cells != self.public_cells:
                    raise ValueError("a sharded proof exposes the circuit's default public cells")
                check(lib.vdb_memcpy_d2d(self.d_inst_lag.ptr, ptr, _sz(ni * B)))
            check(lib.vdb_memcpy_d2h(api._p(inst_host), self.d_inst_lag.ptr, _sz(ni * B)))
        else:
            inst_host[:ni] = given
            check(lib.vdb_memcpy_h2d(self.d_inst_lag.ptr, api._p(inst_host), _sz(ni * B)))

    # ------------------------------------------------------------------ round 2: the lookup argument's permuted columns
    def _lookup_permuted(self, pf):
        """the permuted input and table columns, blinded and committed -> beta, gamma"""
        hp, lib, rows, my_lk, n_lk, lk_ranges = self.hp, self.lib, self.rows, self.my_lk, self.n_lk, self.lk_ranges
        with pf.stage("lookup_permute"):
            if my_lk:
                check(lib.vdb_layout_lookup_range_dev(hp.d_lookup.ptr, ctypes.c_uint64(hp.n_lookup), self.k, MINIMUM_ROWS, ctypes.c_uint64(self.l_lo), ctypes.c_uint64(self.l_hi),
                                                      self.d_lklag.ptr, hp.d_blind.at(hp.n_adv_cols * N_BLIND * B), N_BLIND))
            check(lib.vdb_lookup_permute_dev(self.d_lklag.ptr, self.fixed["table"].lag.ptr, _sz(my_lk), _sz(rows), _sz(self.usable), hp.L, self.d_pa.ptr, self.d_ps.ptr))
        self._blind(self.d_pa, my_lk, self.usable, pf.seed(1), lk_ranges, n_lk)
        self._blind(self.d_ps, my_lk, self.usable, pf.seed(2), lk_ranges, n_lk)
        with pf.stage("commit_permuted"):
            pa_c = self._commit(self.d_pa, my_lk, 1, dense=False)
        with pf.stage("commit_permuted"):
            ps_c = self._commit(self.d_ps, my_lk, 1, dense=False)
        if self.world > 1:
            both = self._globalize(np.concatenate([pa_c, ps_c], axis=1), lk_ranges, n_lk)
            pa_c, ps_c = np.ascontiguousarray(both[:, :8]), np.ascontiguousarray(both[:, 8:])
        pf.polys["pa"] = _Poly("pa", my_lk, lag=self.d_pa, commits=pa_c, ranges=lk_ranges, n_total=n_lk)
        pf.polys["ps"] = _Poly("ps", my_lk, lag=self.d_ps, commits=ps_c, ranges=lk_ranges, n_total=n_lk)
        pf.write_points(np.stack([pa_c, ps_c], axis=1).reshape(-1, 8))     # (pa_c, ps_c) per lookup column
        pf.squeeze("beta", "gamma")

    def _receive_foreign(self):
        """the columns of my sets that another rank holds (the set that spans the advice / lookup junction): their holder sends the
        Lagrange form, blinding rows included; the coefficient form is made here"""
        self._exchange(self.all_foreign, self._held_foreign(), self.d_foreign_lag, self.foreign_slot)
        if self.foreign:
            check(self.lib.vdb_memcpy_d2d(self.d_foreign_coeff.ptr, self.d_foreign_lag.ptr, _sz(len(self.foreign) * self.rows * B)))
            check(self.lib.vdb_lagrange_to_coeff_dev(self.d_foreign_coeff.ptr, _sz(len(self.foreign)), self.k))

    # ------------------------------------------------------------------ round 3 (beta, gamma): the running products
    def _products(self, pf):
        """the running products of both arguments, blinded and committed, then turned (with the permuted columns) into
        coefficient form.  The host absorbs one batch of commitments while the device works on the next thing that needs no
        challenge: the lookup products' MSM beside the permutation products' commitments, the coefficient forms (needed by the
        quotient, independent of y) beside the lookup products' commitments."""
        lib, rows, k, usable, my_lk, my_sets, d_zp, blk = self.lib, self.rows, self.k, self.usable, self.my_lk, self.my_sets, self.d_zp, self._blk
        with pf.stage("products"):
            for s_lo, s_hi in self.set_ranges:
                p_lo, p_hi = self.map.range_cols((s_lo, s_hi))
                for c0 in range(p_lo, p_hi, blk):
                    nb = min(blk, p_hi - c0)
                    self._lagrange_block(c0, nb, self.d_lag_a)
                    if self.d_map32 is not None:
                        check(lib.vdb_permutation_sigma_packed_dev(self.d_map32.at(c0 * rows * 4), _sz(nb), _sz(self.n_perm), k, api._p(self.delta), self.d_lag_s.ptr))
                    else:                                      # a key loaded from a file: back from the coefficient form
                        check(lib.vdb_memcpy_d2d(self.d_lag_s.ptr, self.fixed["sigma"].coeff.at(_position(self.sig_ranges, c0) * rows * B), _sz(nb * rows * B)))
                        check(lib.vdb_ntt_batch_dev(self.d_lag_s.ptr, _sz(nb), k, api._p(pf.omega), 0))
                    check(lib.vdb_permutation_product_range_dev(self.d_lag_a.ptr, self.d_lag_s.ptr, _sz(nb), _sz(c0), k, _sz(usable), _sz(self.chunk_len), pf.p["beta"], pf.p["gamma"],
                                                                api._p(self.delta), d_zp.at(_position(self.set_ranges, c0 // self.chunk_len) * rows * B)))
                # the products of a range run on from set to set
                check(lib.vdb_permutation_chain_dev(d_zp.at(_position(self.set_ranges, s_lo) * rows * B), _sz(s_hi - s_lo), k, _sz(usable)))
            if self.world > 1:
                # ... and from range to range across the ranks: every range starts where the one before it ended.  One field
                # element per range is exchanged (its last running product at the last usable row), every rank multiplies up the
                # ranges before its own.
                order = self.map.all_ranges()
                ends = np.zeros((len(order), 4), dtype=np.uint64)
                for i, (lo, hi, r) in enumerate(order):
                    if r == self.rank:
                        check(lib.vdb_memcpy_d2h(api._p(ends[i]), d_zp.at((_position(self.set_ranges, hi - 1) * rows + usable) * B), _sz(B)))
                ends = self.comm.sum_disjoint(ends)
                acc = 1
                for i, (lo, hi, r) in enumerate(order):
                    if r == self.rank and acc != 1:
                        check(lib.vdb_poly_scale_dev(d_zp.at(_position(self.set_ranges, lo) * rows * B), api._p(_fr_from_int(acc)), _sz((hi - lo) * rows)))
                    acc = acc * _fr_to_int(ends[i]) % R_MOD
            check(lib.vdb_lookup_product_dev(self.d_lklag.ptr, self.fixed["table"].lag.ptr, self.d_pa.ptr, self.d_ps.ptr, _sz(my_lk), _sz(rows), _sz(usable), pf.p["beta"], pf.p["gamma"],
                                             self.d_zl.ptr))
        self._blind(d_zp, my_sets, usable + 1, pf.seed(3), self.set_ranges, self.n_sets)
        self._blind(self.d_zl, my_lk, usable + 1, pf.seed(4), self.lk_ranges, self.n_lk)
        with pf.stage("commit_products"):
            zp_c = self._commit(d_zp, my_sets, 1)
        pf.polys["zp"] = _Poly("zp", my_sets, lag=d_zp, commits=self._globalize(zp_c, self.set_ranges, self.n_sets), ranges=self.set_ranges, n_total=self.n_sets)
        with pf.stage("commit_products"):
            self._commit_begin(self.d_zl, my_lk, 1)
        try:
            pf.write_points(pf.polys["zp"].commits)
        except Exception:
            lib.vdb_msm_batch_end(None, _sz(0))       # a deferred MSM must always be collected, or every later MSM is refused
            raise
        with pf.stage("commit_products"):
            zl_c = self._commit_end(my_lk)
        pf.polys["zl"] = _Poly("zl", my_lk, lag=self.d_zl, commits=self._globalize(zl_c, self.lk_ranges, self.n_lk), ranges=self.lk_ranges, n_total=self.n_lk)
        with pf.stage("derived_ntt"):
            for name in ("pa", "ps", "zp", "zl"):
                q = pf.polys[name]
                check(lib.vdb_lagrange_to_coeff_dev(q.lag.ptr, _sz(q.n_cols), k))      # in place: the Lagrange form is not needed again
                q.coeff, q.lag = q.lag, None
        pf.write_points(pf.polys["zl"].commits)

    def _random_poly(self, pf):
        """The vanishing argument's random polynomial (halo2 plonk/vanishing/prover.rs Argument::commit, [UPSTREAM-RECALL]): n uniform
        coefficients, committed before y is squeezed and opened at x beside the folded quotient — it blinds the one evaluation of h
        the multi-open reveals.  In a sharded proof rank 0 draws it and every rank receives the same coefficients.  -> y"""
        if self.rank == 0:
            api.random_scalars_dev(self.d_rand.ptr, self.rows, seed=pf.seed(5))
        self._exchange([0] if self.world > 1 else [], [(0, self.d_rand.ptr)] if self.rank == 0 else [], self.d_rand, {} if self.rank == 0 else {0: 0})
        with pf.stage("commit_h"):
            rand_c = self._commit(self.d_rand, 1, 0)
        pf.polys["rand"] = _Poly("rand", 1, coeff=self.d_rand, commits=rand_c, replicated=True)
        pf.write_points(rand_c)
        pf.squeeze("y")

    def _receive_boundary_products(self):
        """the boundary products other ranks ask for, in coefficient form: the set before each of their ranges, the first set for the chain's closer"""
        self._exchange(self.all_z, ((j, self._z_coeff(i)) for j, i in enumerate(self.all_z) if self.map.set_owner(i) == self.rank), self.d_zhalo, self.z_slot)

    # ------------------------------------------------------------------ round 4 (y): the quotient
    def _quotient(self, pf):
        """h's pieces, committed -> x.  The numerator is sum_i term_i y^(N-1-i) over the terms in halo2's order: gates (one per advice column),
        the permutation argument (two terms of the product columns alone, the chaining of the sets, one product term per set),
        the lookup argument (five per lookup column).  Each group is folded into an accumulator of its own (acc <- acc y +
        term, from zero) while ONE sweep over blocks of columns produces every coset once — the advice / lookup / constants
        cosets (unless resident), selectors, sigma, product and lookup-argument cosets — and the groups are joined at the end:
        h = ((Ag y^n2 + A2) y^n3 + A3) y^n4 + A4.  (The public inputs have no term of their own: the instance column is one
        of the permutation's columns.)
        Everything is evaluated coset by coset on N_SLOTS = 3 of the extended domain's four cosets (the quotient has degree below
        3 n; 2 of 2 for a circuit of degree 3).  The gates have degree 3: their share of the quotient, Ag / (X^n - 1), has degree below 2 n, so Ag is evaluated on
        two of them (slots 0 and 1 of the advice cosets; the selector cosets are made for those two only), brought back to
        coefficients from there, and joined in coefficient form.
        Sharded: a rank folds the terms of its own columns and sets (the folds skip what other ranks hold: _Fold); every step
        after that — the joins, the division by X^n - 1, the way back to coefficients — is linear, so each rank ends with a
        share of h's coefficients and the shares are added (the one bulk exchange of the proof: 2^(k+2) x 32 B per rank)."""
        lib, rows, k, ne, n_adv, n_sets, blk = self.lib, self.rows, self.k, self.ne, self.n_adv, self.n_sets, self._blk
        ag, a2, a3, a4 = self.d_hg, self.d_h2, self.d_h3, self.d_h4
        n2, n3, n4 = 2 + (n_sets - 1), n_sets, 5 * self.n_lk
        folds = (_Fold(lib, pf, "y", ag, GATE_SLOTS * rows, n_adv), _Fold(lib, pf, "y", a2, ne, n2), _Fold(lib, pf, "y", a3, ne, n3), _Fold(lib, pf, "y", a4, ne, n4))
        perm_args = (_sz(self.n_perm), _sz(self.chunk_len), k, self.n_slots, _sz(self.usable), *self.l_cosets, pf.p["beta"], pf.p["gamma"], api._p(self.delta), pf.p["y"])
        with pf.stage("quotient"):
            for a in (a2, a3, a4):
                check(lib.vdb_memset_dev(a.ptr, 0, _sz(ne * B)))
            check(lib.vdb_memset_dev(ag.ptr, 0, _sz(GATE_SLOTS * rows * B)))
            # l0 (1 - z_0), l_last (z_last^2 - z_last): the first two terms of group 2, folded in by the owner of the last set
            if self.map.head_owner() == self.rank:
                self._ext_into(self._z_coeff(0), self.d_zf.ptr, 1)
                self._ext_into(self._z_coeff(n_sets - 1), self.d_zlast.ptr, 1)
                folds[1].skip_to(0, 2)
                check(lib.vdb_permutation_eval_parts_cosets_dev(None, _sz(0), None, None, _sz(0), self.d_zf.ptr, self.d_zlast.ptr, *perm_args, a2.ptr, 1, _sz(0), _sz(0), _sz(0), _sz(0)))
            # my lookup columns that complete another rank's set (the head of the lookup columns, at the advice / lookup junction):
            # their lookup argument is mine all the same, and comes first in the order of the terms
            stray_lk = sorted(c for c in self.stray if c >= n_adv)
            if stray_lk:
                assert stray_lk == list(range(stray_lk[0], stray_lk[0] + len(stray_lk)))
                base, col0 = self._adv_ext_block(pf, stray_lk[0], len(stray_lk))
                self._lookup_terms(pf, folds[3], base, col0, stray_lk[0] - n_adv, stray_lk[-1] + 1 - n_adv)
            assert all(c >= n_adv for c in self.stray), "an advice column outside its rank's sets"
            for s_lo, s_hi in self.set_ranges:
                p_lo, p_hi = self.map.range_cols((s_lo, s_hi))
                for c0 in range(p_lo, p_hi, blk):
                    self._quotient_block(pf, folds, perm_args, s_lo, c0, min(blk, p_hi - c0))
            for f in folds:
                f.finish()
            # join the groups that live on the 4 n points (acc_next += y^(terms of the next group) * acc), divide, back to coefficients
            y_int = _fr_to_int(pf.ch["y"])
            check(lib.vdb_poly_axpy_dev(a3.ptr, api._p(_fr_from_int(pow(y_int, n3, R_MOD))), a2.ptr, _sz(ne)))
            check(lib.vdb_poly_axpy_dev(a4.ptr, api._p(_fr_from_int(pow(y_int, n4, R_MOD))), a3.ptr, _sz(ne)))
            # (division by X^n - 1 — a constant per coset —, residues modulo X^n - g_t^n, the Vandermonde system in g_t^n: N_H pieces)
            check(lib.vdb_cosets_to_coeff_dev(a4.ptr, self.d_h.ptr, k, self.n_slots))
            # the gates' share: the same from its two cosets, then h += y^(every later term) * (its 2 n coefficients)
            check(lib.vdb_cosets_to_coeff_dev(ag.ptr, a2.ptr, k, GATE_SLOTS))
            check(lib.vdb_poly_axpy_dev(self.d_h.ptr, api._p(_fr_from_int(pow(y_int, n2 + n3 + n4, R_MOD))), a2.ptr, _sz(GATE_SLOTS * rows)))
            self.comm.sum_field_dev(self.d_h.ptr, ne)                      # every rank's share of h (nothing to do on one rank)
        with pf.stage("commit_h"):
            h_c = self._commit(self.d_h, self.n_h, 0)      # h(X) = sum_i X^(n i) h_i(X), degree below (degree - 1) n
        pf.polys["h"] = _Poly("h", self.n_h, coeff=self.d_h, commits=h_c, replicated=True)
        pf.write_points(h_c)
        pf.squeeze("x")

    def _quotient_block(self, pf, folds, perm_args, s_lo, c0, nb):
        """the quotient's terms of the permutation's columns c0 .. c0 + nb (in the range of sets from s_lo): gates, permutation, lookups"""
        lib, rows, k, ne, fx, chunk, d_eb, d_ez = self.lib, self.rows, self.k, self.ne, self.fixed, self.chunk_len, self.d_eb, self.d_ez
        f_g, f_2, f_3, f_4 = folds
        base, col0 = self._adv_ext_block(pf, c0, nb)
        g0, g1 = max(c0, self.a_lo), min(c0 + nb, self.a_hi)
        if g0 < g1:                                            # gates of the block's advice columns
            if self.fixed_cosets_resident:
                sel_ptr = fx["sel"].ext.at((g0 - self.a_lo) * GATE_SLOTS * rows * B)
            else:
                check(lib.vdb_coeff_to_cosets_dev(fx["sel"].coeff.at((g0 - self.a_lo) * rows * B), d_eb.ptr, _sz(g1 - g0), k, GATE_SLOTS, None))
                sel_ptr = d_eb.ptr
            f_g.skip_to(g0, g1 - g0)
            check(lib.vdb_gate_eval_cosets_dev(self._col_ptr(base, col0, g0), self.n_slots, sel_ptr, _sz(g1 - g0), k, GATE_SLOTS, pf.p["y"], self.d_hg.ptr))
        # permutation: the block's sets with their sigma cosets and product cosets (one set more in front for the chaining)
        set_lo, set_hi = c0 // chunk, -(-(c0 + nb) // chunk)
        z0 = max(set_lo - 1, 0)
        if self.fixed_cosets_resident:      # resident sigma cosets (keygen): no transform, the evaluation multiplies by beta itself
            sig_ptr, sig_head = fx["sigma"].ext.at(_position(self.sig_ranges, c0) * ne * B), 0
        else:                               # the cosets of beta sigma: the scalar rides on the transform's coset factors, the evaluation skips a product per point
            check(lib.vdb_coeff_to_cosets_dev(fx["sigma"].coeff.at(_position(self.sig_ranges, c0) * rows * B), d_eb.ptr, _sz(nb), k, self.n_slots, pf.p["beta"]))
            sig_ptr, sig_head = d_eb.ptr, 2
        if z0 < set_lo and (z0 in self.z_slot or z0 < s_lo):          # the set in front is another rank's (or another range's)
            self._ext_into(self._z_coeff(z0), d_ez.ptr, 1)
            self._ext_into(self._z_coeff(set_lo), d_ez.at(ne * B), set_hi - set_lo)
        else:
            self._ext_into(self._z_coeff(z0), d_ez.ptr, set_hi - z0)
        if max(set_lo, 1) < set_hi:
            f_2.skip_to(max(set_lo, 1) + 1, set_hi - max(set_lo, 1))
            check(lib.vdb_permutation_eval_parts_cosets_dev(None, _sz(0), None, d_ez.ptr, _sz(z0), None, None, *perm_args, self.d_h2.ptr, 0, _sz(max(set_lo, 1)), _sz(set_hi),
                                                            _sz(0), _sz(0)))
        f_3.skip_to(set_lo, set_hi - set_lo)
        check(lib.vdb_permutation_eval_parts_cosets_dev(base, _sz(col0), sig_ptr, d_ez.ptr, _sz(z0), None, None, *perm_args, self.d_h3.ptr, sig_head, _sz(0), _sz(0), _sz(set_lo),
                                                        _sz(set_hi)))
        # lookup argument of the block's lookup columns that are mine
        j_lo, j_hi = max(c0 - self.n_adv, self.l_lo), min(c0 + nb - self.n_adv, self.l_hi)
        self._lookup_terms(pf, f_4, base, col0, j_lo, j_hi)

    def _lookup_terms(self, pf, fold, base, col0, j_lo, j_hi):
        """the lookup argument of my lookup columns j_lo .. j_hi, whose input cosets are in the block at `base`:
        [permuted input | permuted table | product] cosets in thirds of one buffer"""
        rows, ne, d_eb, polys, third = self.rows, self.ne, self.d_eb, pf.polys, self._blk // 3
        for j0 in range(j_lo, max(j_hi, j_lo), third):
            m = min(third, j_hi - j0)
            for i, name in enumerate(("pa", "ps", "zl")):
                self._ext_into(polys[name].coeff.at((j0 - self.l_lo) * rows * B), d_eb.at(i * third * ne * B), m)
            fold.skip_to(5 * j0, 5 * m)
            check(self.lib.vdb_lookup_eval_cosets_dev(self._col_ptr(base, col0, self.n_adv + j0), self.fixed["table"].ext.ptr, d_eb.ptr, d_eb.at(third * ne * B),
                                                      d_eb.at(2 * third * ne * B), _sz(m), self.k, self.n_slots, *self.l_cosets, pf.p["beta"], pf.p["gamma"], pf.p["y"], self.d_h4.ptr))

    def _fold_h(self, pf):
        """h folded at x (halo2 vanishing::Constructed::evaluate): hf(X) = sum_i x^(n i) h_i(X), one polynomial of degree below n whose
        commitment the verifier forms from the pieces' and whose value at x it computes from the quotient identity — neither is sent"""
        lib, rows = self.lib, self.rows
        xn = pow(_fr_to_int(pf.ch["x"]), rows, R_MOD)
        check(lib.vdb_memcpy_d2d(self.d_hf.ptr, self.d_h.ptr, _sz(rows * B)))
        for i in range(1, self.n_h):
            check(lib.vdb_poly_axpy_dev(self.d_hf.ptr, api._p(_fr_from_int(pow(xn, i, R_MOD))), self.d_h.at(i * rows * B), _sz(rows)))
        with pf.stage("commit_h"):
            hf_c = self._commit(self.d_hf, 1, 0)
        pf.polys["hf"] = _Poly("hf", 1, coeff=self.d_hf, commits=hf_c, replicated=True)

    # ------------------------------------------------------------------ round 5 (x): evaluations, at the rotations protocol.opened states
    def _evaluations(self, pf, allp, opened, points):
        """every opened polynomial at its points, absorbed into the transcript -> evals[(name, rotation)] (Montgomery arrays)"""
        groups = [(rot, name) for rot, names in opened.items() for name in names]
        evals = {}
        if self.world == 1 and pf.tr is not None and pf.timings is None:
            # the device evaluates group i + 1 while the host absorbs the evaluations of group i (the sponge's host work — ~6 us per four
            # values — is longer than the evaluation itself: only the first group's kernel is not hidden)
            sizes = [allp[name].n_cols for _rot, name in groups]
            offs = [sum(sizes[:i]) * B for i in range(len(groups))]
            d_ev = api.DeviceBuffer(max(sum(sizes), 1) * B)
            launches = [(allp[name], points[rot], d_ev.at(o)) for (rot, name), o in zip(groups, offs)]
            try:
                if groups:
                    self._eval_into(*launches[0])
                for i, (rot, name) in enumerate(groups):
                    out = d_ev.download((sizes[i], 4), offset=offs[i])       # waits for group i's kernel only
                    if i + 1 < len(groups):
                        self._eval_into(*launches[i + 1])
                    evals[(name, rot)] = out
                    if name not in DERIVED:                  # computed by the verifier, not sent
                        with pf.host_transcript():
                            pf.tr.write_scalars(out)
                            pf.tr.flush()
            finally:
                api.sync()
                d_ev.free()
            return evals
        with pf.stage("evaluations"):
            for rot, name in groups:
                q = allp[name]
                out = np.zeros((q.n_cols, 4), dtype=np.uint64)
                check(self.lib.vdb_eval_polys_dev(q.coeff.ptr, _sz(q.n_cols), _sz(self.rows), api._p(_fr_from_int(points[rot])), api._p(out)))
                evals[(name, rot)] = out
            if self.world > 1:
                # every rank evaluated its own polynomials: one exchange puts every group's evaluations in the global order
                # (the polynomials every rank holds are not exchanged)
                shared = [(rot, name) for rot, name in groups if not allp[name].replicated]
                ranges, o = [], 0
                for _rot, name in shared:
                    ranges += [(o + lo, o + hi) for lo, hi in allp[name].ranges]
                    o += allp[name].n_total
                whole = self._globalize(np.concatenate([evals[(name, rot)] for rot, name in shared]), ranges, o)
                o = 0
                for rot, name in shared:
                    evals[(name, rot)] = np.ascontiguousarray(whole[o: o + allp[name].n_total])
                    o += allp[name].n_total
        if pf.tr is not None:
            with pf.host_transcript():
                for rot, name in groups:
                    if name not in DERIVED:                  # computed by the verifier, not sent
                        pf.tr.write_scalars(evals[(name, rot)])
        return evals

    def _eval_into(self, q, point, dest):
        check(self.lib.vdb_eval_polys_dev_out(q.coeff.ptr, _sz(q.n_cols), _sz(self.rows), api._p(_fr_from_int(point)), dest))

    # ------------------------------------------------------------------ round 6: the multi-open
    def _open_gwc(self, pf, allp, opened, points):
        """v -> one opening per rotation point: combine with powers of v, divide by (X - point), commit"""
        lib, rows, d_comb, d_quot = self.lib, self.rows, self.d_comb, self.d_quot
        pf.squeeze("v")
        openings = []
        with pf.stage("openings"):
            for rot, names in opened.items():
                check(lib.vdb_memset_dev(d_comb.ptr, 0, _sz(rows * B)))
                for name in names:
                    q = allp[name]
                    check(lib.vdb_poly_lincomb_dev(q.coeff.ptr, _sz(q.n_cols), _sz(rows), pf.p["v"], d_comb.ptr))
                rem = np.zeros((1, 4), dtype=np.uint64)
                check(lib.vdb_kate_div_dev(d_comb.ptr, _sz(1), _sz(rows), api._p(_fr_from_int(points[rot])), d_quot.ptr, api._p(rem)))
                W = self._commit(d_quot, 1, 0)[0]
                openings.append(dict(rotation=rot, point=points[rot], polys=list(names), eval=rem[0].copy(), W=W))
        pf.write_points([op["W"] for op in openings])
        return openings

    # SHPLONK multi-open (halo2 poly/kzg/multiopen/shplonk)
    def _shplonk(self, pf, allp, opened, points, evals):
        """Polynomials opened at the same set of points form a rotation set S.  With q_S = the set's polynomials combined with
        powers of yo, r_S the interpolant of q_S's values on S and Z_S the vanishing polynomial of S:
            f = sum_S v^(m-1-s) (q_S - r_S) / Z_S                          -> commitment W1, then u,
            L = sum_S v^(m-1-s) Z_{T minus S}(u) (q_S - r_S(u)) - Z_T(u) f,  L(u) = 0  -> W2 = commit(L / (X - u)).
        The polynomial work (combinations, divisions by the linear factors, scaled sums, commits) runs on the device; the
        interpolants have at most four points and are host integers.
        Sharded: q_S is a sum over the set's polynomials, so each rank combines the ones it holds (their powers of yo by their
        place in the whole set); the quotient of a division by Z_S — the remainder dropped — and L's division by X - u are
        linear, so every rank commits its share of f and of L / (X - u) and the shares are added as points (vdb_g1_sum: RCCL has no
        curve operator, two 64-byte points per rank are gathered)."""
        lib, rows, p, R = self.lib, self.rows, pf.p, R_MOD
        sets = protocol.rotation_sets(opened)
        pf.squeeze("yo", "v")
        v = _fr_to_int(pf.ch["v"])
        m = len(sets)
        d_q = [api.DeviceBuffer(rows * B) for _ in sets]
        d_f, d_a, d_b = api.DeviceBuffer(rows * B), self.d_comb, self.d_quot
        r_polys, rems = [], []
        # f, the quotient of all rotation sets
        with pf.stage("openings"):
            check(lib.vdb_memset_dev(d_f.ptr, 0, _sz(rows * B)))
            for s_i, (rots, names) in enumerate(sets):
                self._combine(pf, allp, names, d_q[s_i])
                vals = []
                for rot in rots:                                   # the set's evaluations at this point, combined with powers of yo (host, compiled)
                    acc = np.zeros(4, dtype=np.uint64)
                    for name in names:
                        e = np.ascontiguousarray(evals[(name, rot)], dtype=np.uint64)
                        check(lib.vdb_fr_horner(api._p(e), _sz(e.shape[0]), p["yo"], api._p(acc)))
                    vals.append(_fr_to_int(acc))
                r = protocol.interpolate([points[rot] for rot in rots], vals)
                r_polys.append(r)
                # (q_S - r_S) / Z_S: the low coefficients on the host, one division per point on the device.  (r_S has fewer
                # coefficients than Z_S has roots: it changes the remainders only, which is why a rank's share needs no r_S.)
                check(lib.vdb_memcpy_d2d(d_a.ptr, d_q[s_i].ptr, _sz(rows * B)))
                if self.world == 1:
                    low = np.zeros((len(r), 4), dtype=np.uint64)
                    check(lib.vdb_memcpy_d2h(api._p(low), d_a.ptr, _sz(low.nbytes)))
                    low = np.stack([_fr_from_int(_fr_to_int(low[i]) - r[i]) for i in range(len(r))])
                    check(lib.vdb_memcpy_h2d(d_a.ptr, api._p(low), _sz(low.nbytes)))
                src, dst = d_a, d_b
                for rot in rots:
                    rem = np.zeros((1, 4), dtype=np.uint64)
                    check(lib.vdb_kate_div_dev(src.ptr, _sz(1), _sz(rows), api._p(_fr_from_int(points[rot])), dst.ptr, api._p(rem)))
                    rems.append(_fr_to_int(rem[0]))
                    src, dst = dst, src
                check(lib.vdb_poly_lincomb_dev(src.ptr, _sz(1), _sz(rows), p["v"], d_f.ptr))          # f = f v + (q_S - r_S) / Z_S
            W1 = self._share(self._commit(d_f, 1, 0)[0])
        pf.write_points([W1])
        pf.squeeze("u")
        u = _fr_to_int(pf.ch["u"])
        all_rots = sorted({rot for rots, _ in sets for rot in rots})
        # the linearisation polynomial L and its quotient by X - u
        with pf.stage("openings"):
            check(lib.vdb_memset_dev(d_a.ptr, 0, _sz(rows * B)))
            const = 0
            for s_i, (rots, names) in enumerate(sets):
                coef = pow(v, m - 1 - s_i, R) * protocol.vanishing([points[rot] for rot in all_rots if rot not in rots], u) % R
                check(lib.vdb_poly_axpy_dev(d_a.ptr, api._p(_fr_from_int(coef)), d_q[s_i].ptr, _sz(rows)))
                const = (const + coef * protocol.horner(r_polys[s_i], u)) % R
            check(lib.vdb_poly_axpy_dev(d_a.ptr, api._p(_fr_from_int(-protocol.vanishing([points[rot] for rot in all_rots], u))), d_f.ptr, _sz(rows)))
            if self.rank == 0:                                     # the constant term belongs to one share
                c0 = np.zeros((1, 4), dtype=np.uint64)
                check(lib.vdb_memcpy_d2h(api._p(c0), d_a.ptr, _sz(32)))
                c0[0] = _fr_from_int(_fr_to_int(c0[0]) - const)
                check(lib.vdb_memcpy_h2d(d_a.ptr, api._p(c0), _sz(32)))
            rem = np.zeros((1, 4), dtype=np.uint64)
            check(lib.vdb_kate_div_dev(d_a.ptr, _sz(1), _sz(rows), p["u"], d_b.ptr, api._p(rem)))
            rems.append(_fr_to_int(rem[0]))
            W2 = self._share(self._commit(d_b, 1, 0)[0])
        pf.write_points([W2])
        for b in d_q + [d_f]:
            b.free()
        return dict(kind="shplonk", sets=[(list(rots), list(names)) for rots, names in sets], W1=W1, W2=W2, remainders=rems)

    def _combine(self, pf, allp, names, dest):
        """dest <- this rank's share of the set's polynomials combined with powers of yo: polynomial j of the M the set has in
        all enters with yo^(M - 1 - j).  A fold over the ones held here (the replicated ones by rank 0)."""
        rows = self.rows
        check(self.lib.vdb_memset_dev(dest.ptr, 0, _sz(rows * B)))
        fold = _Fold(self.lib, pf, "yo", dest, rows, sum(allp[name].n_total for name in names))
        base = 0
        for name in names:
            q, loc = allp[name], 0
            for lo, hi in (q.ranges if (not q.replicated or self.rank == 0) else []):
                fold.skip_to(base + lo, hi - lo)
                check(self.lib.vdb_poly_lincomb_dev(q.coeff.at(loc * rows * B), _sz(hi - lo), _sz(rows), pf.p["yo"], dest.ptr))
                loc += hi - lo
            base += q.n_total
        fold.finish()

    def _share(self, point):
        """the sum over the ranks of their partial commitments"""
        if self.world == 1:
            return point
        out = np.zeros((1, 8), dtype=np.uint64)
        parts = np.ascontiguousarray(self.comm.gather_rows(np.asarray(point, dtype=np.uint64).reshape(1, 8)))
        check(self.lib.vdb_g1_sum(api._p(parts), _sz(self.world), _sz(1), api._p(out)))
        return out[0]

    def free(self):
        for q in self.fixed.values():
            q.free()
        self.fixed = {}
        self._vk_digest = None
        for name in ("pool_der", "d_lklag", "d_lag_a", "d_lag_s", "d_ea", "d_eb", "d_ez", "d_zf", "d_zlast", "d_h", "d_h2", "d_h3", "d_h4", "d_hg", "d_comb", "d_quot", "d_map32", "d_inst_lag", "d_inst_coeff", "d_inst_ext", "d_inst_cells",
                     "d_foreign_lag", "d_foreign_coeff", "d_zhalo", "d_rand", "d_hf", "d_key", "d_map"):
            b = getattr(self, name, None)
            if b is not None:
                b.free()
                setattr(self, name, None)
        if hasattr(self.circuit, "free"):
            self.circuit.free()
        for name in ("srs_m", "srs_few"):
            if getattr(self, name, None) is not None:
                getattr(self, name).free()
                setattr(self, name, None)


def quotient_identity_holds(pr, challenges, evals, instances=None):
    """What a verifier checks first: the gate, permutation and lookup expressions recombined from the evaluations at x (and the
    rotated points, protocol.quotient_numerator) equal h(x) (x^n - 1).  `pr`: the ProverRounds that produced them (for the circuit's
    shape); `challenges`, `evals`: as returned by ProverRounds.prove.  False as well when the evaluations do not have the shape of
    pr's circuit.  Plain integer arithmetic on the host."""
    ch = {name: _fr_to_int(challenges[name]) for name in ("beta", "gamma", "y", "x")}
    meta = protocol.key_meta(pr.k, pr.n_adv, pr.n_lk, len(pr.instance_cells))
    try:
        num = protocol.quotient_numerator(meta, ch, evals, list(instances) if instances is not None else [])
    except ValueError:
        return False
    hx = evals[("hf", 0)][0]                 # h folded at x: sum_i x^(n i) h_i(x), evaluated by the prover (a verifier computes it from this very identity)
    return num == hx * (pow(ch["x"], pr.rows, R_MOD) - 1) % R_MOD and num != 0
