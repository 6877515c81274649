"""The Verify arm (the reference's SnarkCmd::Verify, src/scaffold/mod.rs:298-320; halo2's read_snark + verify_proof): checks a proof
that ProverRounds.prove() wrote against its verifying key.

    vk = VerifyingKey.read("kmeans.snark.vk.npz")          # or halo2's RawBytes data/{name}.vk (+ the SRS scalar)
    ok = verify(proof, instances, vk)                       # True / False, never raises on malformed input
    ok = Verifier.from_files("kmeans.snark", "kmeans.snark.vk.npz").verify()

The protocol is the one the prover runs (rounds.py; protocol.py states what the two share), replayed from the proof bytes alone:
  1. every compressed point of the proof decompressed in one device call (vdb_g1_decompress_dev);
  2. the Fiat–Shamir transcript replayed (api.Transcript): the key's digest, the public values, then the proof's points and
     evaluations in the order the prover wrote them, squeezing theta, beta, gamma, y, x, the SHPLONK challenges y', v, u;
  3. the quotient identity's numerator from the evaluations (gates, permutation, lookups; l_0, l_last, l_blind and the instance
     column computed at x), which fixes the value of h folded at x: numerator / (x^n - 1);
  4. SHPLONK: polynomials opened at the same rotations form a set; per set its combination, the interpolation of its values at
     u, and the vanishing polynomial of the other rotations; everything lands in ONE multi-scalar multiplication over the fixed
     commitments, the proof's commitments (the folded h as its pieces with the powers of x^n) and W1, W2
     (vdb_msm_points_dev);
  5. the pairing equation e(lhs + u W2, [1]_2) e(-W2, [tau]_2) = 1 on the host (vdb_pairing_check).
The per-column algebra of 3 and 4 is Python integers (~10^5 modular products at the largest circuit)."""
import ctypes
import time

import numpy as np

from . import _lib, api, protocol
from .api import DeviceBuffer, _p, _sz
from .protocol import FIXED, R_MOD, fr_from_int, fr_from_ints, fr_to_int

Q_MOD = 0x30644E72E131A029B85045B68181585D97816A916871CA8D3C208C16D87CFD47


def _g2_generator_times(s):
    """[s] G2 as a vdb_g2 (16 uint64: x0, x1, y0, y1, Montgomery)"""
    out = np.zeros(16, dtype=np.uint64)
    api.check(_lib.load().vdb_g2_mul_generator(_p(fr_from_int(s)), _p(out)))
    return out


class VerifyingKey:
    """The circuit's shape (meta: rows, k, n_adv, n_lk, n_cols, n_sets, chunk_len, n_blind, delta, n_instances), which polynomial is
    opened at which rotation, the fixed commitments ({name: (m, 8) uint64} for FIXED), and [tau]_2 — from the SRS scalar tau of the
    deterministic setup, or given as a vdb_g2 array — with the SRS's g2 (G2's generator unless given: a params file carries its own)."""

    def __init__(self, meta, fixed, opened=None, tau=None, tau_g2=None, g2=None):
        self.meta = {key: int(meta[key]) for key in ("rows", "k", "n_adv", "n_lk", "n_cols", "n_sets", "chunk_len", "n_blind", "delta", "n_instances")}
        self.fixed = {name: np.ascontiguousarray(fixed[name], dtype=np.uint64).reshape(-1, 8) for name in FIXED}
        self.opened = {int(rot): list(names) for rot, names in (opened or protocol.opened(self.meta["n_lk"], self.meta["n_blind"])).items()}
        if tau_g2 is None:
            if tau is None:
                raise ValueError("a verifying key needs [tau]_2 or the SRS scalar tau")
            tau_g2 = _g2_generator_times(int(tau))
        self.tau_g2 = np.ascontiguousarray(tau_g2, dtype=np.uint64).reshape(16)
        self.g2 = _g2_one() if g2 is None else np.ascontiguousarray(g2, dtype=np.uint64).reshape(16)
        self._digest = None

    @classmethod
    def from_prover(cls, pr, opened=None):
        """the key of a ProverRounds after keygen (what save_verifying_key writes)"""
        meta = protocol.key_meta(pr.k, pr.n_adv, pr.n_lk, len(pr.instance_cells))
        fixed = {name: pr.fixed[name].commits for name in FIXED}
        if pr.hp.tau is None:        # an SRS from a params file
            return cls(meta, fixed, opened, tau_g2=pr.hp.tau_g2, g2=pr.hp.g2)
        return cls(meta, fixed, opened, tau=pr.hp.tau)

    @classmethod
    def read(cls, path, n_instances=None, tau=None, params=None):
        """save_verifying_key's .npz (its stored digest is checked), or else halo2's RawBytes .vk (io.read_verifying_key_raw; the number
        of public values and the SRS scalar come from the caller — the reference's gen_srs scalar by default).  `params`: the SRS's G2
        side from a halo2 params file instead (its path, or an srs.ParamsKZG), for either kind of key; not together with `tau`.
        ValueError when the file is not a key of this circuit family."""
        from . import io
        g2 = tau_g2 = None
        if params is not None:
            if tau is not None:
                raise ValueError("give the SRS as tau or as params, not both")
            from .srs import ParamsKZG, read_params_g2
            g2, tau_g2 = (params.g2, params.s_g2) if isinstance(params, ParamsKZG) else read_params_g2(params)
        if str(path).endswith(".npz"):
            meta, fixed = io.read_verifying_key(path)
            if tau_g2 is None and tau is None and "tau_g2" in meta:      # a key made from a params file carries its G2 points
                tau_g2, g2 = meta["tau_g2"], meta.get("g2")
            if tau_g2 is not None:
                vk = cls(meta, fixed, meta.get("opened"), tau_g2=tau_g2, g2=g2)
            else:
                vk = cls(meta, fixed, meta.get("opened"), tau=meta.get("tau") if tau is None else tau)
            if "vk_digest" in meta and fr_to_int(vk.digest()) != meta["vk_digest"]:
                raise ValueError("the key's digest is not the digest of its commitments")
            return vk
        if tau_g2 is not None:
            meta, fixed, _selectors = io.read_verifying_key_raw(path, n_instances=int(n_instances or 0))
            return cls(meta, fixed, meta.pop("opened"), tau_g2=tau_g2, g2=g2)
        if tau is None:
            from .srs import gen_srs_tau
            tau = gen_srs_tau()
        meta, fixed, _selectors = io.read_verifying_key_raw(path, n_instances=int(n_instances or 0), tau=int(tau))
        return cls(meta, fixed, meta.pop("opened"), tau=meta.pop("tau"))

    def digest(self):
        if self._digest is None:
            self._digest = protocol.vk_digest(self.fixed)
        return self._digest


class _Reject(Exception):
    pass


def _counts(meta):
    """how many evaluations of each opened polynomial a proof carries per rotation (hf: none, the verifier derives it)"""
    return {"adv": meta["n_cols"], "advg": meta["n_adv"], "sel": meta["n_adv"], "sigma": meta["n_cols"] + 2, "cst": 1, "table": 1, "pa": meta["n_lk"],
            "ps": meta["n_lk"], "zp": meta["n_sets"], "zl": meta["n_lk"], "rand": 1, "hf": 0}


def decompress(enc, sign_bit=6):
    """n x 32 bytes of compressed points -> ((n, 8) uint64 Montgomery affine points, (n,) uint8 status: include/vdb.h VDB_G1_*)"""
    enc = np.frombuffer(bytes(enc), dtype=np.uint8)
    n = enc.size // 32
    if n == 0:
        return np.zeros((0, 8), dtype=np.uint64), np.zeros(0, dtype=np.uint8)
    lib = _lib.init()
    bufs = [DeviceBuffer(enc.size), DeviceBuffer(64 * n), DeviceBuffer(n)]
    try:
        bufs[0].upload(enc)
        api.check(lib.vdb_g1_decompress_dev(bufs[0].ptr, _sz(n), ctypes.c_uint32(sign_bit), bufs[1].ptr, bufs[2].ptr))
        return bufs[1].download((n, 8)), bufs[2].download((n,), dtype=np.uint8)
    finally:
        for b in bufs:
            b.free()


def msm_points(points, scalars):
    """sum_i scalars[i] points[i] on the device (vdb_msm_points_dev): points (n, 8) uint64 Montgomery affine, scalars (n, 4)
    Montgomery Fr -> (8,) uint64"""
    points = np.ascontiguousarray(points, dtype=np.uint64).reshape(-1, 8)
    scalars = np.ascontiguousarray(scalars, dtype=np.uint64).reshape(-1, 4)
    assert points.shape[0] == scalars.shape[0]
    lib = _lib.init()
    out = np.zeros(8, dtype=np.uint64)
    n = points.shape[0]
    bufs = [DeviceBuffer(max(points.nbytes, 64)), DeviceBuffer(max(scalars.nbytes, 32))]
    try:
        if n:
            bufs[0].upload(points)
            bufs[1].upload(scalars)
        api.check(lib.vdb_msm_points_dev(bufs[0].ptr, bufs[1].ptr, _sz(n), _p(out)))
        return out
    finally:
        for b in bufs:
            b.free()


def pairing_check(g1, g2):
    """prod e(g1[i], g2[i]) == 1 (vdb_pairing_check): g1 (n, 8), g2 (n, 16) uint64 Montgomery"""
    g1 = np.ascontiguousarray(g1, dtype=np.uint64).reshape(-1, 8)
    g2 = np.ascontiguousarray(g2, dtype=np.uint64).reshape(-1, 16)
    ok = ctypes.c_int(0)
    api.check(_lib.load().vdb_pairing_check(_p(g1), _p(g2), _sz(g1.shape[0]), ctypes.byref(ok)))
    return bool(ok.value)


def _neg_point(pt):
    pt = np.array(pt, dtype=np.uint64).reshape(8)
    if not pt.any():
        return pt
    y = sum(int(pt[4 + i]) << (64 * i) for i in range(4))
    ny = (Q_MOD - y) % Q_MOD              # the Montgomery form of -y
    pt[4:] = [(ny >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)]
    return pt


def verify(proof, instances, vk, sign_bit=6, timings=None):
    """True when `proof` (the bytes ProverRounds.prove() writes) proves the statement `instances` (the public values, integers)
    under `vk` (a VerifyingKey); False for a wrong proof and for any malformed input — a short or long proof, a point off the
    curve or not canonical, a scalar >= r, the wrong number of public values, a key whose shape does not describe the proof.
    timings (dict, optional) receives the seconds of each stage."""
    try:
        return _verify(bytes(proof), [int(v) for v in instances], vk, sign_bit, timings if timings is not None else {})
    except _Reject:
        return False
    except (ValueError, ZeroDivisionError, IndexError, KeyError, TypeError, OverflowError):
        return False


def _verify(proof, instances, vk, sign_bit, t):
    R, meta, opened = R_MOD, vk.meta, vk.opened
    t0 = time.perf_counter()
    counts = _counts(meta)
    if len(instances) != meta["n_instances"] or any(not 0 <= v < R for v in instances):
        raise _Reject
    if meta["rows"] != 1 << meta["k"] or meta["chunk_len"] < 1 or meta["n_sets"] < 1 or any(name not in counts for ns in opened.values() for name in ns):
        raise _Reject
    # the proof's layout: the commitments up to h, the evaluations, W1, W2
    n_front = meta["n_cols"] + 2 * meta["n_lk"] + meta["n_sets"] + meta["n_lk"] + 1 + meta["chunk_len"] + 1
    n_evals = sum(counts[name] for names in opened.values() for name in names)
    if len(proof) != 32 * (n_front + n_evals + 2):
        raise _Reject
    ev_at = 32 * n_front
    pts, status = decompress(proof[:ev_at] + proof[ev_at + 32 * n_evals:], sign_bit)
    if status.any():
        raise _Reject
    evs = [int.from_bytes(proof[ev_at + 32 * i: ev_at + 32 * i + 32], "little") for i in range(n_evals)]
    if any(e >= R for e in evs):
        raise _Reject
    t["decompress"] = time.perf_counter() - t0

    # ---- the transcript, in the prover's order
    t0 = time.perf_counter()
    tr = api.Transcript()
    try:
        if sign_bit != 6:
            tr.set_sign_bit(sign_bit)
        pos = 0

        def points(m):
            nonlocal pos
            out = pts[pos: pos + m]
            pos += m
            if m:
                tr.common_points(out)
            return out
        tr.common_scalar(vk.digest())
        if instances:
            tr.common_scalars(fr_from_ints(instances))
        C = dict(vk.fixed)
        C["adv"] = points(counts["adv"])
        C["advg"] = C["adv"][: meta["n_adv"]]          # the gate columns, opened at rows 1..3 as a group of their own
        ch = {"theta": tr.squeeze()}
        pairs = points(2 * meta["n_lk"])
        C["pa"], C["ps"] = pairs[0::2], pairs[1::2]
        ch["beta"], ch["gamma"] = tr.squeeze(), tr.squeeze()
        C["zp"], C["zl"] = points(counts["zp"]), points(counts["zl"])
        C["rand"] = points(1)
        ch["y"] = tr.squeeze()
        C["h"] = points(meta["chunk_len"] + 1)          # the quotient's degree - 1 pieces
        ch["x"] = tr.squeeze()
        if n_evals:
            tr.common_scalars(fr_from_ints(evs))
        evals, k = {}, 0
        for rot, names in opened.items():
            for name in names:
                evals[(name, rot)] = evs[k: k + counts[name]]
                k += counts[name]
        ch["yo"], ch["v"] = tr.squeeze(), tr.squeeze()
        W1 = points(1)[0]
        ch["u"] = tr.squeeze()
        W2 = points(1)[0]
    finally:
        tr.free()
    ch = {name: fr_to_int(v) for name, v in ch.items()}
    t["transcript"] = time.perf_counter() - t0

    # ---- h folded at x: its value is what the quotient identity demands; its commitment sum_i [x^(n i)] H_i joins the MSM below
    t0 = time.perf_counter()
    x, yo, v, u = ch["x"], ch["yo"], ch["v"], ch["u"]
    xn = pow(x, meta["rows"], R)
    num = protocol.quotient_numerator(meta, ch, evals, instances)
    evals[("hf", 0)] = [num * pow((xn - 1) % R, -1, R) % R]
    for name in ("adv", "advg", "sel", "sigma", "cst", "table", "pa", "ps", "zp", "zl", "rand"):
        if any(name in ns for ns in opened.values()) and len(C[name]) != counts[name]:
            raise _Reject
    # ---- SHPLONK: one set per distinct set of rotations
    at = protocol.rotation_points(x, meta["k"], opened)
    sets = protocol.rotation_sets(opened)
    all_rots = sorted({rot for rots, _ in sets for rot in rots})
    m, scalars, bases, g_scalar = len(sets), [], [], 0
    for s_i, (rots, names) in enumerate(sets):
        vals = []
        for rot in rots:
            acc = 0
            for name in names:
                for e in evals[(name, rot)]:
                    acc = (acc * yo + e) % R
            vals.append(acc)
        r_u = protocol.horner(protocol.interpolate([at[rot] for rot in rots], vals), u)
        coef = pow(v, m - 1 - s_i, R) * protocol.vanishing([at[rot] for rot in all_rots if rot not in rots], u) % R
        n_commits = sum(1 if name == "hf" else len(C[name]) for name in names)
        powers, p = [0] * n_commits, coef
        for i in range(n_commits - 1, -1, -1):            # coef yo^(n_commits - 1 - i) for the i-th commitment of the set
            powers[i] = p
            p = p * yo % R
        i = 0
        for name in names:
            if name == "hf":                               # [s] hf = sum_j [s x^(n j)] H_j
                s, xj = powers[i], 1
                for _ in range(len(C["h"])):
                    scalars.append(s * xj % R)
                    xj = xj * xn % R
                bases.append(C["h"])
                i += 1
            else:
                scalars += powers[i: i + len(C[name])]
                bases.append(C[name])
                i += len(C[name])
        g_scalar = (g_scalar - coef * r_u) % R
    G1 = np.concatenate([_fq_mont(1), _fq_mont(2)])           # the generator (1, 2)
    scalars += [g_scalar, (-protocol.vanishing([at[rot] for rot in all_rots], u)) % R, u]
    bases += [G1.reshape(1, 8), W1.reshape(1, 8), W2.reshape(1, 8)]
    sc = fr_from_ints(scalars)
    t["algebra"] = time.perf_counter() - t0
    t0 = time.perf_counter()
    left = msm_points(np.concatenate(bases), sc)
    t["msm"] = time.perf_counter() - t0
    # ---- e(left, [1]_2) e(-W2, [tau]_2) = 1
    t0 = time.perf_counter()
    ok = pairing_check(np.stack([left, _neg_point(W2)]), np.stack([vk.g2, vk.tau_g2]))
    t["pairing"] = time.perf_counter() - t0
    return ok


def _fq_mont(v):
    """a small integer as a Montgomery Fq (4 uint64)"""
    m = (int(v) << 256) % Q_MOD
    return np.array([(m >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)], dtype=np.uint64)


_G2_ONE = None


def _g2_one():
    global _G2_ONE
    if _G2_ONE is None:
        _G2_ONE = _g2_generator_times(1)
    return _G2_ONE


class Verifier:
    """a proof file (io.write_snark) and its verifying key, ready to check"""

    def __init__(self, proof, instances, vk, sign_bit=6):
        self.proof, self.instances, self.vk, self.sign_bit = proof, list(instances), vk, sign_bit
        self.timings = {}

    @classmethod
    def from_files(cls, snark_path, vk_path, tau=None, sign_bit=6, params=None):
        """snark_path: io.write_snark's file; vk_path: save_verifying_key's .npz or halo2's RawBytes .vk (then tau is the SRS scalar,
        the reference's gen_srs scalar by default); params: a halo2 params file (or srs.ParamsKZG) whose g2 and [tau]_2 the pairing
        uses instead.  ValueError when either file is malformed."""
        from .io import read_snark
        proof, instances = read_snark(snark_path)
        return cls(proof, instances, VerifyingKey.read(vk_path, n_instances=len(instances), tau=tau, params=params), sign_bit)

    def verify(self):
        self.timings = {}
        return verify(self.proof, self.instances, self.vk, self.sign_bit, self.timings)
