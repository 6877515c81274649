"""The Verify arm (the reference's SnarkCmd::Verify, src/scaffold/mod.rs:298-320; halo2's read_snark + verify_proof): checks a proof
that ProverRounds.prove() wrote against its verifying key.

    vk = VerifyingKey.read("kmeans.snark.vk.npz")          # or halo2's RawBytes data/{name}.vk (+ the SRS scalar)
    ok = verify(proof, instances, vk)                       # True / False, never raises on malformed input
    ok = Verifier.from_files("kmeans.snark", "kmeans.snark.vk.npz").verify()

The protocol is the one the prover runs (rounds.py), replayed from the proof bytes alone:
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

from . import _lib, api
from .api import DeviceBuffer, _p, _sz

R_MOD = 0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001
Q_MOD = 0x30644E72E131A029B85045B68181585D97816A916871CA8D3C208C16D87CFD47
_R_INV = pow(1 << 256, -1, R_MOD)
FIXED = ("sel", "sigma", "cst", "table")


def _fr_int(a):
    """Montgomery limbs -> canonical integer"""
    a = np.asarray(a, dtype=np.uint64).reshape(4)
    return sum(int(a[i]) << (64 * i) for i in range(4)) * _R_INV % R_MOD


def _fr_mont(values):
    """canonical integers -> (n, 4) Montgomery limbs"""
    raw = b"".join(((int(v) << 256) % R_MOD).to_bytes(32, "little") for v in values)
    return np.frombuffer(raw, dtype="<u8").astype(np.uint64).reshape(-1, 4)


def _default_opened(n_lk, n_blind):
    """which polynomial ProverRounds opens at which rotation (rounds.py; what a key without that record describes)"""
    names = {0: ["adv", "sel", "sigma", "cst", "table", "pa", "ps", "zp", "zl", "hf", "rand"], 1: ["advg", "zp", "zl"], 2: ["advg"], 3: ["advg"], -1: ["pa"],
             -n_blind: ["zp"]}
    lookup_only = {"pa", "ps", "zl"}
    opened = {rot: [n for n in ns if n_lk or n not in lookup_only] for rot, ns in names.items()}
    return {rot: ns for rot, ns in opened.items() if ns}


def _g2_generator_times(s):
    """[s] G2 as a vdb_g2 (16 uint64: x0, x1, y0, y1, Montgomery)"""
    out = np.zeros(16, dtype=np.uint64)
    api.check(_lib.load().vdb_g2_mul_generator(_p(_fr_mont([s % R_MOD])), _p(out)))
    return out


def vk_digest(fixed):
    """the key's one scalar in the transcript (halo2's vk.transcript_repr): the squeeze of a sponge of its own over every fixed
    commitment in FIXED order — ProverRounds.vk_digest's construction"""
    tr = api.Transcript()
    try:
        for name in FIXED:
            tr.common_points(fixed[name])
        return tr.squeeze()
    finally:
        tr.free()


class VerifyingKey:
    """The circuit's shape (meta: rows, k, n_adv, n_lk, n_cols, n_sets, chunk_len, n_blind, delta, n_instances), which polynomial is
    opened at which rotation, the fixed commitments ({name: (m, 8) uint64} for FIXED), and [tau]_2 — from the SRS scalar tau of the
    deterministic setup, or given as a vdb_g2 array — with the SRS's g2 (G2's generator unless given: a params file carries its own)."""

    def __init__(self, meta, fixed, opened=None, tau=None, tau_g2=None, g2=None):
        self.meta = {key: int(meta[key]) for key in ("rows", "k", "n_adv", "n_lk", "n_cols", "n_sets", "chunk_len", "n_blind", "delta", "n_instances")}
        self.fixed = {name: np.ascontiguousarray(fixed[name], dtype=np.uint64).reshape(-1, 8) for name in FIXED}
        self.opened = {int(rot): list(names) for rot, names in (opened or _default_opened(self.meta["n_lk"], self.meta["n_blind"])).items()}
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
        from .rounds import N_BLIND, _fr_to_int
        meta = dict(rows=pr.rows, k=pr.k, n_adv=pr.n_adv, n_lk=pr.n_lk, n_cols=pr.n_cols, n_sets=pr.n_sets, chunk_len=pr.chunk_len, n_blind=N_BLIND,
                    delta=_fr_to_int(pr.delta), n_instances=len(pr.instance_cells))
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
            if "vk_digest" in meta and _fr_int(vk.digest()) != meta["vk_digest"]:
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
            self._digest = vk_digest(self.fixed)
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


def _interpolate(pts, vals):
    """coefficients (low first) of the polynomial through (pts[i], vals[i])"""
    R = R_MOD
    coeffs = [0] * len(pts)
    for i, (xi, yi) in enumerate(zip(pts, vals)):
        basis, denom = [1], 1
        for j, xj in enumerate(pts):
            if j != i:
                basis = [(a - xj * b) % R for a, b in zip([0] + basis, basis + [0])]
                denom = denom * (xi - xj) % R
        scale = yi * pow(denom, -1, R) % R
        coeffs = [(c + scale * b) % R for c, b in zip(coeffs, basis)]
    return coeffs


def _instance_at(instances, x, k, w):
    """the instance column at x from the public values: sum_i v_i L_i(x), L_i(x) = w^i (x^n - 1) / (n (x - w^i))"""
    R, n = R_MOD, 1 << k
    acc, wi = 0, 1
    for v in instances:
        acc = (acc + v * wi * pow((x - wi) % R, -1, R)) % R
        wi = wi * w % R
    return acc * (pow(x, n, R) - 1) * pow(n, -1, R) % R


def quotient_numerator(meta, ch, evals, instances):
    """gates + permutation + lookup expressions recombined from the evaluations at x (the prover's quotient identity, rounds.py);
    raises _Reject when the evaluations do not have the shape the key describes"""
    R = R_MOD
    b, g, yv, x = ch["beta"], ch["gamma"], ch["y"], ch["x"]
    delta, n, n_adv, chunk, n_blind = meta["delta"], meta["rows"], meta["n_adv"], meta["chunk_len"], meta["n_blind"]
    ev = lambda name, rot=0: evals.get((name, rot), [])
    acc = 0
    a0, a1, a2, a3, q = ev("adv"), ev("advg", 1), ev("advg", 2), ev("advg", 3), ev("sel")
    if min(len(a0), len(a1), len(a2), len(a3), len(q)) < n_adv:
        raise _Reject
    for c in range(n_adv):
        acc = (acc * yv + q[c] * (a0[c] + a1[c] * a2[c] - a3[c])) % R
    w = _fr_int(api.root_of_unity(meta["k"]))
    zn = (pow(x, n, R) - 1) * pow(n, -1, R) % R
    l_at = lambda i: pow(w, i, R) * zn % R * pow((x - pow(w, i, R)) % R, -1, R) % R
    usable = n - n_blind
    if not 0 < usable < n:
        raise _Reject
    l0, ll = l_at(0), l_at(usable)
    la = (1 - ll - sum(l_at(i) for i in range(usable + 1, n))) % R
    sg, z0, z1, zb = ev("sigma"), ev("zp"), ev("zp", 1), ev("zp", -n_blind)
    # the permutation's columns: advice, lookup, the constants' fixed column, the instance column (from the public values)
    pcols = list(a0) + list(ev("cst")) + [_instance_at(instances, x, meta["k"], w)]
    n_cols, n_sets = len(pcols), len(z0)
    if n_cols != meta["n_cols"] + 2 or len(sg) != n_cols or n_sets == 0 or len(z1) < n_sets or len(zb) < n_sets - 1 or chunk < 1:
        raise _Reject
    if n_sets * chunk < n_cols or (n_sets - 1) * chunk >= n_cols:
        raise _Reject
    acc = (acc * yv + l0 * (1 - z0[0])) % R
    acc = (acc * yv + ll * (z0[-1] * z0[-1] - z0[-1])) % R
    for i in range(1, n_sets):
        acc = (acc * yv + l0 * (z0[i] - zb[i - 1])) % R
    cur = b * x % R
    for i in range(n_sets):
        left, right = z1[i], z0[i]
        for c in range(i * chunk, min((i + 1) * chunk, n_cols)):
            left = left * (pcols[c] + b * sg[c] + g) % R
            right = right * (pcols[c] + cur + g) % R
            cur = cur * delta % R
        acc = (acc * yv + la * (left - right)) % R
    A, PA, PS, PAm, Z, Z1 = a0[n_adv:], ev("pa"), ev("ps"), ev("pa", -1), ev("zl"), ev("zl", 1)
    if A:
        if not ev("table") or min(len(PA), len(PS), len(PAm), len(Z), len(Z1)) < len(A):
            raise _Reject
        S = ev("table")[0]
    for c in range(len(A)):
        acc = (acc * yv + l0 * (1 - Z[c])) % R
        acc = (acc * yv + ll * (Z[c] * Z[c] - Z[c])) % R
        acc = (acc * yv + la * (Z1[c] * (PA[c] + b) * (PS[c] + g) - Z[c] * (A[c] + b) * (S + g))) % R
        acc = (acc * yv + l0 * (PA[c] - PS[c])) % R
        acc = (acc * yv + la * (PA[c] - PS[c]) * (PA[c] - PAm[c])) % R
    return acc


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
            tr.common_scalars(_fr_mont(instances))
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
            tr.common_scalars(_fr_mont(evs))
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
    ch = {name: _fr_int(v) for name, v in ch.items()}
    t["transcript"] = time.perf_counter() - t0

    # ---- h folded at x: its value is what the quotient identity demands; its commitment sum_i [x^(n i)] H_i joins the MSM below
    t0 = time.perf_counter()
    x, yo, v, u = ch["x"], ch["yo"], ch["v"], ch["u"]
    xn = pow(x, meta["rows"], R)
    num = quotient_numerator(meta, ch, evals, instances)
    evals[("hf", 0)] = [num * pow((xn - 1) % R, -1, R) % R]
    for name in ("adv", "advg", "sel", "sigma", "cst", "table", "pa", "ps", "zp", "zl", "rand"):
        if any(name in ns for ns in opened.values()) and len(C[name]) != counts[name]:
            raise _Reject
    # ---- SHPLONK: one set per distinct set of rotations
    w = _fr_int(api.root_of_unity(meta["k"]))
    at = {rot: x * pow(w, rot % meta["rows"], R) % R for rot in opened}
    by_poly = {}
    for rot, names in opened.items():
        for name in names:
            by_poly.setdefault(name, []).append(rot)
    sets = []
    for name, rots in by_poly.items():
        key = tuple(sorted(rots))
        for sset in sets:
            if sset[0] == key:
                sset[1].append(name)
                break
        else:
            sets.append((key, [name]))
    all_rots = sorted({rot for rots, _ in sets for rot in rots})

    def vanish(rots, z):
        acc = 1
        for rot in rots:
            acc = acc * (z - at[rot]) % R
        return acc
    m, scalars, bases, g_scalar = len(sets), [], [], 0
    for s_i, (rots, names) in enumerate(sets):
        vals = []
        for rot in rots:
            acc = 0
            for name in names:
                for e in evals[(name, rot)]:
                    acc = (acc * yo + e) % R
            vals.append(acc)
        r_u = 0
        for c in reversed(_interpolate([at[rot] for rot in rots], vals)):
            r_u = (r_u * u + c) % R
        coef = pow(v, m - 1 - s_i, R) * vanish([rot for rot in all_rots if rot not in rots], u) % R
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
    scalars += [g_scalar, (-vanish(all_rots, u)) % R, u]
    bases += [G1.reshape(1, 8), W1.reshape(1, 8), W2.reshape(1, 8)]
    sc = _fr_mont(scalars)
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
