"""The host side of the proof protocol, stated once for the prover (rounds.py), the verifier (verifier.py) and the key files (io.py):
the constants, the opening table, the verifying key's shape and digest, the quotient identity's numerator at x, and SHPLONK's host
algebra.  Plain functions over canonical Python integers and (4,) uint64 Montgomery limbs; the only library calls are constants of
the field (api.root_of_unity, api.fr_delta) and the digest's sponge (api.Transcript), all host code."""
from functools import lru_cache

import numpy as np

from . import api

R_MOD = 0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001
_R_INV = pow(1 << 256, -1, R_MOD)
# Rows at the end of every column that the prover fills with random scalars: halo2's blinding_factors() + 1.  blinding_factors() =
# max(3, advice queries per column) + 2 [UPSTREAM-RECALL]; halo2-base's vertical gate reads a column at four rotations, so 6 — which is
# what the reference's own MINIMUM_ROWS = 9 = blinding_factors() + 3 says (src/scaffold/mod.rs:383) — and the last usable row, where
# l_last sits and the running products end, is row 2^k - 7.  (Rounds 1-2 used 6.)
N_BLIND = 7
MINIMUM_ROWS = 9    # rows at the end of every column that the layout leaves free (src/scaffold/mod.rs:383)
FIXED = ("sel", "sigma", "cst", "table")     # the committed fixed polynomials, in the order the verifying key's digest absorbs their commitments
DERIVED = ("hf",)   # opened polynomials whose evaluation is not in the proof: the verifier computes it (h folded at x, from the quotient identity)
# (the Lagrange selectors l_0, l_last, l_active = 1 - l_last - l_blind the quotient multiplies by are not polynomials of the key: halo2
#  neither commits nor opens them, its verifier evaluates them at x from the domain — lagrange_evals below; the prover keeps their
#  cosets as key material, ProverRounds.fixed["lag"])


# The constraint system's degree, halo2 ConstraintSystem::degree() [UPSTREAM-RECALL; SURVEY App. C.4 / C.5]: the maximum of the
# permutation argument's required degree (3), the lookup arguments' (max(4, 2 + input degree + table degree) = 4: halo2-base's "lookup wo
# selector" reads one lookup-advice column against the table column, both of degree 1) and the gates' (the vertical gate
# q (a + b c - d): 3).  A circuit with lookup columns has degree 4; one without (merkle_commitment alone: the builder's auto-config
# gives it no lookup-advice column, so RangeConfig creates no lookup argument) degree 3.  Everything below follows from it the way
# halo2 derives it:
#   chunk_len = degree - 2   columns per product polynomial of the permutation argument (permutation::Argument)
#   n_h       = degree - 1   pieces of the quotient (quotient_poly_degree; extended domain 2^(k + ceil(log2(degree - 1))))
def constraint_degree(n_lookup_columns):
    return 4 if n_lookup_columns else 3


def fr_to_int(a):
    """(4,) Montgomery limbs -> canonical integer"""
    a = np.asarray(a, dtype=np.uint64).reshape(4)
    return sum(int(a[i]) << (64 * i) for i in range(4)) * _R_INV % R_MOD


def fr_from_int(v):
    """integer -> (4,) Montgomery limbs"""
    v = v % R_MOD * (1 << 256) % R_MOD
    return np.array([(v >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)], dtype=np.uint64)


def fr_from_ints(values):
    """integers -> (n, 4) Montgomery limbs"""
    raw = b"".join(((int(v) << 256) % R_MOD).to_bytes(32, "little") for v in values)
    return np.frombuffer(raw, dtype="<u8").astype(np.uint64).reshape(-1, 4)


@lru_cache(maxsize=None)
def omega(k):
    """the generator w of the domain of 2^k rows, canonical"""
    return fr_to_int(api.root_of_unity(k))


def opened(n_lk, n_blind=N_BLIND):
    """Which polynomial is opened at which rotation, in the order the proof carries the evaluations: the gate reads the advice at
    rows 0..3, the products one row ahead, the permuted input one row back, the chained product n_blind rows back.  A circuit without
    lookup columns opens no lookup polynomial (and so nothing at w^-1 x)."""
    names = {0: ["adv", "sel", "sigma", "cst", "table", "pa", "ps", "zp", "zl", "hf", "rand"], 1: ["advg", "zp", "zl"], 2: ["advg"], 3: ["advg"], -1: ["pa"],
             -n_blind: ["zp"]}
    lookup_only = {"pa", "ps", "zl"}
    table = {rot: [name for name in ns if n_lk or name not in lookup_only] for rot, ns in names.items()}
    return {rot: ns for rot, ns in table.items() if ns}


def key_meta(k, n_adv, n_lk, n_instances):
    """the circuit's shape as the verifying key states it: rows, k, n_adv, n_lk, n_cols (advice + lookup), n_sets (product polynomials
    of the permutation argument over [advice | lookup | constants | instance]), chunk_len, n_blind, delta (canonical), n_instances"""
    chunk_len = constraint_degree(n_lk) - 2
    n_cols = n_adv + n_lk
    return dict(rows=1 << k, k=k, n_adv=n_adv, n_lk=n_lk, n_cols=n_cols, n_sets=-(-(n_cols + 2) // chunk_len), chunk_len=chunk_len, n_blind=N_BLIND,
                delta=fr_to_int(api.fr_delta()), n_instances=n_instances)


def vk_digest(fixed):
    """The verifying key's entry into the transcript: ONE scalar, as halo2 absorbs vk.transcript_repr (a hash of the key made at
    keygen) — here the squeeze of a sponge of its own over every fixed commitment ({name: (m, 8) uint64}) in FIXED order"""
    tr = api.Transcript()
    try:
        for name in FIXED:
            tr.common_points(fixed[name])
        return tr.squeeze()
    finally:
        tr.free()


def instance_eval(instances, x, k):
    """The instance polynomial at x from the public values alone (what a verifier does instead of reading an evaluation from the
    proof): sum_i v_i L_i(x), L_i(x) = w^i (x^n - 1) / (n (x - w^i)) over the domain of 2^k rows.  Canonical integers."""
    n = 1 << k
    w = omega(k)
    if not instances:
        return 0
    xn1 = (pow(x, n, R_MOD) - 1) % R_MOD
    acc, wi = 0, 1
    dens = []
    for _ in instances:
        dens.append((x - wi) % R_MOD)
        wi = wi * w % R_MOD
    # one inversion for all denominators
    pref = [1]
    for d in dens:
        pref.append(pref[-1] * d % R_MOD)
    inv = pow(pref[-1], -1, R_MOD)
    wi_list = [pow(w, i, R_MOD) for i in range(len(instances))]
    for i in range(len(instances) - 1, -1, -1):
        di = inv * pref[i] % R_MOD
        inv = inv * dens[i] % R_MOD
        acc = (acc + int(instances[i]) * wi_list[i] % R_MOD * di) % R_MOD
    return acc * xn1 % R_MOD * pow(n, -1, R_MOD) % R_MOD


def lagrange_evals(x, k, usable):
    """(l_0(x), l_last(x), l_active(x)) as a verifier computes them (halo2 EvaluationDomain::l_i_range): l_i(x) = w^i (x^n - 1) / (n (x - w^i));
    l_last = l_usable, l_active = 1 - l_last - l_blind with l_blind the sum over the rows behind `usable`"""
    R, n = R_MOD, 1 << k
    w = omega(k)
    zn = (pow(x, n, R) - 1) * pow(n, -1, R) % R
    li = lambda i: pow(w, i, R) * zn % R * pow((x - pow(w, i, R)) % R, -1, R) % R
    l_last = li(usable)
    l_blind = sum(li(i) for i in range(usable + 1, n)) % R
    return li(0), l_last, (1 - l_last - l_blind) % R


def quotient_numerator(meta, ch, evals, instances):
    """The gate, permutation and lookup expressions recombined from the evaluations at x and the rotated points, in the order the
    prover's quotient combines them with powers of y: what must equal h(x) (x^n - 1).  meta: key_meta's dict; ch: the challenges
    beta, gamma, y, x; evals: (name, rotation) -> canonical integers; instances: the public values.  Raises ValueError when the
    evaluations do not have the shape meta describes."""
    R = R_MOD
    b, g, yv, x = ch["beta"], ch["gamma"], ch["y"], ch["x"]
    delta, n, n_adv, chunk, n_blind = meta["delta"], meta["rows"], meta["n_adv"], meta["chunk_len"], meta["n_blind"]
    ev = lambda name, rot=0: evals.get((name, rot), [])
    acc = 0
    a0, a1, a2, a3, q = ev("adv"), ev("advg", 1), ev("advg", 2), ev("advg", 3), ev("sel")
    if min(len(a0), len(a1), len(a2), len(a3), len(q)) < n_adv:
        raise ValueError("fewer gate evaluations than gate columns")
    for c in range(n_adv):
        acc = (acc * yv + q[c] * (a0[c] + a1[c] * a2[c] - a3[c])) % R
    usable = n - n_blind
    if not 0 < usable < n:
        raise ValueError("no usable rows")
    l0, ll, la = lagrange_evals(x, meta["k"], usable)
    sg, z0, z1, zb = ev("sigma"), ev("zp"), ev("zp", 1), ev("zp", -n_blind)
    # the permutation's columns: advice, lookup, the constants' fixed column, the instance column (from the public values)
    pcols = list(a0) + list(ev("cst")) + [instance_eval(instances, x, meta["k"])]
    n_cols, n_sets = len(pcols), len(z0)
    if n_cols != meta["n_cols"] + 2 or len(sg) != n_cols or n_sets == 0 or len(z1) < n_sets or len(zb) < n_sets - 1 or chunk < 1:
        raise ValueError("the permutation's evaluations do not match the key")
    if n_sets * chunk < n_cols or (n_sets - 1) * chunk >= n_cols:
        raise ValueError("the number of product polynomials does not match the key")
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
            raise ValueError("fewer lookup evaluations than lookup columns")
        S = ev("table")[0]
    for c in range(len(A)):
        acc = (acc * yv + l0 * (1 - Z[c])) % R
        acc = (acc * yv + ll * (Z[c] * Z[c] - Z[c])) % R
        acc = (acc * yv + la * (Z1[c] * (PA[c] + b) * (PS[c] + g) - Z[c] * (A[c] + b) * (S + g))) % R
        acc = (acc * yv + l0 * (PA[c] - PS[c])) % R
        acc = (acc * yv + la * (PA[c] - PS[c]) * (PA[c] - PAm[c])) % R
    return acc


# ---------------------------------------------------------------- SHPLONK's host algebra (halo2 poly/kzg/multiopen/shplonk)
def rotation_points(x, k, rotations):
    """{rotation: x w^rotation} over the domain of 2^k rows"""
    w = omega(k)
    return {rot: x * pow(w, rot % (1 << k), R_MOD) % R_MOD for rot in rotations}


def rotation_sets(opened):
    """the polynomials opened at the same set of rotations form one set: [(sorted rotations, [names])], in the order of their first
    polynomial in `opened`"""
    by_poly = {}
    for rot, names in opened.items():
        for name in names:
            by_poly.setdefault(name, []).append(rot)
    sets = {}
    for name, rots in by_poly.items():
        sets.setdefault(tuple(sorted(rots)), []).append(name)
    return list(sets.items())


def interpolate(pts, vals):
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


def horner(coeffs, z):
    """the polynomial with these coefficients (low first) at z"""
    acc = 0
    for c in reversed(coeffs):
        acc = (acc * z + c) % R_MOD
    return acc


def vanishing(pts, z):
    """prod_i (z - pts[i])"""
    acc = 1
    for p in pts:
        acc = acc * (z - p) % R_MOD
    return acc
