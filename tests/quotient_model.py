"""Python-integer restatement of the pointwise kernels of the quotient numerator (halo2_vectordb_amd/csrc/polyops.hip: k_perm_eval,
k_lookup_eval, k_gate_eval, k_poly_axpy, k_poly_scale, k_gather_fr) — one function per entry point of include/vdb.h, each with the
entry point's own arguments, arrays as Montgomery words (numpy uint64, last axis 4) and the accumulator returned instead of updated.

Everything is written from the formulas, on integers mod r: a term is computed whole at its point, the terms of a call are listed in
halo2's order, and the list is folded as acc <- acc y + term.  Nothing here knows about limbs, offsets or scalings.

Points.  Natural order of ne = 2^(k+e) points: X_j = zeta w_ne^j, one row is a step of 2^e (mod ne).  Coset by coset: slot t, row rho
is the point 4 rho + (0, 2, 1, 3)[t] of the natural order of 4 n points, one row is a step of 1 (mod n); arrays are [column][slot][row],
the accumulator and the l-selectors [slot][row].

tests/test_quotient_model_cpu.py holds this file to the mathematics (a satisfied instance's numerator vanishes on the rows, an altered
one's does not); tests/test_gpu_quotient_pointwise.py holds the kernels to this file, bit for bit."""
import functools

import numpy as np

from oracle import oracle as O

R = O.R_MOD
SLOT_POINT = (0, 2, 1, 3)


def scalar(a):
    return O.fr_to_ints(np.asarray(a, dtype=np.uint64).reshape(1, 4))[0]


def words(vals):
    return O.fr_from_ints(vals)


def _const(name, k=0):
    a = O.zeta() if name == "zeta" else O.root_of_unity(k)
    return scalar(a)


class Natural:
    """the 2^(k+e) points in their natural order"""
    def __init__(self, k, e):
        self.n, self.ne, self.step = 1 << k, 1 << (k + e), 1 << e
        w, x = _const("w", k + e), _const("zeta")
        self.X = []
        for _ in range(self.ne):
            self.X.append(x)
            x = x * w % R
        self.size = self.ne

    def rot(self, j, rows):
        return (j + rows * self.step) % self.ne

    def flat(self, a, lead):
        """(lead..., ne, 4) words -> list over the leading axis of lists of values per point"""
        if a is None:
            return None
        a = np.asarray(a, dtype=np.uint64).reshape(-1, self.ne, 4)
        return [O.fr_to_ints(c) for c in a]

    def shape(self):
        return (self.ne, 4)


class Cosets:
    """n_slots cosets of n points each out of the four of the 4 n-point domain; point index = slot * n + row"""
    def __init__(self, k, n_slots):
        assert 1 <= n_slots <= 4
        self.n, self.n_slots = 1 << k, n_slots
        w, zeta = _const("w", k + 2), _const("zeta")
        self.X = [zeta * pow(w, 4 * rho + SLOT_POINT[t], R) % R for t in range(n_slots) for rho in range(self.n)]
        self.size = n_slots * self.n

    def rot(self, j, rows):
        t, rho = divmod(j, self.n)
        return t * self.n + (rho + rows) % self.n

    def flat(self, a, lead):
        if a is None:
            return None
        a = np.asarray(a, dtype=np.uint64).reshape(-1, self.size, 4)
        return [O.fr_to_ints(c) for c in a]

    def shape(self):
        return (self.n_slots, self.n, 4)


@functools.lru_cache(maxsize=None)
def natural(k, e):
    return Natural(k, e)


@functools.lru_cache(maxsize=None)
def cosets(k, n_slots):
    return Cosets(k, n_slots)


def _fold(acc, y, terms):
    for t in terms:
        acc = (acc * y + t) % R
    return acc


# ---- permutation ------------------------------------------------------------------------------------------------------------------------
def _perm(dom, adv, adv_col0, sigma, z, z_set0, z_first, z_last, n_cols, chunk_len, usable, l0, l_last, l_active, beta, gamma, delta, y, acc,
          head, chain_lo, chain_hi, set_lo, set_hi):
    adv, sigma, z = dom.flat(adv, 1), dom.flat(sigma, 1), dom.flat(z, 1)
    z_first, z_last = dom.flat(z_first, 0), dom.flat(z_last, 0)
    l0, l_last, l_active, acc = (dom.flat(a, 0)[0] for a in (l0, l_last, l_active, acc))
    beta, gamma, delta, y = (scalar(a) for a in (beta, gamma, delta, y))
    back = dom.n - usable
    dbeta = [pow(delta, c, R) * beta % R for c in range(n_cols)]
    col = lambda c: adv[c - adv_col0]                      # the buffers are indexed globally
    sig = lambda c: sigma[c - set_lo * chunk_len]
    zs = lambda i: z[i - z_set0]
    out = []
    for j in range(dom.size):
        terms = []
        if head & 1:
            zf, zl = z_first[0][j], z_last[0][j]
            terms.append(l0[j] * (1 - zf))
            terms.append(l_last[j] * (zl * zl - zl))
        for i in range(chain_lo, chain_hi):
            terms.append(l0[j] * (zs(i)[j] - zs(i - 1)[dom.rot(j, -back)]))
        for i in range(set_lo, set_hi):
            left, right = zs(i)[dom.rot(j, 1)], zs(i)[j]
            for c in range(i * chunk_len, min((i + 1) * chunk_len, n_cols)):
                bs = sig(c)[j] if head & 2 else beta * sig(c)[j]
                left = left * (col(c)[j] + bs + gamma) % R
                right = right * (col(c)[j] + dbeta[c] * dom.X[j] + gamma) % R
            terms.append(l_active[j] * (left - right))
        out.append(_fold(acc[j], y, terms))
    return words(out).reshape(dom.shape())


def permutation_eval_parts_dev(adv, adv_col0, sigma, z, z_set0, z_first, z_last, n_cols, chunk_len, k, ext_k, usable, l0, l_last, l_active, beta,
                               gamma, delta, y, acc, head, chain_lo, chain_hi, set_lo, set_hi):
    return _perm(natural(k, ext_k), adv, adv_col0, sigma, z, z_set0, z_first, z_last, n_cols, chunk_len, usable, l0, l_last, l_active, beta, gamma,
                 delta, y, acc, head, chain_lo, chain_hi, set_lo, set_hi)


def permutation_eval_parts_cosets_dev(adv, adv_col0, sigma, z, z_set0, z_first, z_last, n_cols, chunk_len, k, n_slots, usable, l0, l_last, l_active,
                                      beta, gamma, delta, y, acc, head, chain_lo, chain_hi, set_lo, set_hi):
    return _perm(cosets(k, n_slots), adv, adv_col0, sigma, z, z_set0, z_first, z_last, n_cols, chunk_len, usable, l0, l_last, l_active, beta, gamma,
                 delta, y, acc, head, chain_lo, chain_hi, set_lo, set_hi)


def permutation_eval_range_dev(adv, sigma, z, n_cols, chunk_len, k, ext_k, usable, l0, l_last, l_active, beta, gamma, delta, y, acc, set_lo, set_hi):
    """everything resident (`sigma` still starts at the first column of set_lo): the head and all chaining terms come with set_lo == 0"""
    dom = natural(k, ext_k)
    n_sets = -(-n_cols // chunk_len)
    zz = np.asarray(z, dtype=np.uint64).reshape(-1, dom.ne, 4)
    first = set_lo == 0
    return _perm(dom, adv, 0, sigma, z, 0, zz[0], zz[n_sets - 1], n_cols, chunk_len, usable, l0, l_last, l_active, beta, gamma, delta, y, acc,
                 1 if first else 0, 1 if first else 0, n_sets if first else 0, set_lo, set_hi)


def permutation_eval_dev(adv, sigma, z, n_cols, chunk_len, k, ext_k, usable, l0, l_last, l_active, beta, gamma, delta, y, acc):
    return permutation_eval_range_dev(adv, sigma, z, n_cols, chunk_len, k, ext_k, usable, l0, l_last, l_active, beta, gamma, delta, y, acc, 0,
                                      -(-n_cols // chunk_len))


# ---- lookup -----------------------------------------------------------------------------------------------------------------------------
def _lookup(dom, inp, table, perm_in, perm_tab, z, n_cols, l0, l_last, l_active, beta, gamma, y, acc):
    inp, perm_in, perm_tab, z = (dom.flat(a, 1) for a in (inp, perm_in, perm_tab, z))
    table, l0, l_last, l_active, acc = (dom.flat(a, 0)[0] for a in (table, l0, l_last, l_active, acc))
    beta, gamma, y = (scalar(a) for a in (beta, gamma, y))
    out = []
    for j in range(dom.size):
        terms = []
        nxt, prv = dom.rot(j, 1), dom.rot(j, -1)
        for c in range(n_cols):
            a, s, ap, sp, zc = inp[c][j], table[j], perm_in[c][j], perm_tab[c][j], z[c][j]
            terms.append(l0[j] * (1 - zc))
            terms.append(l_last[j] * (zc * zc - zc))
            terms.append(l_active[j] * (z[c][nxt] * (ap + beta) * (sp + gamma) - zc * (a + beta) * (s + gamma)))
            terms.append(l0[j] * (ap - sp))
            terms.append(l_active[j] * (ap - sp) * (ap - perm_in[c][prv]))
        out.append(_fold(acc[j], y, terms))
    return words(out).reshape(dom.shape())


def lookup_eval_dev(inp, table, perm_in, perm_tab, z, n_cols, k, ext_k, l0, l_last, l_active, beta, gamma, y, acc):
    return _lookup(natural(k, ext_k), inp, table, perm_in, perm_tab, z, n_cols, l0, l_last, l_active, beta, gamma, y, acc)


def lookup_eval_cosets_dev(inp, table, perm_in, perm_tab, z, n_cols, k, n_slots, l0, l_last, l_active, beta, gamma, y, acc):
    return _lookup(cosets(k, n_slots), inp, table, perm_in, perm_tab, z, n_cols, l0, l_last, l_active, beta, gamma, y, acc)


# ---- gates ------------------------------------------------------------------------------------------------------------------------------
def gate_eval_sub_dev(adv, adv_ext_k, sel, n_cols, k, ext_k, y, acc):
    """the advice cosets live on 2^(k + adv_ext_k) points, selectors and accumulator on every 2^(adv_ext_k - ext_k)-th of them"""
    ne, na = 1 << (k + ext_k), 1 << (k + adv_ext_k)
    stride, row = 1 << (adv_ext_k - ext_k), 1 << adv_ext_k
    a = [O.fr_to_ints(c) for c in np.asarray(adv, dtype=np.uint64).reshape(-1, na, 4)]
    q = [O.fr_to_ints(c) for c in np.asarray(sel, dtype=np.uint64).reshape(-1, ne, 4)]
    h, yv = O.fr_to_ints(np.asarray(acc, dtype=np.uint64).reshape(ne, 4)), scalar(y)
    out = []
    for j in range(ne):
        at = lambda c, rows: a[c][(j * stride + rows * row) % na]
        out.append(_fold(h[j], yv, [q[c][j] * (at(c, 0) + at(c, 1) * at(c, 2) - at(c, 3)) for c in range(n_cols)]))
    return words(out).reshape(ne, 4)


def gate_eval_dev(adv, sel, n_cols, k, ext_k, y, acc):
    return gate_eval_sub_dev(adv, ext_k, sel, n_cols, k, ext_k, y, acc)


def gate_eval_cosets_dev(adv, adv_slots, sel, n_cols, k, n_slots, y, acc):
    """advice [column][adv_slots][row]; selectors [column][n_slots][row]; accumulator [n_slots][row]"""
    n = 1 << k
    a = np.asarray(adv, dtype=np.uint64).reshape(-1, adv_slots, n, 4)
    q = np.asarray(sel, dtype=np.uint64).reshape(-1, n_slots, n, 4)
    h = np.asarray(acc, dtype=np.uint64).reshape(n_slots, n, 4)
    yv = scalar(y)
    out = []
    for t in range(n_slots):
        at, qt, ht = [O.fr_to_ints(a[c, t]) for c in range(n_cols)], [O.fr_to_ints(q[c, t]) for c in range(n_cols)], O.fr_to_ints(h[t])
        for rho in range(n):
            cell = lambda c, rows: at[c][(rho + rows) % n]
            out.append(_fold(ht[rho], yv, [qt[c][rho] * (cell(c, 0) + cell(c, 1) * cell(c, 2) - cell(c, 3)) for c in range(n_cols)]))
    return words(out).reshape(n_slots, n, 4)


# ---- the others -------------------------------------------------------------------------------------------------------------------------
def poly_axpy_dev(acc, a, x, n):
    av = scalar(a)
    return words([(s + av * t) % R for s, t in zip(O.fr_to_ints(np.asarray(acc)[:n]), O.fr_to_ints(np.asarray(x)[:n]))])


def poly_scale_dev(x, a, n):
    av = scalar(a)
    return words([av * t % R for t in O.fr_to_ints(np.asarray(x)[:n])])


def gather_fr_dev(src, idx, n):
    src = np.asarray(src, dtype=np.uint64)
    return np.stack([src[int(i)] for i in np.asarray(idx)[:n]])
