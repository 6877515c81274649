"""Copy constraints of the fixed-point circuits: for every advice cell that the distance / nearest_vector /
k-means gadgets emit — /root/reference/src/gadget/{fixed_point,distance,vectordb}.rs on the halo2-base GateChip / RangeChip
cell templates — what kind of cell it is and, for copies, which earlier cell it copies.  This is what halo2-base records
while the reference's closure runs (`Existing(cell)` -> an equality with that cell, `Constant(c)` -> an equality with the
fixed column that holds c, `constrain_equal` / `assert_is_const` -> explicit equalities) and what `keygen_pk`
(src/scaffold/mod.rs:273) turns into the permutation argument.

The structure is data independent, so it is derived symbolically: `Sym` replays the gadgets' call tree with cell handles
instead of values, in exactly the cell order of halo2_vectordb_amd/csrc/gadgets.hpp and witness.hip (a copy arises wherever
the reference passes an assigned cell, by construction of the data flow here).  Small circuits are traced whole
(`trace_*`); the BASELINE-sized ones (hundreds of millions of cells) are assembled with numpy from traced unit blocks —
one distance, one per-vector assignment, one filter, one division — whose external inputs are resolved per instance
(`build_kmeans`, `build_nearest`).  tests/test_circuit_sym_cpu.py holds both against real witnesses: every gate flag,
every copy, every constant and every lookup source agree with the values of streams produced independently.

Cell codes of a traced block: src >= 0 copy of that block cell; SELF fresh witness; CONST constant (value in `cval`);
<= EXT0: external input number EXT0 - src.  [UPSTREAM-RECALL] for the halo2-base templates, as for the kernels.
"""
import math

import numpy as np

from .copymap import T, perm_cells, permutation_template

R = 0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001
SELF, CONST, EXT0 = -1, -2, -10
# the FixedPointInstructions calls of one operand (Sym.fp_op; what pipeline.FixedPointHotPath proves)
FP_UNARY_OPS = ("qexp2", "qlog2", "qsin", "qexp", "qlog", "qsqrt", "qabs", "is_neg", "neg", "signed_div_scale", "sign", "clip", "qcos", "qtan",
                "qsinh", "qcosh", "qtanh")

EXP2_COEF = [3.6240421303547230336183979205877e-11, 4.1284327467833130245549169910389e-10, 0.0000000071086385644026346316624185550542,
             0.00000010172297085296590958930245291448, 0.0000013215904023658396206789543841996, 0.000015252713316417140696221389106544,
             0.00015403531076657894204857389177279, 0.0013333558131297097698435464957392, 0.0096181291078409107025643582456283,
             0.055504108664804181586140094858174, 0.24022650695910142332414229540187, 0.69314718055994529934452147700678, 1.0]      # fixed_point.rs:138-160
LOG_COEF = [-3.319586265362338e-08, 1.4957235315170112e-06, -3.1350053389526744e-05, 0.00040554177582512901, -0.0036218342998850703,
            0.023663846121538389, -0.11691877183255484, 0.44524062371564499, -1.3195777548208449, 3.0518128028712077, -5.4904626000399528,
            7.6298580090181591, -8.1653313719804235, 7.1389971101896279, -3.1937385492842112]                                      # fixed_point.rs:162-187
SIN_COEF = [-1.1008071636607462e-11, 2.4208013888629323e-10, -3.8584805817996712e-10, -2.3786993104309845e-08, -2.9795813710683115e-09,
            2.7608543130047009e-06, -6.4467066994122565e-09, -0.00019840680551418068, -3.839555844512214e-09, 0.0083333350601673614,
            -5.0943769725466814e-10, -0.16666666657583049, -8.5029878414113731e-12, 1.0000000000003146, -1.9323057584419828e-15]  # fixed_point.rs:189-211


class C:
    """QuantumCell::Constant"""
    __slots__ = ("v",)

    def __init__(self, v):
        self.v = v % R


def ext(i):
    """handle of external input i of a block"""
    return EXT0 - i


def quantize(x, P):
    """fixed_point.rs:104-119 on a Python float: round half away from zero of |x| 2^P, negatives as r - q"""
    v = abs(x) * float(1 << P)
    q = int(math.floor(v))
    if v - math.floor(v) >= 0.5:
        q += 1
    return (R - q) % R if x < 0 else q


class Sym:
    """symbolic halo2-base Context: cell kinds instead of values"""

    def __init__(self, P, L):
        self.P, self.L = P, L
        self.src, self.gate, self.cval, self.asserted, self.lk = [], [], [], [], []

    def __len__(self):
        return len(self.src)

    # ------------------------------------------------------------------ Context
    def push(self, x, gate=False):
        p = len(self.src)
        if x is None:
            self.src.append(SELF)
            self.cval.append(None)
        elif isinstance(x, C):
            self.src.append(CONST)
            self.cval.append(x.v)
        else:
            assert x < p and (x >= 0 or x <= EXT0)
            self.src.append(x)
            self.cval.append(None)
        self.gate.append(bool(gate))
        return p

    def root(self, cell):
        while cell >= 0 and self.src[cell] >= 0:
            cell = self.src[cell]
        return cell

    def tie(self, a, fresh):
        """ctx.constrain_equal(a, fresh) where `fresh` is a witness cell of this block that copies nothing yet"""
        assert self.src[fresh] == SELF and a != fresh
        self.src[fresh] = a

    def tie_const(self, cell, value):
        """gate.assert_is_const(cell, value): the cell (through the cell it copies) is tied to the fixed column's `value`"""
        r = self.root(cell)
        assert r >= 0 and self.src[r] == SELF, "assert_is_const on a cell that is not rooted in this block"
        self.src[r] = CONST
        self.cval[r] = value % R
        self.asserted.append(r)

    def assign_witnesses(self, n):
        return [self.push(None) for _ in range(n)]

    def load_constant(self, v):
        return self.push(C(v))

    # ------------------------------------------------------------------ GateChip (flex_gate.rs)
    def g_add(self, a, b):
        self.push(a, True); self.push(b); self.push(C(1))
        return self.push(None)

    def g_sub(self, a, b):
        o = self.push(None, True)
        self.push(b); self.push(C(1)); self.push(a)
        return o

    def g_neg(self, a):
        self.push(a, True)
        o = self.push(None)
        self.push(C(1)); self.push(C(0))
        return o

    def g_mul(self, a, b):
        self.push(C(0), True); self.push(a); self.push(b)
        return self.push(None)

    def g_assert_bit(self, x):
        self.push(C(0), True); self.push(x); self.push(x); self.push(x)

    def g_not(self, a):
        return self.g_sub(C(1), a)

    def g_and(self, a, b):
        return self.g_mul(a, b)

    def g_or(self, a, b):
        nb = self.push(None, True)
        self.push(C(1)); self.push(b); self.push(C(1))
        self.push(b, True); self.push(a); self.push(nb)
        return self.push(None)

    def g_select(self, a, b, s):
        d = self.push(None, True)
        self.push(C(1)); self.push(b); self.push(a)
        self.push(b, True); self.push(s); self.push(d)
        return self.push(None)

    def g_is_zero(self, a):
        z = self.push(None, True)
        self.push(a); self.push(None); self.push(C(1))
        self.push(C(0), True); self.push(a)
        z2 = self.push(z)
        self.push(C(0))
        return z2                                            # ctx.get(-2)

    def g_is_equal(self, a, b):
        return self.g_is_zero(self.g_sub(a, b))

    def g_sum(self, cells):
        s = self.push(cells[0], len(cells) > 1)
        for i in range(1, len(cells)):
            self.push(cells[i]); self.push(C(1))
            s = self.push(None, i + 1 < len(cells))
        return s

    def g_select_by_indicator(self, cells, inds):
        n = len(cells)
        s = self.push(C(0), n > 0)
        for i in range(n):
            self.push(cells[i]); self.push(inds[i])
            s = self.push(None, i + 1 < n)
        return s

    def g_select_from_idx(self, cells, idx):
        inds = []
        for i in range(len(cells)):
            if i == 0:
                inds.append(self.g_is_zero(idx))             # the unrolled is_zero of idx_to_indicator
            else:
                d = self.push(None, True)                    # is_equal(idx, Constant(i)) = sub [d, i, 1, idx] + is_zero
                self.push(C(i)); self.push(C(1)); self.push(idx)
                inds.append(self.g_is_zero(d))
        return self.g_select_by_indicator(cells, inds)

    # ------------------------------------------------------------------ RangeChip (range.rs)
    def r_range_check(self, a, bits):
        L = self.L
        k, rem = -(-bits // L), bits % L
        if k == 1:
            self.lk.append(a)
            last = a
        else:
            limbs = [self.push(None, True)]
            acc = limbs[0]
            for i in range(1, k):
                limbs.append(self.push(None))
                self.push(C(1 << (i * L)))
                acc = self.push(None, i + 1 < k)
            self.tie(a, acc)                                 # ctx.constrain_equal(&a, &acc)
            self.lk.extend(limbs)
            last = limbs[-1]
        if rem == 1:
            self.g_assert_bit(last)
        elif rem > 1:
            last = self.g_mul(last, C(1 << (L - rem)))
            self.lk.append(last)
        return last

    def r_check_less_than(self, a, b, bits):
        chk = self.push(None, True)
        self.push(b); self.push(C(1))
        self.push(None, True)
        self.push(C(-(1 << bits))); self.push(C(1)); self.push(a)
        self.r_range_check(chk, bits)

    def r_check_big_less_than_safe(self, a, bound):
        rb = -(-bound.bit_length() // self.L) * self.L
        self.r_range_check(a, rb)
        self.r_check_less_than(a, C(bound), rb)

    def r_is_less_than(self, a, b, bits):
        padded = -(-bits // self.L) * self.L
        sh = self.push(None, True)
        self.push(b); self.push(C(1))
        self.push(None, True)
        self.push(C(-(1 << padded))); self.push(C(1)); self.push(a)
        return self.g_is_zero(self.r_range_check(sh, padded + self.L))

    def r_div_mod(self, a, shift, a_bits):
        """div_mod(a, 2^shift, a_bits) -> (div, rem)"""
        rem = self.push(None, True)
        self.push(C(1 << shift))
        div = self.push(None)
        self.push(a)
        self.r_check_big_less_than_safe(div, (1 << (a_bits - shift)) + 1)
        self.r_check_big_less_than_safe(rem, 1 << shift)
        return div, rem

    def r_div_mod_var(self, a, b, a_bits, b_bits):
        rem = self.push(None, True)
        self.push(b)
        div = self.push(None)
        self.push(a)
        self.r_range_check(div, a_bits)
        self.r_check_less_than(rem, b, b_bits)
        return div, rem

    # ------------------------------------------------------------------ FixedPointChip (fixed_point.rs)
    def is_neg(self, a):                                     # :523-539
        div, _ = self.r_div_mod(a, 2 * self.P + 1, 254)
        return self.g_not(self.g_is_zero(div))

    def qabs(self, a):                                       # :511-521
        rev = self.g_neg(a)
        n = self.is_neg(a)
        return self.g_select(rev, a, n)

    def cond_neg(self, a, flag):                             # :541-556
        return self.g_select(self.g_neg(a), a, flag)

    def signed_div_scale(self, a):                           # :974-1016
        P = self.P
        rem = self.push(None, True)
        self.push(C(1 << P))
        div = self.push(None)
        self.push(a)
        self.r_check_big_less_than_safe(rem, 1 << P)
        self.r_check_big_less_than_safe(self.qabs(div), 1 << (3 * P))
        return div

    def qmul(self, a, b):                                    # :588-604
        return self.signed_div_scale(self.g_mul(a, b))

    def bit_xor(self, a, b):                                 # :797-815
        a2 = self.g_add(C(0), a)
        b2 = self.g_add(C(0), b)
        self.g_assert_bit(a2)
        self.g_assert_bit(b2)
        ab = self.g_add(a2, b2)
        one = self.g_add(C(1), C(0))
        return self.g_is_equal(ab, one)

    def qdiv(self, a, b):                                    # :631-656
        P = self.P
        sa, sb = self.is_neg(a), self.is_neg(b)
        aa, ba = self.qabs(a), self.qabs(b)
        ar = self.g_mul(aa, C(1 << P))
        q, _ = self.r_div_mod_var(ar, ba, 4 * P, 2 * P)
        return self.cond_neg(q, self.bit_xor(sa, sb))

    def qmin(self, a, b):                                    # :936-952
        return self.g_select(a, b, self.is_neg(self.g_sub(a, b)))

    def polynomial(self, x, coef):                           # :658-686
        self.g_add(x, C(0))                                  # the dead qadd(x, 0)
        last, result = C(0), None
        for i, c in enumerate(coef):
            y = self.g_add(last, C(c))
            if i + 1 < len(coef):
                last = self.qmul(x, y)
            else:
                result = y
        return result

    def check_power_of_two(self, p2, e):                     # :688-708
        nb = 2 * self.P
        bits = [self.push(None, True)]                       # num_to_bits: inner_product(bits, pow_of_two), then assert_bit each
        acc = bits[0]
        for i in range(1, nb):
            bits.append(self.push(None))
            self.push(C(1 << i))
            acc = self.push(None, i + 1 < nb)
        self.tie(p2, acc)
        for b in bits:
            self.g_assert_bit(b)
        s = self.g_sum(bits)
        self.tie_const(self.g_is_zero(self.g_sub(s, C(1))), 1)
        bit = self.g_select_from_idx(bits, e)
        self.tie_const(self.g_is_zero(self.g_sub(bit, C(1))), 1)

    def qlog2(self, a):                                      # :736-795
        P = self.P
        a_assigned = self.g_add(a, C(0))
        is_neg = self.is_neg(a)
        is_zero = self.g_is_zero(a_assigned)
        self.tie_const(self.g_or(is_neg, is_zero), 0)
        pow1 = self.g_add(None, C(0))
        exp1 = self.g_add(None, C(0))
        self.check_power_of_two(pow1, exp1)
        pow2 = self.g_mul(pow1, C(2))
        exp2 = self.g_add(exp1, C(1))
        self.check_power_of_two(pow2, exp2)
        lt2 = self.r_is_less_than(a, pow2, 2 * P)
        gt1 = self.r_is_less_than(pow1, a, 2 * P)
        eq1 = self.g_is_equal(a, pow1)
        self.tie_const(self.g_and(lt2, self.g_or(eq1, gt1)), 1)
        shift = self.g_sub(C(P + 2), exp2)
        shift_neg = self.is_neg(shift)
        shift_abs = self.qabs(shift)
        spw = self.g_add(None, C(0))
        self.check_power_of_two(spw, shift_abs)
        a_ls = self.g_mul(a, spw)
        a_rs, _ = self.r_div_mod_var(a, spw, 2 * P, P + 1)
        a_norm = self.g_select(a_rs, a_ls, shift_neg)
        log_norm = self.polynomial(a_norm, [quantize(c, P) for c in LOG_COEF])
        lsq = self.g_mul(self.g_neg(shift), C(1 << P))
        return self.g_add(log_norm, lsq)

    def qexp2(self, a):                                      # :710-734
        P = self.P
        a_abs = self.qabs(a)
        ip, fpart = self.r_div_mod(a_abs, P, 2 * P)
        ip2 = self.g_select_from_idx([C(1 << i) for i in range(254)], ip)
        yf = self.polynomial(fpart, [quantize(c, P) for c in EXP2_COEF])
        res_pos = self.g_mul(ip2, yf)
        res_neg = self.qdiv(C(1 << P), res_pos)
        return self.g_select(res_neg, res_pos, self.is_neg(a))

    def qlog(self, a):                                       # :954-964
        l2e = self.load_constant(quantize(1.44269504088896340735992468100189214, self.P))
        return self.qdiv(self.qlog2(a), l2e)

    def qexp(self, a):                                       # :876-886
        ln2 = self.load_constant(quantize(0.693147180559945309417232121458176568, self.P))
        return self.qexp2(self.qdiv(a, ln2))

    def qsqrt(self, x):                                      # :966-972, 441-456
        half = self.load_constant(quantize(0.5, self.P))
        return self.qexp(self.qmul(half, self.qlog(x)))

    # the rest of FixedPointInstructions that examples/fixed_point.rs reaches
    def qmod(self, a, b):                                    # :606-629 (b: a positive constant or cell)
        P = self.P
        sa, sb = self.is_neg(a), self.is_neg(b)
        self.tie_const(sb, 0)                                # gate().assert_is_const(b_sign, 0)
        aa = self.qabs(a)
        _, r = self.r_div_mod_var(aa, b, 4 * P, 2 * P)
        return self.g_select(self.g_sub(b, r), r, sa)

    def qsin(self, a):                                       # :817-841
        P = self.P
        a_abs, a_sign = self.qabs(a), self.is_neg(a)
        a_mod = self.qmod(a_abs, C(quantize(math.pi * 2.0, P)))
        a_mpi = self.g_sub(a_mod, C(quantize(math.pi, P)))
        lower = self.is_neg(a_mpi)
        coef = [quantize(c, P) for c in SIN_COEF]
        s_mod = self.polynomial(a_mod, coef)
        s_mpi = self.g_neg(self.polynomial(a_mpi, coef))
        return self.cond_neg(self.g_select(s_mod, s_mpi, lower), a_sign)

    def sign(self, a):                                       # :558-569
        neg_one = self.g_neg(C(1))
        return self.g_select(neg_one, C(1), self.is_neg(a))

    def clip(self, a):                                       # :571-586
        sgn, aa = self.is_neg(a), self.qabs(a)
        _, rem = self.r_div_mod(aa, 2 * self.P, 254)
        return self.cond_neg(rem, sgn)

    def qcos(self, a):                                       # :843-852
        hp = self.load_constant(quantize(1.57079632679489661923132169163975144, self.P))
        return self.qsin(self.g_add(a, hp))

    def qtan(self, a):                                       # :383-393
        s = self.qsin(a)
        return self.qdiv(s, self.qcos(a))

    def _sinh_cosh(self, a, cosh):                           # :888-916
        ea = self.qexp(a)
        ena = self.qexp(self.g_neg(a))
        nume = self.g_add(ea, ena) if cosh else self.g_sub(ea, ena)
        return self.qdiv(nume, self.load_constant(quantize(2.0, self.P)))

    def qtanh(self, a):                                      # :407-417
        s = self._sinh_cosh(a, False)
        return self.qdiv(s, self._sinh_cosh(a, True))

    def fp_op(self, name, a):
        """one unary FixedPointInstructions call (the numbering of vdb_wit_fp_op names the same set)"""
        named = dict(neg=self.g_neg, qsinh=lambda x: self._sinh_cosh(x, False), qcosh=lambda x: self._sinh_cosh(x, True))
        return {op: named.get(op) or getattr(self, op) for op in FP_UNARY_OPS}[name](a)

    def inner_product(self, a, b):                           # :854-874
        res = self.g_add(C(0), C(0))
        for x, y in zip(a, b):
            res = self.g_add(res, self.qmul(x, y))
        return res

    # ------------------------------------------------------------------ DistanceChip (distance.rs)
    def distance(self, metric, a, b):
        if metric == "euclidean":                            # :97-119
            ab = [self.g_sub(x, y) for x, y in zip(a, b)]
            return self.qsqrt(self.inner_product(ab, ab))
        if metric == "cosine":                               # :121-144
            ab, aa, bb = self.inner_product(a, b), self.inner_product(a, a), self.inner_product(b, b)
            sa, sb = self.qsqrt(aa), self.qsqrt(bb)
            sim = self.qdiv(ab, self.qmul(sa, sb))
            return self.g_sub(self.load_constant(quantize(1.0, self.P)), sim)
        if metric == "manhattan":                            # :177-195
            d = [self.g_sub(x, y) for x, y in zip(a, b)]
            return self.g_sum([self.qabs(x) for x in d])
        if metric == "hamming":                              # :146-175; `len` and `ab_sum_q` are load_witness cells nothing ties
            s = self.g_sum([self.g_is_equal(x, y) for x, y in zip(a, b)])
            len_q, sum_q = self.push(None), self.push(None)
            sim = self.qdiv(sum_q, len_q)
            return self.g_sub(self.load_constant(quantize(1.0, self.P)), sim)
        raise ValueError(metric)

    # ------------------------------------------------------------------ VectorDBChip (vectordb.rs)
    def nearest_vector(self, metric, query, vectors):        # :122-163, distance(v, query)
        dist = [self.distance(metric, v, query) for v in vectors]
        m = dist[0]
        for d in dist[1:]:
            m = self.qmin(m, d)
        ind = [self.g_is_equal(m, d) for d in dist]
        res = [self.g_select_by_indicator([v[j] for v in vectors], ind) for j in range(len(query))]
        return ind, res

    def nearest_topk(self, metric, query, vectors, topk):
        """the topk nearest vectors (include/vdb.h vdb_wit_nearest_topk): nearest_vector's distances, then per round its qmin chain,
        is_equal and select_by_indicator over the entries the earlier rounds left, every winner replaced by Constant(M), M = 2^(2P) - 1,
        through gate.select before the next round; -> (indicators per round, results per round)"""
        assert 1 <= topk <= len(vectors)
        cur = [self.distance(metric, v, query) for v in vectors]
        big = C((1 << (2 * self.P)) - 1)
        inds, ress = [], []
        for r in range(topk):
            m = cur[0]
            for d in cur[1:]:
                m = self.qmin(m, d)
            ind = [self.g_is_equal(m, d) for d in cur]
            ress.append([self.g_select_by_indicator([v[j] for v in vectors], ind) for j in range(len(query))])
            inds.append(ind)
            if r + 1 < topk:
                cur = [self.g_select(big, d, i) for d, i in zip(cur, ind)]
        return inds, ress

    def kmeans(self, metric, vectors, K, I):                 # :225-362, distance(c, v)
        one = self.load_constant(quantize(1.0, self.P))
        zero = self.load_constant(0)
        cent = [list(v) for v in vectors[:K]]
        inds = None
        for _ in range(I):
            inds = []
            for v in vectors:
                inds.append(self.assign_block(one, zero, [self.distance(metric, c, v) for c in cent]))
            sizes = list(inds[0])
            for iv in inds[1:]:
                sizes = [self.g_add(s, x) for s, x in zip(sizes, iv)]
            for k in range(K):
                filt = [self.filter_block(zero, iv[k], v) for v, iv in zip(vectors, inds)]
                sums = list(filt[0])
                for f in filt[1:]:
                    sums = [self.g_add(x, s) for x, s in zip(f, sums)]                       # qadd(vector element, running sum)
                cent[k] = [self.qdiv(s, sizes[k]) for s in sums]
        return cent, inds

    def assign_block(self, one, zero, dist):
        """per vector: running qmin over its K distances, then (is_equal, select(one, zero, eq)) per cluster (:270-283)"""
        m = dist[0]
        for d in dist[1:]:
            m = self.qmin(m, d)
        return [self.g_select(one, zero, self.g_is_equal(m, d)) for d in dist]

    def filter_block(self, zero, sel, v):
        """is_zero(sel) and select(zero, v_j, is_zero) per dimension (:329-335)"""
        iz = self.g_is_zero(sel)
        return [self.g_select(zero, x, iz) for x in v]

    # ------------------------------------------------------------------ read-out
    def arrays(self):
        """(src, gate, const value index, constants, asserted cells, lookup sources) as numpy arrays of this block"""
        consts, cidx = {}, np.full(len(self.src), -1, dtype=np.int64)
        for p, v in enumerate(self.cval):
            if v is not None:
                cidx[p] = consts.setdefault(v, len(consts))
        return (np.asarray(self.src, dtype=np.int64), np.asarray(self.gate, dtype=bool), cidx, list(consts), np.asarray(self.asserted, dtype=np.int64),
                np.asarray(self.lk, dtype=np.int64))


# ---------------------------------------------------------------------------------------------------------------------------
# whole small circuits, cell by cell (the tests' ground truth for the block builders below)
class CopyMap:
    """copy constraints of a whole circuit over its flat advice stream:
    copy_of[i]    the earlier cell that cell i copies (i itself: none)
    const_idx[i]  index into `consts` (canonical integers) of the fixed-column value cell i is tied to, -1: none
    asserted[i]   the tie is an assert_is_const (the cell is a witness the circuit forces to that constant), not a Constant cell
    gate[i]       gate start
    lookup_src[j] the advice cell lookup cell j copies"""

    def __init__(self, copy_of, const_idx, consts, asserted, gate, lookup_src):
        self.copy_of, self.const_idx, self.consts, self.asserted, self.gate, self.lookup_src = copy_of, const_idx, consts, asserted, gate, lookup_src

    @property
    def n_cells(self):
        return self.copy_of.shape[0]

    def check_witness(self, values, lookup_values, flags=None):
        """every constraint of the map on a witness given as canonical Python / numpy integers (object arrays): returns a dict of
        violation counts.  `flags`: the kernels' flag bytes (bit 0 gate start, bit 1 constant): their gate bits must equal the
        map's and their constant bits must be a subset of the map's constants."""
        values = np.asarray(values, dtype=object)
        out = {}
        tied = np.flatnonzero(self.copy_of != np.arange(self.n_cells))
        out["copies_unequal"] = int(np.count_nonzero(values[tied] != values[self.copy_of[tied]]))
        cst = np.flatnonzero((self.const_idx >= 0) & ~self.asserted)
        out["constants_wrong"] = int(np.count_nonzero(values[cst] != np.asarray(self.consts, dtype=object)[self.const_idx[cst]]))
        asr = np.flatnonzero(self.asserted)
        out["asserts_violated"] = int(np.count_nonzero(values[asr] != np.asarray(self.consts, dtype=object)[self.const_idx[asr]]))
        lk = np.asarray(lookup_values, dtype=object)
        out["lookup_count"] = int(len(lk) != len(self.lookup_src))
        if len(lk) == len(self.lookup_src):
            out["lookup_copies_unequal"] = int(np.count_nonzero(lk != values[self.lookup_src])) if len(lk) else 0
        if flags is not None:
            flags = np.asarray(flags, dtype=np.uint8)
            out["gate_flags_differ"] = int(np.count_nonzero((flags & 1).astype(bool) != self.gate))
            out["kernel_constants_not_in_map"] = int(np.count_nonzero(((flags & 2) != 0) & ~((self.const_idx >= 0) & ~self.asserted)))
        return out


def _whole(sym, n_inputs):
    src, gate, cidx, consts, asserted, lk = sym.arrays()
    assert src.min() >= CONST, "external inputs in a whole circuit"
    n = len(src)
    copy_of = np.where(src >= 0, src, np.arange(n))
    am = np.zeros(n, dtype=bool)
    am[asserted] = True
    return CopyMap(copy_of, cidx, consts, am, gate, lk)


def trace_distance(metric, dim, P, L, n_pairs=1):
    """ctx.assign_witnesses(a); ctx.assign_witnesses(b); distance(a, b) — n_pairs times on the same two vectors (examples/euclid.rs)"""
    s = Sym(P, L)
    a, b = s.assign_witnesses(dim), s.assign_witnesses(dim)
    outs = [s.distance(metric, a, b) for _ in range(n_pairs)]
    return _whole(s, 2 * dim), outs


def trace_distances(metrics, dim, P, L):
    """ctx.assign_witnesses(a); ctx.assign_witnesses(b); then one distance after the other on the same two vectors
    (examples/distances.rs:40-59; pipeline.DistancesHotPath)"""
    s = Sym(P, L)
    a, b = s.assign_witnesses(dim), s.assign_witnesses(dim)
    outs = [s.distance(m, a, b) for m in metrics]
    return _whole(s, 2 * dim), outs


def trace_fixed_point(ops, P, L):
    """examples/fixed_point.rs:55-111: x = ctx.load_witness(..), then one FixedPointInstructions call after the other on x; -> the map and the
    cells the example makes public: x, then every result"""
    s = Sym(P, L)
    (x,) = s.assign_witnesses(1)
    outs = [x] + [s.fp_op(name, x) for name in ops]
    return _whole(s, 1), outs


def trace_nearest(metric, n, dim, P, L):
    s = Sym(P, L)
    q = s.assign_witnesses(dim)
    vs = [s.assign_witnesses(dim) for _ in range(n)]
    ind, res = s.nearest_vector(metric, q, vs)
    return _whole(s, (n + 1) * dim), (ind, res)


def trace_nearest_batch(metric, q, n, dim, P, L):
    """assign the q queries, assign the n database vectors, then nearest_vector(query, vectors) query after query over the same
    assigned database cells (pipeline.BatchQueryHotPath before its merkle_commitment); -> the map, (indicators (q, n), results (q, dim))"""
    s = Sym(P, L)
    qs = [s.assign_witnesses(dim) for _ in range(q)]
    vs = [s.assign_witnesses(dim) for _ in range(n)]
    outs = [s.nearest_vector(metric, qq, vs) for qq in qs]
    return _whole(s, (q + n) * dim), ([o[0] for o in outs], [o[1] for o in outs])


def trace_nearest_topk(metric, q, n, dim, topk, P, L):
    """assign the q queries, assign the n database vectors, then Sym.nearest_topk query after query over the same assigned database
    cells (pipeline.TopKQueryHotPath before its merkle_commitment); -> the map, (indicators (q, topk, n), results (q, topk, dim))"""
    s = Sym(P, L)
    qs = [s.assign_witnesses(dim) for _ in range(q)]
    vs = [s.assign_witnesses(dim) for _ in range(n)]
    outs = [s.nearest_topk(metric, qq, vs, topk) for qq in qs]
    return _whole(s, (q + n) * dim), ([o[0] for o in outs], [o[1] for o in outs])


def trace_kmeans(metric, n, dim, K, I, P, L):
    s = Sym(P, L)
    vs = [s.assign_witnesses(dim) for _ in range(n)]
    cent, inds = s.kmeans(metric, vs, K, I)
    return _whole(s, n * dim), (cent, inds)


# ---------------------------------------------------------------------------------------------------------------------------
# BASELINE-sized circuits: traced unit blocks, instantiated with numpy
class ConstPool:
    """the distinct fixed-column values of a map or of a block, numbered by first use"""

    def __init__(self):
        self.consts, self._cmap = [], {}

    def const_index(self, v):
        if v not in self._cmap:
            self._cmap[v] = len(self.consts)
            self.consts.append(v)
        return self._cmap[v]


class Block:
    """a traced unit with `n_ext` external inputs and `outs` (block cells handed to later blocks)"""

    def __init__(self, sym, outs):
        """`sym`: the Sym that traced the unit, or what its arrays() would return (from_arrays)"""
        self.src, self.gate, self.cidx, self.consts, self.asserted, self.lk = sym.arrays() if isinstance(sym, Sym) else sym
        self.n, self.n_lk, self.outs = len(self.src), len(self.lk), np.asarray(outs, dtype=np.int64)
        self.local = self.src >= 0
        self.isext = self.src <= EXT0
        self.ext_no = np.where(self.isext, EXT0 - self.src, 0)
        self.lk_isext = self.lk <= EXT0
        self.lk_ext_no = np.where(self.lk_isext, EXT0 - self.lk, 0)

    @classmethod
    def from_arrays(cls, src, gate, cidx, consts, asserted, lk, outs):
        """a unit that no Sym traced (the Poseidon permutation, whose template copymap.py holds)"""
        return cls((src, gate, cidx, consts, asserted, lk), outs)


class _Builder(ConstPool):
    def __init__(self, n_cells, n_lookup):
        super().__init__()
        self.copy_of = np.arange(n_cells, dtype=np.int64)
        self.const_idx = np.full(n_cells, -1, dtype=np.int64)
        self.asserted = np.zeros(n_cells, dtype=bool)
        self.gate = np.zeros(n_cells, dtype=bool)
        self.lookup_src = np.full(n_lookup, -1, dtype=np.int64)

    def constant_cell(self, pos, value):
        self.const_idx[pos] = self.const_index(value % R)

    def tie(self, cell, src):
        """ctx.constrain_equal(src, cell): `cell` (a placed block's fresh witness) copies the earlier cell `src`"""
        assert src < cell
        self.copy_of[cell] = src

    def place(self, blk, bases, lk_bases, ext_cells):
        """instances of `blk` at advice offsets `bases` (m,), lookup offsets `lk_bases` (m,), external inputs `ext_cells` (m, n_ext);
        returns the absolute cells of the block's outputs, (m, n_outs)"""
        bases = np.asarray(bases, dtype=np.int64).reshape(-1)
        m = bases.size
        ext_cells = np.asarray(ext_cells, dtype=np.int64).reshape(m, -1)
        remap = np.asarray([self.const_index(v) for v in blk.consts], dtype=np.int64)
        cid = np.where(blk.cidx >= 0, remap[np.maximum(blk.cidx, 0)] if len(remap) else -1, -1)
        step = max(1, (1 << 24) // max(blk.n, 1))                      # bounded temporaries
        for lo in range(0, m, step):
            b = bases[lo: lo + step, None]
            idx = b + np.arange(blk.n, dtype=np.int64)[None, :]
            val = np.where(blk.local[None, :], b + np.maximum(blk.src, 0)[None, :], idx)
            if blk.isext.any():
                val = np.where(blk.isext[None, :], ext_cells[lo: lo + step][:, blk.ext_no], val)
            self.copy_of[idx.reshape(-1)] = val.reshape(-1)
            self.const_idx[idx.reshape(-1)] = np.broadcast_to(cid[None, :], idx.shape).reshape(-1)
            self.gate[idx.reshape(-1)] = np.broadcast_to(blk.gate[None, :], idx.shape).reshape(-1)
            if blk.asserted.size:
                self.asserted[(b + blk.asserted[None, :]).reshape(-1)] = True
            if blk.n_lk:
                lb = np.asarray(lk_bases, dtype=np.int64).reshape(-1)[lo: lo + step, None]
                lval = np.where(blk.lk_isext[None, :], ext_cells[lo: lo + step][:, blk.lk_ext_no], b + np.maximum(blk.lk, 0)[None, :])
                self.lookup_src[(lb + np.arange(blk.n_lk, dtype=np.int64)[None, :]).reshape(-1)] = lval.reshape(-1)
        return bases[:, None] + blk.outs[None, :]

    def finish(self):
        assert (self.lookup_src >= 0).all(), "lookup cells without a source"
        return CopyMap(self.copy_of, self.const_idx, self.consts, self.asserted, self.gate, self.lookup_src)


def _distance_block(metric, dim, P, L):
    s = Sym(P, L)
    out = s.distance(metric, [ext(i) for i in range(dim)], [ext(dim + i) for i in range(dim)])
    return Block(s, [out])


def nearest_units(metric, n, dim, topk, P, L):
    """the unit blocks of Sym.nearest_topk over n vectors of `dim` words and where its stages lie: dict(db, qm, ie, sb, mk: the blocks of
    one distance, qmin, is_equal, select_by_indicator over n cells, select(Constant(M), ..); rounds_off / rounds_loff: where round 0 starts
    in a query's block; iseq_off, sel_off, mask_off: the stages of a round after its qmin chain; per_r / per_r_l, per_q / per_q_l: cells
    and lookup cells of a round that masks and of a query's block)"""
    if not 1 <= topk <= n:
        raise ValueError("topk must be at least 1 and at most n")
    u = dict(n=n, dim=dim, topk=topk, db=_distance_block(metric, dim, P, L))
    s = Sym(P, L)
    u["qm"] = Block(s, [s.qmin(ext(0), ext(1))])
    s = Sym(P, L)
    u["ie"] = Block(s, [s.g_is_equal(ext(0), ext(1))])
    s = Sym(P, L)
    u["sb"] = Block(s, [s.g_select_by_indicator([ext(k) for k in range(n)], [ext(n + k) for k in range(n)])])
    s = Sym(P, L)
    u["mk"] = Block(s, [s.g_select(C((1 << (2 * P)) - 1), ext(0), ext(1))])
    u["rounds_off"], u["rounds_loff"] = n * u["db"].n, n * u["db"].n_lk
    u["iseq_off"] = (n - 1) * u["qm"].n
    u["sel_off"] = u["iseq_off"] + u["ie"].n * n
    u["mask_off"] = u["sel_off"] + dim * u["sb"].n
    u["per_r"], u["per_r_l"] = u["mask_off"] + u["mk"].n * n, (n - 1) * u["qm"].n_lk
    u["per_q"], u["per_q_l"] = u["rounds_off"] + topk * u["per_r"] - u["mk"].n * n, u["rounds_loff"] + topk * u["per_r_l"]
    return u


def place_nearest(B, u, queries, vec, base, lbase):
    """q x Sym.nearest_topk(query_i, vectors, topk) placed into builder `B`: `u`: nearest_units of the shape; `queries` (q, dim) / `vec`
    (n, dim): the stream cells of the queries' and the vectors' words; query i's block starts at stream cell base + i per_q, its lookup cells
    at lbase + i per_q_l, in the stream order of witness.hip (nv_emit).  -> (indicators (q, topk, n), results (q, topk, dim))"""
    n, dim, topk = u["n"], u["dim"], u["topk"]
    db, qm, ie, sb, mk = u["db"], u["qm"], u["ie"], u["sb"], u["mk"]
    per_q, per_q_l, per_r, per_r_l = u["per_q"], u["per_q_l"], u["per_r"], u["per_r_l"]
    iseq_off, sel_off, mask_off = u["iseq_off"], u["sel_off"], u["mask_off"]
    queries, vec = np.asarray(queries, dtype=np.int64).reshape(-1, dim), np.asarray(vec, dtype=np.int64).reshape(n, dim)
    q = queries.shape[0]
    qq, ii = np.repeat(np.arange(q, dtype=np.int64), n), np.tile(np.arange(n, dtype=np.int64), q)
    bq, lbq = base + qq * per_q, lbase + qq * per_q_l
    cur = B.place(db, bq + ii * db.n, lbq + ii * db.n_lk, np.concatenate([vec[ii], queries[qq]], axis=1))[:, 0].reshape(q, n)
    qj, j = np.repeat(np.arange(q, dtype=np.int64), n - 1), np.tile(np.arange(n - 1, dtype=np.int64), q)
    qd, jd = np.repeat(np.arange(q, dtype=np.int64), dim), np.tile(np.arange(dim, dtype=np.int64), q)
    inds, ress = [], []
    for r in range(topk):
        rbase, rlbase = u["rounds_off"] + r * per_r, u["rounds_loff"] + r * per_r_l
        acc = np.empty((q, n), dtype=np.int64)
        acc[:, 0] = cur[:, 0]
        if n > 1:
            bases = base + qj * per_q + rbase + j * qm.n
            acc[:, 1:] = (bases + qm.outs[0]).reshape(q, n - 1)
            B.place(qm, bases, lbase + qj * per_q_l + rlbase + j * qm.n_lk, np.stack([acc[:, :-1].reshape(-1), cur[:, 1:].reshape(-1)], axis=1))
        ind = B.place(ie, bq + rbase + iseq_off + ie.n * ii, np.zeros(q * n, dtype=np.int64),
                      np.stack([acc[qq, n - 1], cur.reshape(-1)], axis=1))[:, 0].reshape(q, n)
        res = B.place(sb, base + qd * per_q + rbase + sel_off + jd * sb.n, np.zeros(q * dim, dtype=np.int64),
                      np.concatenate([vec.T[jd], ind[qd]], axis=1))[:, 0].reshape(q, dim)
        inds.append(ind)
        ress.append(res)
        if r + 1 < topk:
            cur = B.place(mk, bq + rbase + mask_off + mk.n * ii, np.zeros(q * n, dtype=np.int64),
                          np.stack([cur.reshape(-1), ind.reshape(-1)], axis=1))[:, 0].reshape(q, n)
    return np.stack(inds, axis=1), np.stack(ress, axis=1)


def build_nearest_topk(metric, q, n, dim, topk, P, L, builder=None, extra_cells=0, finish=True):
    """q x Sym.nearest_topk(query_i, vectors, topk) after [queries | vectors] have been assigned (tests/vectordb/mod.rs:220-247 assigns
    the query, then the vectors), in the stream order of witness.hip (wit_nearest_dev): the map the whole-circuit trace gives, assembled
    from one block per gadget (place_nearest).  Query i's block is its n distances, then per round n - 1 qmin, n is_equal, dim
    select_by_indicator and — before every round but the first — the n select(Constant(M), cur, ind) of the round before; the lookup cells
    are the distance runs, then the qmin runs round by round.  M is a constant of the map (a fixed-column value), tied to the cell that
    holds it in every select.  Outputs (indicators (q, topk, n), results (q, topk, dim)).  `extra_cells`: room for a gadget that follows
    in the same stream (the query circuits' merkle_commitment); with finish=False the builder itself is returned, (builder, outputs, cells
    used so far), for the caller to go on placing."""
    u = nearest_units(metric, n, dim, topk, P, L)
    n_in = (q + n) * dim
    total = n_in + q * u["per_q"]
    B = (builder or _Builder)(total + extra_cells, q * u["per_q_l"])
    queries = np.arange(q * dim, dtype=np.int64).reshape(q, dim)
    vec = q * dim + np.arange(n * dim, dtype=np.int64).reshape(n, dim)
    outs = place_nearest(B, u, queries, vec, n_in, 0)
    if not finish:
        return B, outs, total
    return B.finish(), outs


def _squeeze(built, axes):
    """a build_nearest_topk result with the axes of length one in `axes` taken out of its (indicators, results)"""
    return (built[0], tuple(np.squeeze(o, axis=axes) for o in built[1])) + tuple(built[2:])


def build_nearest_batch(metric, q, n, dim, P, L, builder=None, extra_cells=0, finish=True):
    """q x nearest_vector(query_i, vectors): build_nearest_topk at topk = 1, which emits no select(M, ..) and names no constant M;
    outputs (indicators (q, n), results (q, dim))"""
    return _squeeze(build_nearest_topk(metric, q, n, dim, 1, P, L, builder=builder, extra_cells=extra_cells, finish=finish), 1)


def build_nearest(metric, n, dim, P, L, builder=None, extra_cells=0, finish=True):
    """nearest_vector(query, vectors): build_nearest_topk at q = topk = 1; outputs (indicators (n,), result (dim,))"""
    return _squeeze(build_nearest_topk(metric, 1, n, dim, 1, P, L, builder=builder, extra_cells=extra_cells, finish=finish), (0, 1))


def build_kmeans(metric, n, dim, K, I, P, L, builder=None):
    """kmeans::<K, I>(vectors) after the vectors have been assigned (examples/kmeans.rs:40-49), in the stream order of
    witness.hip (KmLayout): [one, zero] then per iteration N x (K distances, assignment), the sizes chain, and per cluster
    (N filters, the sums chain, D divisions).  `builder`: the class that holds the map's arrays (default: numpy on the host;
    circuit_dev.DeviceBuilder assembles them on the GPU)"""
    db = _distance_block(metric, dim, P, L)
    s = Sym(P, L)
    ab = Block(s, s.assign_block(ext(0), ext(1), [ext(2 + k) for k in range(K)]))
    s = Sym(P, L)
    fb = Block(s, s.filter_block(ext(0), ext(1), [ext(2 + j) for j in range(dim)]))
    s = Sym(P, L)
    qd = Block(s, [s.qdiv(ext(0), ext(1))])
    s = Sym(P, L)
    add = Block(s, [s.g_add(ext(0), ext(1))])
    per_vec, per_vec_l = K * db.n + ab.n, K * db.n_lk + ab.n_lk
    assign, assign_l = n * per_vec, n * per_vec_l
    sizes = (n - 1) * K * 4
    per_cluster, per_cluster_l = n * fb.n + (n - 1) * dim * 4 + dim * qd.n, dim * qd.n_lk
    it_cells, it_lk = assign + sizes + K * per_cluster, assign_l + K * per_cluster_l
    n_in = n * dim
    total, total_l = n_in + 2 + I * it_cells, I * it_lk
    B = (builder or _Builder)(total, total_l)
    one, zero = n_in, n_in + 1
    B.constant_cell(one, quantize(1.0, P))
    B.constant_cell(zero, 0)
    vec = np.arange(n * dim, dtype=np.int64).reshape(n, dim)
    cent = vec[:K].copy()
    v = np.arange(n, dtype=np.int64)
    ind = None
    for it in range(I):
        pos, lpos = n_in + 2 + it * it_cells, it * it_lk
        vk = np.repeat(v, K)
        kk = np.tile(np.arange(K, dtype=np.int64), n)
        d = B.place(db, pos + vk * per_vec + kk * db.n, lpos + vk * per_vec_l + kk * db.n_lk, np.concatenate([cent[kk], vec[vk]], axis=1))[:, 0].reshape(n, K)
        ind = B.place(ab, pos + v * per_vec + K * db.n, lpos + v * per_vec_l + K * db.n_lk,
                      np.concatenate([np.full((n, 1), one), np.full((n, 1), zero), d], axis=1))          # (n, K)
        # cluster sizes: for v = 1 .. n-1, for k: qadd(size_k, ind[v][k]); the fold starts from ind[0]
        sb = pos + assign
        size_cells = ind[0].copy()
        if n > 1:
            vv = np.repeat(np.arange(1, n, dtype=np.int64), K)
            kk2 = np.tile(np.arange(K, dtype=np.int64), n - 1)
            bases = sb + (vv - 1) * 4 * K + 4 * kk2
            outs = bases + add.outs[0]
            prev = np.where(vv == 1, ind[0][kk2], outs - 4 * K)
            B.place(add, bases, np.zeros_like(bases), np.stack([prev, ind[vv, kk2]], axis=1))
            size_cells = outs.reshape(n - 1, K)[-1]
        new_cent = np.empty((K, dim), dtype=np.int64)
        for k in range(K):
            cb, clb = pos + assign + sizes + k * per_cluster, lpos + assign_l + k * per_cluster_l
            filt = B.place(fb, cb + v * fb.n, np.zeros(n, dtype=np.int64), np.concatenate([np.full((n, 1), zero), ind[:, k: k + 1], vec], axis=1))    # (n, dim)
            sums0 = cb + n * fb.n
            sum_cells = filt[0].copy()
            if n > 1:
                vv = np.repeat(np.arange(1, n, dtype=np.int64), dim)
                jj = np.tile(np.arange(dim, dtype=np.int64), n - 1)
                bases = sums0 + (vv - 1) * 4 * dim + 4 * jj
                outs = bases + add.outs[0]
                prev = np.where(vv == 1, filt[0][jj], outs - 4 * dim)
                B.place(add, bases, np.zeros_like(bases), np.stack([filt[vv, jj], prev], axis=1))    # qadd(vector element, running sum)
                sum_cells = outs.reshape(n - 1, dim)[-1]
            j = np.arange(dim, dtype=np.int64)
            new_cent[k] = B.place(qd, sums0 + (n - 1) * dim * 4 + j * qd.n, clb + j * qd.n_lk, np.stack([sum_cells, np.full(dim, size_cells[k])], axis=1))[:, 0]
        cent = new_cent
    return B.finish(), (cent, ind)


# ---------------------------------------------------------------------------------------------------------------------------
# merkle_commitment (src/gadget/vectordb.rs:165-223 through PoseidonChip<F, 3, 2>): copymap.py's permutation template as a unit block
def merkle_leaf_layout(dim):
    """the sponge of one leaf of `dim` words and one tree node: dict(nperm, n_ins: words each of the leaf's permutations absorbs,
    sizes: their cells, leaf_cells, node_cells: absorb [left, right], then the padding-only permutation)"""
    nperm = (dim + 1) // 2 + (1 if dim % 2 == 0 else 0)
    n_ins = [max(0, min(2, dim - 2 * p)) for p in range(nperm)]
    sizes = [perm_cells(k) for k in n_ins]
    return dict(nperm=nperm, n_ins=n_ins, sizes=sizes, leaf_cells=sum(sizes), node_cells=perm_cells(2) + perm_cells(0))


def _perm_block(flags, values, n_in, fresh, tied):
    """one PoseidonChip::permutation as a unit block (external inputs 0..2: the sponge state, 3..4: the absorbed words): `fresh`: the
    state is the chip's initial one (constants 2^64, 0, 0, though the kernels do not flag them) instead of external cells; `tied`: the
    words copy external cells.  `flags` / `values`: the kernel's flag bytes / the canonical values of one such permutation."""
    flags = np.asarray(flags, dtype=np.uint8)
    src, fin = permutation_template(flags, n_in)
    out = np.where(src >= 0, src, SELF).astype(np.int64)
    pool, cidx = ConstPool(), np.full(src.size, -1, dtype=np.int64)
    for i in np.flatnonzero(flags & 2):
        cidx[i] = pool.const_index(int(values[i]) % R)
    for i in range(T):
        cols = np.flatnonzero(src == -10 - i)
        if fresh:
            for c in cols:
                cidx[c] = pool.const_index((1 << 64) if i == 0 else 0)
        else:
            out[cols] = ext(i)
    if tied:
        for i in range(2):
            out[np.flatnonzero(src == -20 - i)] = ext(T + i)
    none = np.zeros(0, dtype=np.int64)
    return Block.from_arrays(out, (flags & 1).astype(bool), cidx, pool.consts, none, none, fin)


def _perm_placer(B, fetch_flags, fetch_values):
    """perm(bases, n_in, state, msgs): permutations absorbing n_in words placed into builder `B` at the stream cells `bases`; `state`:
    the T cell arrays of the state they go on from (None: the chip's initial state), `msgs`: the n_in cell arrays of the words (None:
    free cells); -> the T cell arrays of the final state.  One block per kind (n_in, fresh, tied), made from the flags and values of
    the first instance placed."""
    blocks = {}

    def perm(bases, n_in, state, msgs):
        fresh, tied = state is None, n_in > 0 and msgs is not None
        key = (n_in, fresh, tied)
        if key not in blocks:
            at, size = int(bases[0]), perm_cells(n_in)
            blocks[key] = _perm_block(fetch_flags(at, at + size), fetch_values(at, at + size), n_in, fresh, tied)
        e = np.zeros((bases.size, T + 2), dtype=np.int64)
        if not fresh:
            for i in range(T):
                e[:, i] = state[i]
        if tied:
            for i in range(n_in):
                e[:, T + i] = msgs[i]
        outs = B.place(blocks[key], bases, np.zeros(bases.size, dtype=np.int64), e)
        return [outs[:, i] for i in range(T)]
    return perm


def _node(perm, bases, left, right):
    """a tree node's hash placed at `bases`: the permutation absorbing [left, right], then the padding-only one -> the digest cells"""
    return perm(bases + perm_cells(2), 0, perm(bases, 2, None, [left, right]), [])[1]


def _place_leaf_sponge(perm, bases, lay, words):
    """the sponge of a leaf (lay: merkle_leaf_layout of its word count) placed at `bases`; words[k]: the cells its word k copies, one per
    base (words None: free words) -> (the squeeze cells, the first cell after each sponge)"""
    state, at = None, bases
    for p, n_in in enumerate(lay["n_ins"]):
        state = perm(at, n_in, state, None if words is None else [words[2 * p + i] for i in range(n_in)])
        at = at + lay["sizes"][p]
    return state[1], at


def place_merkle(B, n, dim, base, vec_base, fetch_flags, fetch_values, zero_cell=None):
    """merkle_commitment over n vectors of `dim` words whose trace starts at stream cell `base`, placed into builder `B` in the cell
    order of witness.hip: the leaves' sponges, the load_zero cell of the padding, the tree.  `vec_base`: stream cell of word 0 of
    vector 0 (the assigned vectors the leaves absorb; None: free words).  fetch_flags(lo, hi) / fetch_values(lo, hi): the kernel's
    flag bytes / the canonical values of stream cells [lo, hi) of a keygen-style run (one instance of each kind of permutation is
    read).  `zero_cell`: the cell an earlier ctx.load_zero() of the same circuit made (Context::load_zero caches it): the padding then
    copies that cell and the trace has none of its own.  -> (stream cell of the root, first cell after the trace)"""
    lay = merkle_leaf_layout(dim)
    perm = _perm_placer(B, fetch_flags, fetch_values)
    v = np.arange(n, dtype=np.int64)
    leaves, _ = _place_leaf_sponge(perm, base + v * lay["leaf_cells"], lay, None if vec_base is None else [vec_base + v * dim + k for k in range(dim)])
    lp, pos = 1 << (n - 1).bit_length(), base + n * lay["leaf_cells"]
    digest = np.full(lp, pos if zero_cell is None else zero_cell, dtype=np.int64)   # the padding leaves: the zero cell that follows the leaves
    digest[:n] = leaves
    if lp > n and zero_cell is None:
        B.constant_cell(pos, 0)                              # ctx.load_zero()
        pos += 1
    while digest.size > 1:
        bases = pos + np.arange(digest.size // 2, dtype=np.int64) * lay["node_cells"]
        digest = _node(perm, bases, digest[0::2], digest[1::2])
        pos += bases.size * lay["node_cells"]
    return int(digest[0]), pos


def build_merkle(n, dim, fetch_flags, fetch_values, builder=None):
    """the stand-alone Merkle circuit (examples/merkle.rs; pipeline.MerkleHotPath): the n * dim vector words assigned first
    (ctx.assign_witnesses, as the reference's chip_merkle does), then merkle_commitment over them (`builder`, fetch_flags,
    fetch_values: as build_merkle_update).  Constant cells are the cells the kernels flag, the zero cell of the padding and the
    sponge's initial state at the start of every leaf and tree node.  -> (CopyMap, root cell)"""
    n_in = n * dim
    if n < 1 or dim < 1:
        raise ValueError("a commitment is over at least one vector of at least one word")
    if np.asarray(fetch_flags(0, n_in)).any():
        raise ValueError("the assigned vector words carry no gate or constant flag")
    lay, lp = merkle_leaf_layout(dim), 1 << (n - 1).bit_length()
    total = n_in + n * lay["leaf_cells"] + (lp > n) + (lp - 1) * lay["node_cells"]
    B = (builder or _Builder)(total, 0)
    root, end = place_merkle(B, n, dim, n_in, 0, fetch_flags, fetch_values)
    if end != total:
        raise ValueError("the trace does not end where the circuit does")
    return B.finish(), root


def merkle_cells(n, dim, zero_cached=False):
    """cells of merkle_commitment over n vectors of `dim` words (vdb_wit_merkle_size)"""
    lay, lp = merkle_leaf_layout(dim), 1 << (n - 1).bit_length()
    return n * lay["leaf_cells"] + (1 if lp > n and not zero_cached else 0) + (lp - 1) * lay["node_cells"]


def place_sponge(B, base, words, fetch_flags, fetch_values):
    """poseidon.clear(); update(words); squeeze() over the stream cells `words` — merkle_commitment's leaf hash of one vector — placed
    into builder `B` from stream cell `base` on.  -> (stream cell of the digest, first cell after the trace)"""
    one = lambda c: np.asarray([c], dtype=np.int64)
    digest, end = _place_leaf_sponge(_perm_placer(B, fetch_flags, fetch_values), one(base), merkle_leaf_layout(len(words)), [one(w) for w in words])
    return int(digest[0]), int(end[0])


def ann_probe_layout(metric, K, sizes, dim, p, t, P, L):
    """where the blocks of the query over the p nearest clusters start (include/vdb.h vdb_wit_ann_probe); `sizes`: the size of the cluster
    round r of the centroid search states, r < p.  dict(query, centroids, candidates, roots: the assigned inputs; n_in; N; offsets (p + 1):
    candidate rows [offsets[r], offsets[r + 1]) are round r's cluster; nearest_c, merkle_c, nearest_m, merkle_m (p), select (p), sponge:
    the blocks; total; lk_m, total_l; units_c, units_m: nearest_units of the two searches at p and t rounds; zero_cell: the load_zero cell
    of the first padded tree among [centroids, members_0 ..] (None: none is padded); zero_cached (p): the members' tree copies it)"""
    sizes = [int(x) for x in sizes]
    if len(sizes) != p or not 1 <= p <= K or min(sizes) < 1:
        raise ValueError("one non-empty cluster per probe, at least 1 and at most K probes")
    N = sum(sizes)
    uc, um = nearest_units(metric, K, dim, p, P, L), nearest_units(metric, N, dim, t, P, L)
    leaf = merkle_leaf_layout(dim)["leaf_cells"]
    padded = lambda n: (1 << (n - 1).bit_length()) > n
    lay = dict(query=0, centroids=dim, candidates=dim + K * dim, roots=dim + K * dim + N * dim, N=N, units_c=uc, units_m=um,
               offsets=[sum(sizes[:r]) for r in range(p + 1)], sizes=sizes)
    lay["n_in"] = lay["nearest_c"] = lay["roots"] + K
    lay["merkle_c"] = lay["nearest_c"] + uc["per_q"]
    lay["nearest_m"] = lay["merkle_c"] + merkle_cells(K, dim)
    zero = lay["merkle_c"] + K * leaf if padded(K) else None
    at, lay["merkle_m"], lay["zero_cached"] = lay["nearest_m"] + um["per_q"], [], []
    for n_r in sizes:
        lay["merkle_m"].append(at)
        lay["zero_cached"].append(zero is not None)
        if padded(n_r) and zero is None:
            zero = at + n_r * leaf
        at += merkle_cells(n_r, dim, lay["zero_cached"][-1])
    lay["zero_cell"] = zero
    lay["select"] = [at + r * (1 + 3 * K) for r in range(p)]
    lay["sponge"] = at + p * (1 + 3 * K)
    lay["total"] = lay["sponge"] + merkle_leaf_layout(K + 1)["leaf_cells"]
    lay["lk_m"], lay["total_l"] = uc["per_q_l"], uc["per_q_l"] + um["per_q_l"]
    return lay


def build_ann_probe(metric, K, sizes, dim, p, t, P, L, fetch_flags, fetch_values, builder=None):
    """The query over the p nearest clusters that returns the t nearest candidates, in one circuit (pipeline.AnnProbeQueryHotPath):
    [query | centroids | candidates | cluster roots] assigned, then nearest_topk(query, centroids, p), merkle_commitment(centroids),
    nearest_topk(query, candidates, t), merkle_commitment(members_r) over the candidate rows of every round r — the padded trees sharing one
    zero cell, as Context::load_zero caches it —, p select_by_indicator(cluster roots, centroid indicators of round r), each TIED to the
    root of the members' tree of its round, and the sponge over [centroids' root | cluster roots].  build_ann_query is this at p = t = 1.
    -> (CopyMap, public cells: the t x dim result cells nearest first, then the index root, dict(centroid_indicators (p, K),
    candidate_indicators (t, N), results (t, dim), centroids_root, members_roots (p), selected (p), index_root, layout))"""
    if K < 1 or dim < 1:
        raise ValueError("at least one centroid and one word")
    lay = ann_probe_layout(metric, K, sizes, dim, p, t, P, L)
    if np.asarray(fetch_flags(0, lay["n_in"])).any():
        raise ValueError("the assigned inputs carry no gate or constant flag")
    N = lay["N"]
    B = (builder or _Builder)(lay["total"], lay["total_l"])
    query = np.arange(dim, dtype=np.int64).reshape(1, dim)
    cent = lay["centroids"] + np.arange(K * dim, dtype=np.int64).reshape(K, dim)
    cand = lay["candidates"] + np.arange(N * dim, dtype=np.int64).reshape(N, dim)
    roots = lay["roots"] + np.arange(K, dtype=np.int64)
    ind_c, _ = place_nearest(B, lay["units_c"], query, cent, lay["nearest_c"], 0)
    croot, end = place_merkle(B, K, dim, lay["merkle_c"], lay["centroids"], fetch_flags, fetch_values)
    assert end == lay["nearest_m"]
    ind_m, res = place_nearest(B, lay["units_m"], query, cand, lay["nearest_m"], lay["lk_m"])
    mroots = []
    for r in range(p):
        mroot, end = place_merkle(B, lay["sizes"][r], dim, lay["merkle_m"][r], lay["candidates"] + lay["offsets"][r] * dim, fetch_flags, fetch_values,
                                  zero_cell=lay["zero_cell"] if lay["zero_cached"][r] else None)
        assert end == (lay["merkle_m"][r + 1] if r + 1 < p else lay["select"][0])
        mroots.append(mroot)
    ind_c, ind_m, res = ind_c.reshape(p, K), ind_m.reshape(t, N), res.reshape(t, dim)
    sel = B.place(lay["units_c"]["sb"], lay["select"], np.zeros(p, dtype=np.int64), np.concatenate([np.broadcast_to(roots, (p, K)), ind_c], axis=1))[:, 0]
    for r in range(p):
        B.tie(int(sel[r]), mroots[r])                        # constrain_equal(sel_r, mroot_r)
    index_root, end = place_sponge(B, lay["sponge"], [croot] + [int(c) for c in roots], fetch_flags, fetch_values)
    if end != lay["total"]:
        raise ValueError("the trace does not end where the circuit does")
    public = [int(c) for c in res.reshape(-1)] + [index_root]
    return B.finish(), public, dict(centroid_indicators=ind_c, candidate_indicators=ind_m, results=res, centroids_root=croot, members_roots=mroots,
                                    selected=[int(c) for c in sel], index_root=index_root, layout=lay)


def _one_cluster(lay):
    """an ann_probe_layout at p = 1 with the one cluster's entries as scalars: members (= candidates), merkle_m, select, and zero_c: the
    centroids' padding loads the zero cell (the members' tree copies it)"""
    return dict(lay, members=lay["candidates"], merkle_m=lay["merkle_m"][0], select=lay["select"][0], zero_c=lay["zero_cached"][0])


def ann_query_layout(metric, K, n_c, dim, P, L):
    """where the blocks of the single-cluster query start (include/vdb.h vdb_wit_ann_query): ann_probe_layout at sizes = [n_c], p = t = 1,
    through _one_cluster"""
    return _one_cluster(ann_probe_layout(metric, K, [n_c], dim, 1, 1, P, L))


def build_ann_query(metric, K, n_c, dim, P, L, fetch_flags, fetch_values, builder=None):
    """The query of the nearest cluster alone that returns its nearest member (pipeline.AnnQueryHotPath): build_ann_probe at sizes = [n_c],
    p = t = 1.  -> (CopyMap, public cells: the dim result cells then the index root, dict(centroid_indicator (K,), member_indicator (n_c,),
    result (dim,), centroids_root, members_root, selected, index_root, layout: ann_query_layout's))"""
    cmap, public, info = build_ann_probe(metric, K, [n_c], dim, 1, 1, P, L, fetch_flags, fetch_values, builder=builder)
    return cmap, public, dict(centroid_indicator=info["centroid_indicators"][0], member_indicator=info["candidate_indicators"][0], result=info["results"][0],
                              centroids_root=info["centroids_root"], members_root=info["members_roots"][0], selected=info["selected"][0],
                              index_root=info["index_root"], layout=_one_cluster(info["layout"]))


# ---------------------------------------------------------------------------------------------------------------------------
# The Merkle path that updates and openings share: per level [assert_bit 4 | select 8 | select 8 | H] for the first running digest and
# [select 8 | select 8 | H] for a second one (an update's new path), then the index inner product over the bits
def _path_layout(dim, depth, sides):
    """merkle_leaf_layout(dim) with level_cells for `sides` running digests and ip_cells"""
    lay = merkle_leaf_layout(dim)
    lay.update(level_cells=20 + lay["node_cells"] + (sides - 1) * (16 + lay["node_cells"]), ip_cells=1 + 3 * (depth - 1))
    return lay


def _path_units(depth):
    """the unit blocks of a path: head (bit, sibling, cur) -> lo, ro behind assert_bit(bit); tail: the same two selects alone;
    ip (bits) -> inner_product(bits, Constant(2^l))"""
    s = Sym(0, 0)
    s.g_assert_bit(ext(0))
    head = Block(s, [s.g_select(ext(1), ext(2), ext(0)), s.g_select(ext(2), ext(1), ext(0))])
    s = Sym(0, 0)
    tail = Block(s, [s.g_select(ext(1), ext(2), ext(0)), s.g_select(ext(2), ext(1), ext(0))])
    s = Sym(0, 0)
    acc = s.push(ext(0), depth > 1)
    for l in range(1, depth):
        s.push(ext(l))
        s.push(C(1 << l))
        acc = s.push(None, l + 1 < depth)
    return head, tail, Block(s, [acc])


def _place_path(B, perm, lay, levels_at, bits, sibs, curs):
    """the levels and the index of the paths of all instances at once, level after level: levels_at: the first cell of each instance's
    level 0, bits / sibs: its (instance, level) cells, curs: the one or two arrays of leaf cells the running digests start from
    -> (the tops of the running digests, the index cells)"""
    depth = bits.shape[1]
    head, tail, ip = _path_units(depth)
    zeros, curs = np.zeros(levels_at.size, dtype=np.int64), list(curs)
    for l in range(depth):
        at = levels_at + l * lay["level_cells"]
        for k, cur in enumerate(curs):
            lr = B.place(tail if k else head, at, zeros, np.stack([bits[:, l], sibs[:, l], cur], axis=1))
            at = at + (16 if k else 20)
            curs[k] = _node(perm, at, lr[:, 0], lr[:, 1])
            at = at + lay["node_cells"]
    return curs, B.place(ip, levels_at + depth * lay["level_cells"], zeros, bits)[:, 0]


# ---------------------------------------------------------------------------------------------------------------------------
# Merkle path updates (include/vdb.h vdb_wit_merkle_update; pipeline.UpdateHotPath)
def merkle_update_layout(m, dim, depth, kinds=None, grow=0, carried=False):
    """where the cells of a batch of m path updates lie: dict(nperm, n_ins, sizes, leaf_cells, node_cells, level_cells, ip_cells,
    per_update, n_vec, old_leaf, bits, sibs, n_in, total) — the last five stream cells: [new vectors | old leaves | bits | siblings],
    then update j's block at n_in + j * per_update: its leaf sponge, per level [assert_bit 4 | select lo 8 | select ro 8 | H old |
    select ln 8 | select rn 8 | H new], the index inner product.
    kinds[j] = 1 makes update j a delete (one load_constant(0) cell in place of the sponge; only the w writes have a new vector) and
    `grow` doublings of the tree before the batch put R_0 behind the siblings and the growth block [Z_0 | depth - 1 hashes Z_{l+1} =
    H(Z_l, Z_l) | grow hashes R_{i+1} = H(R_i, Z_{d+i})] behind the assigned witnesses (`depth` is the grown one, d = depth - grow).
    Further keys: kinds, grow, w, write_no (per update: its row among the new vectors, -1 for a delete), r0 and z0 (cells; None when
    grow = 0), grow_cells, block and levels_at (per update: its first cell, the first cell of its level 0); per_update is the size of
    a write's block.  `carried` admits kind 2 (the index delete's move, ann_delete_layout): a carried leaf, ONE unflagged witness cell
    where a delete has its constant 0."""
    kinds = [0] * m if kinds is None else [int(k) for k in kinds]
    if m < 1 or depth < 1 or dim < 1:
        raise ValueError("a batch holds at least one update of a tree with at least two leaves")
    if len(kinds) != m or not set(kinds) <= ({0, 1, 2} if carried else {0, 1}) or grow < 0 or grow > depth:
        raise ValueError("one kind (0 write, 1 delete) per update, and no more doublings than the grown tree has levels")
    lay = _path_layout(dim, depth, 2)
    w = kinds.count(0)
    lay.update(n_vec=w * dim, old_leaf=w * dim, bits=w * dim + m, sibs=w * dim + m + m * depth, kinds=kinds, grow=grow, w=w)
    lay["per_update"] = lay["leaf_cells"] + depth * lay["level_cells"] + lay["ip_cells"]
    lay["n_in"] = w * dim + m * (1 + 2 * depth) + (1 if grow else 0)
    lay["r0"], lay["z0"] = (lay["n_in"] - 1, lay["n_in"]) if grow else (None, None)
    lay["grow_cells"] = 1 + (depth - 1 + grow) * lay["node_cells"] if grow else 0
    at, wn = lay["n_in"] + lay["grow_cells"], 0
    lay["block"], lay["levels_at"], lay["write_no"] = [], [], []
    for k in kinds:
        lay["block"].append(at)
        at += 1 if k else lay["leaf_cells"]
        lay["levels_at"].append(at)
        lay["write_no"].append(-1 if k else wn)
        wn += k == 0
        at += depth * lay["level_cells"] + lay["ip_cells"]
    lay["total"] = at
    return lay


def merkle_update_instances(m, top_old0, idx, old_leaf, new_leaf, top_new_last):
    """the public cells in make_public order: the old root, per update (idx, old leaf, new leaf), the new root"""
    out = [int(top_old0)]
    for j in range(m):
        out += [int(idx[j]), int(old_leaf[j]), int(new_leaf[j])]
    return out + [int(top_new_last)]


class _CellTrace:
    """the cell-by-cell tracer of the Merkle path circuits (trace_merkle_update, trace_merkle_open): the GateChip templates they use,
    written straight into copy_of / const_idx / gate.  fetch_flags / fetch_values: as trace_merkle_update."""

    def __init__(self, total, fetch_flags, fetch_values):
        self.total, self.fetch_flags, self.fetch_values = total, fetch_flags, fetch_values
        self.copy_of, self.cidx, self.gate = list(range(total)), [-1] * total, [False] * total
        self.consts, self.cmap, self.tmpl = [], {}, {}

    def cid(self, v):
        v %= R
        if v not in self.cmap:
            self.cmap[v] = len(self.consts)
            self.consts.append(v)
        return self.cmap[v]

    def put(self, at, cells, gates):
        """cells: ('c', earlier cell) | ('k', constant) | None (a new value)"""
        for i, (x, g) in enumerate(zip(cells, gates)):
            self.gate[at + i] = bool(g)
            if x is None:
                continue
            if x[0] == "k":
                self.cidx[at + i] = self.cid(x[1])
            else:
                self.copy_of[at + i] = x[1]
        return at + len(cells)

    def assert_bit(self, at, b):                             # [0, b, b, b]
        return self.put(at, [("k", 0), ("c", b), ("c", b), ("c", b)], [1, 0, 0, 0])

    def select(self, at, a, b, s):                           # [a - b, 1, b, a, b, sel, a - b, out]
        self.put(at, [None, ("k", 1), ("c", b), ("c", a), ("c", b), ("c", s), ("c", at), None], [1, 0, 0, 0, 1, 0, 0, 0])
        return at + 7

    def perm(self, at, n_in, state, msgs):
        if n_in not in self.tmpl:
            size = perm_cells(n_in)
            flags = np.asarray(self.fetch_flags(at, at + size), dtype=np.uint8)
            self.tmpl[n_in] = (permutation_template(flags, n_in), flags, self.fetch_values(at, at + size))
        (src, fin), flags, vals = self.tmpl[n_in]
        for i, s in enumerate(src.tolist()):
            p = at + i
            self.gate[p] = bool(flags[i] & 1)
            if flags[i] & 2:
                self.cidx[p] = self.cid(int(vals[i]))
            elif s >= 0:
                self.copy_of[p] = at + s
            elif s <= -20:
                self.copy_of[p] = msgs[-20 - s]
            elif s <= -10:
                if state is None:                            # the chip's initial state: capacity 2^64, then zeros
                    self.cidx[p] = self.cid((1 << 64) if s == -10 else 0)
                else:
                    self.copy_of[p] = state[-10 - s]
        return [at + f for f in fin]

    def node(self, at, left, right):
        st = self.perm(at, 2, None, [left, right])
        return self.perm(at + perm_cells(2), 0, st, [])[1]

    def leaf(self, at, lay, word0, words=None):
        """the sponge of one leaf over the assigned words word0, word0 + 1, ... (or over the cells `words`) -> (the squeeze cell, the
        first cell after it)"""
        state = None
        for p in range(lay["nperm"]):
            k = [2 * p + i for i in range(lay["n_ins"][p])]
            state = self.perm(at, lay["n_ins"][p], state, [word0 + i for i in k] if words is None else [words[i] for i in k])
            at += lay["sizes"][p]
        return state[1], at

    def is_zero(self, at, a):                                # [z, a, inv, 1, 0, a, z, 0] -> the second z (ctx.get(-2))
        self.put(at, [None, ("c", a), None, ("k", 1), ("k", 0), ("c", a), ("c", at), ("k", 0)], [1, 0, 0, 0, 1, 0, 0, 0])
        return at + 6

    def path(self, at, curs, bits, sibs):
        """the levels of a path from cell `at` on, for the one or two running digests that start at the cells `curs` (an update: its old
        and its new path), and the index behind them -> (the tops of the running digests, the index cell, the first cell after it)"""
        curs = list(curs)
        for b, sib in zip(bits, sibs):
            at = self.assert_bit(at, b)
            for k, cur in enumerate(curs):
                lo = self.select(at, sib, cur, b)
                ro = self.select(at + 8, cur, sib, b)
                curs[k] = self.node(at + 16, lo, ro)
                at += 16 + perm_cells(2) + perm_cells(0)
        idx_cell, at = self.index(at, bits)
        return curs, idx_cell, at

    def index(self, at, bits):
        """inner_product(bits, Constant(2^l)): 2^0 = 1, the sum starts with b_0 itself -> (the sum's cell, the first cell after it)"""
        depth = len(bits)
        cells, gates = [("c", bits[0])], [depth > 1]
        for l in range(1, depth):
            cells += [("c", bits[l]), ("k", 1 << l), None]
            gates += [0, 0, l + 1 < depth]
        at = self.put(at, cells, gates)
        return at - 1, at

    def finish(self):
        return CopyMap(np.asarray(self.copy_of, dtype=np.int64), np.asarray(self.cidx, dtype=np.int64), self.consts, np.zeros(self.total, dtype=bool),
                       np.asarray(self.gate, dtype=bool), np.zeros(0, dtype=np.int64))


def _trace_update_block(t, lay, base):
    """the cells of a batch of updates (lay: merkle_update_layout) traced into `t` from stream cell `base` on -> the public cells"""
    m, grow = len(lay["kinds"]), lay["grow"]
    dim, depth = lay["n_vec"] // max(lay["w"], 1), (lay["sibs"] - lay["bits"]) // m
    idx_cells, new_leaves, prev_top, top_old0 = [], [], None, None
    if grow:
        at = t.put(base + lay["z0"], [("k", 0)], [0])         # Z_0 = ctx.load_constant(0)
        z, prev_top = [base + lay["z0"]], base + lay["r0"]
        for l in range(depth - 1):
            z.append(t.node(at, z[l], z[l]))
            at += lay["node_cells"]
        for i in range(grow):
            prev_top = t.node(at, prev_top, z[depth - grow + i])
            at += lay["node_cells"]
        assert at == base + lay["block"][0]
    for j in range(m):
        if lay["kinds"][j]:
            cur_new = base + lay["block"][j]                 # new_leaf = ctx.load_constant(0), or the carried leaf: ctx.load_witness
            at = t.put(cur_new, [("k", 0) if lay["kinds"][j] == 1 else None], [0])
        else:
            cur_new, at = t.leaf(base + lay["block"][j], lay, base + lay["write_no"][j] * dim)
        assert at == base + lay["levels_at"][j]
        cur_old = base + lay["old_leaf"] + j
        new_leaves.append(cur_new)
        (cur_old, cur_new), idx_cell, at = t.path(at, [cur_old, cur_new], range(base + lay["bits"] + j * depth, base + lay["bits"] + (j + 1) * depth),
                                                  range(base + lay["sibs"] + j * depth, base + lay["sibs"] + (j + 1) * depth))
        idx_cells.append(idx_cell)
        assert at == base + (lay["block"][j + 1] if j + 1 < m else lay["total"])
        if j == 0:
            top_old0 = base + lay["r0"] if grow else cur_old
        if prev_top is not None:
            t.copy_of[cur_old] = prev_top                    # ctx.constrain_equal(cur_old, root_{j-1}) (update 0: R_grow)
        prev_top = cur_new
    return merkle_update_instances(m, top_old0, idx_cells, [base + lay["old_leaf"] + j for j in range(m)], new_leaves, prev_top)


def trace_merkle_update(m, dim, depth, fetch_flags, fetch_values, kinds=None, grow=0):
    """The closure of a batch of m path updates cell by cell (the ground truth of build_merkle_update): assign the witness groups, the
    growth block when the tree was grown, then per update the leaf sponge (a write) or the constant 0 (a delete), the levels and the
    index, the top of the old path tied to the top of the update before — that of update 0 to R_grow when the tree was grown.
    fetch_flags(lo, hi) / fetch_values(lo, hi): flag bytes / canonical values of stream cells of a keygen-style run (one instance of
    every kind of permutation is read: the Poseidon constants are fixed-column values).  -> (CopyMap, public cells)"""
    lay = merkle_update_layout(m, dim, depth, kinds, grow)
    t = _CellTrace(lay["total"], fetch_flags, fetch_values)
    public = _trace_update_block(t, lay, 0)
    return t.finish(), public


def place_merkle_update(B, m, dim, depth, fetch_flags, fetch_values, base=0, kinds=None, grow=0, carried=False):
    """trace_merkle_update's cells placed into builder `B` from stream cell `base` on, from unit blocks — one per kind of permutation,
    the bit with its two selects, the two selects of the new path, the index inner product — each placed for all m updates at once, level
    after level; the growth block's hashes one after the other, the constants (Z_0, each delete's 0) as fixed-column cells.
    A carried leaf (kind 2, `carried`) is one unflagged witness cell: nothing is placed for it.
    -> the public cells [old root | idx, old leaf, new leaf per update | new root]"""
    lay = merkle_update_layout(m, dim, depth, kinds, grow, carried)
    j = np.arange(m, dtype=np.int64)
    blocks = base + np.asarray(lay["block"], dtype=np.int64)
    perm = _perm_placer(B, fetch_flags, fetch_values)
    top = None
    if grow:
        B.constant_cell(base + lay["z0"], 0)                 # Z_0 = ctx.load_constant(0)
        one = lambda c: np.asarray([c], dtype=np.int64)
        z, top, at = [one(base + lay["z0"])], one(base + lay["r0"]), base + lay["z0"] + 1
        for l in range(depth - 1):
            z.append(_node(perm, one(at), z[l], z[l]))
            at += lay["node_cells"]
        for i in range(grow):
            top = _node(perm, one(at), top, z[depth - grow + i])
            at += lay["node_cells"]

    is_write = np.asarray(lay["kinds"], dtype=np.int64) == 0
    new_leaf = blocks.copy()                                 # a delete: its block starts with new_leaf = ctx.load_constant(0)
    for c in blocks[np.asarray(lay["kinds"], dtype=np.int64) == 1]:
        B.constant_cell(int(c), 0)
    if lay["w"]:
        word0 = base + np.arange(lay["w"], dtype=np.int64) * dim
        new_leaf[is_write], _ = _place_leaf_sponge(perm, blocks[is_write], lay, [word0 + k for k in range(dim)])
    path = base + j[:, None] * depth + np.arange(depth, dtype=np.int64)[None, :]
    (cur_old, cur_new), idx = _place_path(B, perm, lay, base + np.asarray(lay["levels_at"], dtype=np.int64), lay["bits"] + path, lay["sibs"] + path,
                                          [base + lay["old_leaf"] + j, new_leaf])
    if grow:
        B.tie(int(cur_old[0]), int(top[0]))                  # ctx.constrain_equal(cur_old, R_grow)
    for k in range(1, m):
        B.tie(int(cur_old[k]), int(cur_new[k - 1]))          # ctx.constrain_equal(cur_old, root_{j-1})
    return merkle_update_instances(m, base + lay["r0"] if grow else cur_old[0], idx, base + lay["old_leaf"] + j, new_leaf, cur_new[m - 1])


def build_merkle_update(m, dim, depth, fetch_flags, fetch_values, builder=None, kinds=None, grow=0):
    """trace_merkle_update's map assembled by place_merkle_update at stream cell 0 (`builder`: as build_kmeans).
    -> (CopyMap, public cells)"""
    lay = merkle_update_layout(m, dim, depth, kinds, grow)
    B = (builder or _Builder)(lay["total"], 0)
    public = place_merkle_update(B, m, dim, depth, fetch_flags, fetch_values, 0, kinds, grow)
    return B.finish(), public


# ---------------------------------------------------------------------------------------------------------------------------
# Inserts and replacements against the index root (include/vdb.h vdb_wit_ann_update; pipeline.AnnUpdateHotPath)
def _ann_frame_layout(K, sp, inner_cells):
    """The frame of a circuit against the index root (the update's and the delete's) around `inner_cells` cells of its own: dict(c,
    centroids_root, roots: the assigned header A; n_in; indicator B, select C, sponge_old D, update: the inner block, new_roots F,
    sponge_new G: the blocks; total; sponge: sp = merkle_leaf_layout(K + 1))"""
    if K < 1:
        raise ValueError("an index has at least one cluster")
    lay = dict(c=0, centroids_root=1, roots=2, n_in=K + 2, indicator=K + 2, sponge=sp)
    lay["select"] = lay["indicator"] + 8 + 12 * (K - 1)
    lay["sponge_old"] = lay["select"] + 1 + 3 * K
    lay["update"] = lay["sponge_old"] + sp["leaf_cells"]
    lay["new_roots"] = lay["update"] + inner_cells
    lay["sponge_new"] = lay["new_roots"] + 8 * K
    lay["total"] = lay["sponge_new"] + sp["leaf_cells"]
    return lay


def ann_update_layout(K, m, dim, depth, grow=0):
    """where the blocks of the index update circuit start: _ann_frame_layout's keys and update_layout: merkle_update_layout of block E
    (relative to `update`)"""
    upd = merkle_update_layout(m, dim, depth, None, grow)
    return dict(_ann_frame_layout(K, merkle_leaf_layout(K + 1), upd["total"]), update_layout=upd)


def _indicator_at(lay, j):
    return lay["indicator"] + (8 + 12 * (j - 1) if j else 0)


def ann_update_instances(index_root_old, c, update_public, index_root_new):
    """the public cells in make_public order: [index_root_old | c | idx, old leaf, new leaf per write | index_root_new] (the update
    block's own old and new roots are not public)"""
    return [int(index_root_old), int(c)] + [int(x) for x in update_public[1:-1]] + [int(index_root_new)]


def _trace_ann_head(t, lay):
    """blocks A - D of the frame on a _CellTrace: the header assigned, idx_to_indicator(c, K) as select_from_idx unrolls it,
    select_by_indicator(cluster roots, indicators) -> picked, the sponge over the header's roots.  -> (inds, picked, root_old)"""
    K = lay["n_in"] - 2
    c, roots = lay["c"], [lay["roots"] + j for j in range(K)]
    inds = [t.is_zero(lay["indicator"], c)]
    for j in range(1, K):
        at = _indicator_at(lay, j)
        t.put(at, [None, ("k", j), ("k", 1), ("c", c)], [1, 0, 0, 0])      # is_equal(c, Constant(j)) = sub [d, j, 1, c] + is_zero(d)
        inds.append(t.is_zero(at + 4, at))
    cells, gates = [("k", 0)], [1]
    for j in range(K):
        cells += [("c", roots[j]), ("c", inds[j]), None]
        gates += [0, 0, j + 1 < K]
    picked = t.put(lay["select"], cells, gates) - 1
    root_old, at = t.leaf(lay["sponge_old"], lay["sponge"], None, [lay["centroids_root"]] + roots)
    assert at == lay["update"]
    return inds, picked, root_old


def _trace_ann_tail(t, lay, inds, new_root):
    """blocks F and G: out_j = select(new_root, cluster_root_j, indicator_j), the sponge over [centroids_root | out_j].
    -> (outs, root_new)"""
    outs = [t.select(lay["new_roots"] + 8 * j, new_root, lay["roots"] + j, inds[j]) for j in range(len(inds))]
    root_new, at = t.leaf(lay["sponge_new"], lay["sponge"], None, [lay["centroids_root"]] + outs)
    assert at == lay["total"]
    return outs, root_new


def trace_ann_update(K, m, dim, depth, fetch_flags, fetch_values, grow=0):
    """The closure of m writes into one cluster of a committed index cell by cell (the ground truth of build_ann_update): the header
    [c | centroids_root | cluster roots] assigned, idx_to_indicator(c, K) as select_from_idx unrolls it, select_by_indicator(cluster
    roots, indicators) -> picked, the sponge over the header's roots, the update block (trace_merkle_update's cells), whose old root is
    tied to picked, out_j = select(new cluster root, cluster_root_j, indicator_j) and the sponge over [centroids_root | out_j].
    -> (CopyMap, public cells, dict(indicators, picked, old_root, new_root, outs, index_root_old, index_root_new, layout))"""
    lay = ann_update_layout(K, m, dim, depth, grow)
    t = _CellTrace(lay["total"], fetch_flags, fetch_values)
    inds, picked, root_old = _trace_ann_head(t, lay)
    upub = _trace_update_block(t, lay["update_layout"], lay["update"])
    t.copy_of[upub[0]] = picked                              # ctx.constrain_equal(picked, the update block's old root)
    outs, root_new = _trace_ann_tail(t, lay, inds, upub[-1])
    info = dict(indicators=inds, picked=picked, old_root=upub[0], new_root=upub[-1], outs=outs, index_root_old=root_old, index_root_new=root_new, layout=lay)
    return t.finish(), ann_update_instances(root_old, lay["c"], upub, root_new), info


def _build_ann_head(lay, fetch_flags, fetch_values, builder):
    """blocks A - D of the frame from unit blocks on a new builder: is_equal(c, Constant(j)) placed for all j >= 1 at once (its
    constant j set per instance), select_by_indicator over K cells, the sponge (place_sponge).  -> (B, inds, picked, root_old)"""
    if np.asarray(fetch_flags(0, lay["n_in"])).any():
        raise ValueError("the assigned header carries no gate or constant flag")
    B = (builder or _Builder)(lay["total"], lay.get("total_l", 0))
    K = lay["n_in"] - 2
    c, roots = lay["c"], lay["roots"] + np.arange(K, dtype=np.int64)
    s = Sym(0, 0)
    iz = Block(s, [s.g_is_zero(ext(0))])
    inds = [int(B.place(iz, [lay["indicator"]], [0], [[c]])[0, 0])]
    if K > 1:
        s = Sym(0, 0)
        d = s.push(None, True)                               # is_equal(c, Constant(j)) = sub [d, j, 1, c] + is_zero(d)
        s.push(None); s.push(C(1)); s.push(ext(0))
        ie = Block(s, [s.g_is_zero(d)])
        at = np.asarray([_indicator_at(lay, j) for j in range(1, K)], dtype=np.int64)
        inds += [int(x) for x in B.place(ie, at, np.zeros(K - 1, dtype=np.int64), np.full((K - 1, 1), c, dtype=np.int64))[:, 0]]
        for j in range(1, K):
            B.constant_cell(int(at[j - 1]) + 1, j)
    inds = np.asarray(inds, dtype=np.int64)
    s = Sym(0, 0)
    sb = Block(s, [s.g_select_by_indicator([ext(i) for i in range(K)], [ext(K + i) for i in range(K)])])
    picked = int(B.place(sb, [lay["select"]], [0], np.concatenate([roots, inds])[None, :])[0, 0])
    root_old, end = place_sponge(B, lay["sponge_old"], [lay["centroids_root"]] + [int(r) for r in roots], fetch_flags, fetch_values)
    assert end == lay["update"]
    return B, inds, picked, root_old


def _build_ann_tail(B, lay, inds, new_root, fetch_flags, fetch_values):
    """blocks F and G: the K selects placed at once, the sponge over [centroids_root | out_j].  -> (outs, root_new)"""
    K = len(inds)
    s = Sym(0, 0)
    sl = Block(s, [s.g_select(ext(0), ext(1), ext(2))])
    outs = B.place(sl, lay["new_roots"] + 8 * np.arange(K, dtype=np.int64), np.zeros(K, dtype=np.int64),
                   np.stack([np.full(K, new_root, dtype=np.int64), lay["roots"] + np.arange(K, dtype=np.int64), inds], axis=1))[:, 0]
    root_new, end = place_sponge(B, lay["sponge_new"], [lay["centroids_root"]] + [int(o) for o in outs], fetch_flags, fetch_values)
    if end != lay["total"]:
        raise ValueError("the trace does not end where the circuit does")
    return [int(o) for o in outs], root_new


def build_ann_update(K, m, dim, depth, fetch_flags, fetch_values, builder=None, grow=0):
    """trace_ann_update's map assembled from unit blocks: is_equal(c, Constant(j)) placed for all j >= 1 at once (its constant j set per
    instance), select_by_indicator over K cells, the two sponges (place_sponge), the update block (place_merkle_update at its base) and
    the K selects placed at once (`builder`: as build_kmeans).  -> as trace_ann_update"""
    lay = ann_update_layout(K, m, dim, depth, grow)
    B, inds, picked, root_old = _build_ann_head(lay, fetch_flags, fetch_values, builder)
    upub = place_merkle_update(B, m, dim, depth, fetch_flags, fetch_values, lay["update"], None, grow)
    B.tie(upub[0], picked)                                   # ctx.constrain_equal(picked, the update block's old root)
    outs, root_new = _build_ann_tail(B, lay, inds, upub[-1], fetch_flags, fetch_values)
    info = dict(indicators=[int(i) for i in inds], picked=picked, old_root=upub[0], new_root=upub[-1], outs=outs, index_root_old=root_old,
                index_root_new=root_new, layout=lay)
    return B.finish(), ann_update_instances(root_old, lay["c"], upub, root_new), info


# ---------------------------------------------------------------------------------------------------------------------------
# Linked writes: one batch against the database root and the index root (include/vdb.h vdb_wit_ann_write; pipeline.AnnWriteHotPath)
def ann_write_layout(K, m, dim, depth, grow, depth_db, grow_db):
    """where the blocks of the linked write start: ann_update_layout's keys (A - D, E at `update`, F, G; update_layout) with block E_db
    between E and F: update_db its first cell, update_db_layout merkle_update_layout of m carried updates at dim 1 on the database tree
    (`depth_db` the grown one)"""
    upd = merkle_update_layout(m, dim, depth, None, grow)
    upd_db = merkle_update_layout(m, 1, depth_db, [2] * m, grow_db, carried=True)
    lay = dict(_ann_frame_layout(K, merkle_leaf_layout(K + 1), upd["total"] + upd_db["total"]), update_layout=upd, update_db_layout=upd_db)
    lay["update_db"] = lay["update"] + upd["total"]
    return lay


def ann_write_instances(index_root_old, c, update_public, update_db_public, index_root_new):
    """the public cells in make_public order: [database_root_old | index_root_old | c | idx, db_idx, old leaf, new leaf per write |
    database_root_new | index_root_new] from the two update blocks' [old root | idx, old leaf, new leaf per update | new root]"""
    u, d = update_public, update_db_public
    out = [int(d[0]), int(index_root_old), int(c)]
    for j in range((len(u) - 2) // 3):
        out += [int(u[1 + 3 * j]), int(d[1 + 3 * j]), int(u[2 + 3 * j]), int(u[3 + 3 * j])]
    return out + [int(d[-1]), int(index_root_new)]


def _write_info(lay, m, upub, updb):
    """what both forms report about E and E_db: carried (the carried-leaf cell of E_db's update j), new_leaves (the squeeze of E's
    leaf sponge j, tied to it), old_leaves / old_leaves_db (the assigned old-leaf cells of the two blocks, tied), each block's roots"""
    u, db = lay["update_layout"], lay["update_db_layout"]
    return dict(carried=[lay["update_db"] + db["block"][j] for j in range(m)], new_leaves=[int(upub[3 + 3 * j]) for j in range(m)],
                old_leaves=[lay["update"] + u["old_leaf"] + j for j in range(m)], old_leaves_db=[lay["update_db"] + db["old_leaf"] + j for j in range(m)],
                old_root=int(upub[0]), new_root=int(upub[-1]), old_root_db=int(updb[0]), new_root_db=int(updb[-1]))


def trace_ann_write(K, m, dim, depth, fetch_flags, fetch_values, grow=0, depth_db=1, grow_db=0):
    """The closure of a linked write cell by cell (the ground truth of build_ann_write): trace_ann_update's blocks A - D and E, then E_db
    (the update block of the database tree, m carried updates), then F and G over E's final root.  Ties beyond trace_ann_update's: the
    carried leaf of E_db's update j to the new leaf E's update j hashed, the old leaf of E_db's update j to the old leaf of E's.
    -> (CopyMap, public cells, dict(trace_ann_update's keys and _write_info's))"""
    lay = ann_write_layout(K, m, dim, depth, grow, depth_db, grow_db)
    t = _CellTrace(lay["total"], fetch_flags, fetch_values)
    inds, picked, root_old = _trace_ann_head(t, lay)
    upub = _trace_update_block(t, lay["update_layout"], lay["update"])
    t.copy_of[upub[0]] = picked                              # ctx.constrain_equal(picked, the update block's old root)
    updb = _trace_update_block(t, lay["update_db_layout"], lay["update_db"])
    info = _write_info(lay, m, upub, updb)
    for x, y in zip(info["carried"], info["new_leaves"]):
        t.copy_of[x] = y                                     # THE LINK: the database gains the digest the cluster gains
    for x, y in zip(info["old_leaves_db"], info["old_leaves"]):
        t.copy_of[x] = y                                     # and loses the digest the cluster loses
    outs, root_new = _trace_ann_tail(t, lay, inds, upub[-1])
    info = dict(info, indicators=inds, picked=picked, outs=outs, index_root_old=root_old, index_root_new=root_new, layout=lay)
    return t.finish(), ann_write_instances(root_old, lay["c"], upub, updb, root_new), info


def build_ann_write(K, m, dim, depth, fetch_flags, fetch_values, builder=None, grow=0, depth_db=1, grow_db=0):
    """trace_ann_write's map assembled from unit blocks: build_ann_update's head and tail, place_merkle_update twice, the second with
    the carried kind (`builder`: as build_kmeans).  -> as trace_ann_write"""
    lay = ann_write_layout(K, m, dim, depth, grow, depth_db, grow_db)
    B, inds, picked, root_old = _build_ann_head(lay, fetch_flags, fetch_values, builder)
    upub = place_merkle_update(B, m, dim, depth, fetch_flags, fetch_values, lay["update"], None, grow)
    B.tie(upub[0], picked)                                   # ctx.constrain_equal(picked, the update block's old root)
    updb = place_merkle_update(B, m, 1, depth_db, fetch_flags, fetch_values, lay["update_db"], [2] * m, grow_db, carried=True)
    info = _write_info(lay, m, upub, updb)
    for x, y in zip(info["carried"], info["new_leaves"]):
        B.tie(x, y)                                          # THE LINK: the database gains the digest the cluster gains
    for x, y in zip(info["old_leaves_db"], info["old_leaves"]):
        B.tie(x, y)                                          # and loses the digest the cluster loses
    outs, root_new = _build_ann_tail(B, lay, inds, upub[-1], fetch_flags, fetch_values)
    info = dict(info, indicators=[int(i) for i in inds], picked=picked, outs=outs, index_root_old=root_old, index_root_new=root_new, layout=lay)
    return B.finish(), ann_write_instances(root_old, lay["c"], upub, updb, root_new), info


# ---------------------------------------------------------------------------------------------------------------------------
# Deletes against the index root (include/vdb.h vdb_wit_ann_delete; pipeline.AnnDeleteHotPath)
def ann_delete_shrink(n_c, m):
    """(depth of the cluster's tree over n_c members, the halvings s after m deletes: lp >> s is the power of two >= n_c - m)"""
    if not 1 <= m < n_c:
        raise ValueError("a batch holds at least one delete and leaves at least one member")
    depth = (n_c - 1).bit_length()
    return depth, depth - (n_c - m - 1).bit_length()


def ann_delete_layout(K, m, dim, depth, shrink=0):
    """where the blocks of the index delete circuit start: _ann_frame_layout's keys, update_layout (merkle_update_layout of block E' over
    the 2 m path updates [carried, delete] * m), `shrink`: the first cell of block S [S_0 | Z_0 | Z hashes depth - 1 | S hashes s]
    between E' and F, shrink_cells (0 when the tree keeps its size), s"""
    if m < 1 or not 0 <= shrink <= depth:
        raise ValueError("at least one delete, and no more halvings than the tree has levels")
    upd = merkle_update_layout(2 * m, dim, depth, [2, 1] * m, 0, carried=True)
    cells = 2 + (depth - 1 + shrink) * upd["node_cells"] if shrink else 0
    lay = _ann_frame_layout(K, merkle_leaf_layout(K + 1), upd["total"] + cells)
    return dict(lay, update_layout=upd, shrink=lay["update"] + upd["total"], shrink_cells=cells, s=shrink)


def ann_delete_instances(index_root_old, c, update_public, index_root_new):
    """the public cells in make_public order: [index_root_old | c | slot, removed leaf, last, moved leaf per delete | index_root_new] from
    the update block's [old root | idx, old leaf, new leaf per path update | new root]: delete j is updates 2 j and 2 j + 1"""
    u, out = update_public, [int(index_root_old), int(c)]
    for j in range((len(u) - 2) // 6):
        out += [int(u[1 + 6 * j]), int(u[2 + 6 * j]), int(u[4 + 6 * j]), int(u[3 + 6 * j])]
    return out + [int(index_root_new)]


def _delete_info(lay, m, upub, s0, top):
    """what both forms report about E' and S: carried (the carried-leaf cell of each delete), moved_old (the old-leaf cell it is tied
    to), s0, shrink_top (S_s), z0"""
    u, base = lay["update_layout"], lay["update"]
    return dict(carried=[base + u["block"][2 * j] for j in range(m)], moved_old=[base + u["old_leaf"] + 2 * j + 1 for j in range(m)], s0=s0, shrink_top=top,
                z0=lay["shrink"] + 1 if lay["s"] else None, old_root=upub[0], new_root=upub[-1])


def trace_ann_delete(K, m, dim, depth, fetch_flags, fetch_values, shrink=0):
    """The closure of m deletes from one cluster of a committed index cell by cell (the ground truth of build_ann_delete): blocks A - D
    (_trace_ann_head), the update block over 2 m path updates (a carried leaf into slot_j, then the last slot emptied), the carried
    cell tied to the old leaf of the update behind it, block S when the tree halves (its top tied to the update block's final root), F
    over the new cluster root (S_0, or the final root when nothing shrinks) and G.
    -> (CopyMap, public cells, dict(indicators, picked, old_root, new_root, outs, index_root_old, index_root_new, carried, moved_old, s0,
    shrink_top, z0, layout))"""
    lay = ann_delete_layout(K, m, dim, depth, shrink)
    t = _CellTrace(lay["total"], fetch_flags, fetch_values)
    inds, picked, root_old = _trace_ann_head(t, lay)
    upub = _trace_update_block(t, lay["update_layout"], lay["update"])
    t.copy_of[upub[0]] = picked                              # ctx.constrain_equal(picked, the update block's old root)
    s0, top = None, None
    info = _delete_info(lay, m, upub, None, None)
    for a, b in zip(info["carried"], info["moved_old"]):
        t.copy_of[a] = b                                     # the move: what left the last slot is what arrived
    new_root = upub[-1]
    if shrink:
        s0 = top = lay["shrink"]                             # S_0 = ctx.load_witness, Z_0 = ctx.load_constant(0)
        at = t.put(s0 + 1, [("k", 0)], [0])
        z = [s0 + 1]
        for l in range(depth - 1):
            z.append(t.node(at, z[l], z[l]))
            at += lay["update_layout"]["node_cells"]
        for i in range(shrink):
            top = t.node(at, top, z[depth - shrink + i])
            at += lay["update_layout"]["node_cells"]
        assert at == lay["new_roots"]
        t.copy_of[top] = upub[-1]                            # ctx.constrain_equal(S_s, the update block's final root)
        new_root = s0
    outs, root_new = _trace_ann_tail(t, lay, inds, new_root)
    info = dict(_delete_info(lay, m, upub, s0, top), indicators=inds, picked=picked, outs=outs, index_root_old=root_old, index_root_new=root_new, layout=lay)
    return t.finish(), ann_delete_instances(root_old, lay["c"], upub, root_new), info


def build_ann_delete(K, m, dim, depth, fetch_flags, fetch_values, builder=None, shrink=0):
    """trace_ann_delete's map assembled from unit blocks, as build_ann_update: the update block is place_merkle_update at its base with
    the carried kind, block S's hashes are placed one after the other (`builder`: as build_kmeans).  -> as trace_ann_delete"""
    lay = ann_delete_layout(K, m, dim, depth, shrink)
    B, inds, picked, root_old = _build_ann_head(lay, fetch_flags, fetch_values, builder)
    upub = place_merkle_update(B, 2 * m, dim, depth, fetch_flags, fetch_values, lay["update"], [2, 1] * m, 0, carried=True)
    B.tie(upub[0], picked)                                   # ctx.constrain_equal(picked, the update block's old root)
    info = _delete_info(lay, m, upub, None, None)
    for a, b in zip(info["carried"], info["moved_old"]):
        B.tie(a, b)                                          # the move: what left the last slot is what arrived
    s0, top, new_root = None, None, upub[-1]
    if shrink:
        one = lambda x: np.asarray([x], dtype=np.int64)
        perm = _perm_placer(B, fetch_flags, fetch_values)
        s0 = lay["shrink"]
        B.constant_cell(s0 + 1, 0)                           # Z_0 = ctx.load_constant(0)
        z, top, at = [one(s0 + 1)], one(s0), s0 + 2
        for l in range(depth - 1):
            z.append(_node(perm, one(at), z[l], z[l]))
            at += lay["update_layout"]["node_cells"]
        for i in range(shrink):
            top = _node(perm, one(at), top, z[depth - shrink + i])
            at += lay["update_layout"]["node_cells"]
        assert at == lay["new_roots"]
        top = int(top[0])
        B.tie(top, upub[-1])                                 # ctx.constrain_equal(S_s, the update block's final root)
        new_root = s0
    outs, root_new = _build_ann_tail(B, lay, inds, new_root, fetch_flags, fetch_values)
    info = dict(_delete_info(lay, m, upub, s0, top), indicators=[int(i) for i in inds], picked=picked, outs=outs, index_root_old=root_old,
                index_root_new=root_new, layout=lay)
    return B.finish(), ann_delete_instances(root_old, lay["c"], upub, root_new), info


# ---------------------------------------------------------------------------------------------------------------------------
# Moves from one cluster to another against the index root (include/vdb.h vdb_wit_ann_move; pipeline.AnnMoveHotPath)
def ann_move_shape(n_a, n_b, m):
    """(d_a, s, d_b, g): the depth of a's tree and its halvings after m members left (ann_delete_shrink), the depth of b's GROWN tree
    and the doublings after which it holds n_b + m members"""
    d_a, s = ann_delete_shrink(n_a, m)
    if n_b < 1:
        raise ValueError("an empty destination cluster")
    d_b = (n_b + m - 1).bit_length()
    return d_a, s, d_b, d_b - (n_b - 1).bit_length()


def ann_move_layout(K, m, depth_a, shrink, depth_b, grow):
    """where the blocks of the index move circuit start: a, b, centroids_root, roots (the assigned header A, n_in = K + 3 cells);
    indicator, select, sponge_old (B_a, C_a, D); update (E' on a's tree, update_layout: merkle_update_layout over [carried, delete] * m);
    shrink (block S, shrink_cells, s); mid (F_a); indicator_b, select_b (B_b, C_b); update_b (E_b on b's grown tree, update_b_layout: m
    carried appends, grow); new_roots (F_b); sponge_new (G); total.  No vector enters the circuit: the update layouts are taken at dim 1,
    which no cell of theirs depends on."""
    if K < 2:
        raise ValueError("a move needs two clusters")
    if m < 1 or not 0 <= shrink <= depth_a:
        raise ValueError("at least one move, and no more halvings than the tree has levels")
    upd_a = merkle_update_layout(2 * m, 1, depth_a, [2, 1] * m, 0, carried=True)
    upd_b = merkle_update_layout(m, 1, depth_b, [2] * m, grow, carried=True)
    sp = merkle_leaf_layout(K + 1)
    ind_cells, sel_cells = 8 + 12 * (K - 1), 1 + 3 * K
    lay = dict(K=K, a=0, b=1, c=0, centroids_root=2, roots=3, n_in=K + 3, sponge=sp, update_layout=upd_a, update_b_layout=upd_b, s=shrink, g=grow)
    lay["indicator"] = K + 3
    lay["select"] = lay["indicator"] + ind_cells
    lay["sponge_old"] = lay["select"] + sel_cells
    lay["update"] = lay["sponge_old"] + sp["leaf_cells"]
    lay["shrink"] = lay["update"] + upd_a["total"]
    lay["shrink_cells"] = 2 + (depth_a - 1 + shrink) * upd_a["node_cells"] if shrink else 0
    lay["mid"] = lay["shrink"] + lay["shrink_cells"]
    lay["indicator_b"] = lay["mid"] + 8 * K
    lay["select_b"] = lay["indicator_b"] + ind_cells
    lay["update_b"] = lay["select_b"] + sel_cells
    lay["new_roots"] = lay["update_b"] + upd_b["total"]
    lay["sponge_new"] = lay["new_roots"] + 8 * K
    lay["total"] = lay["sponge_new"] + sp["leaf_cells"]
    return lay


def ann_move_instances(index_root_old, a, b, public_a, public_b, index_root_new):
    """the public cells in make_public order: [index_root_old | a | b | slot, leaf, last, moved leaf, dest, dest old leaf per move |
    index_root_new] from the two update blocks' [old root | idx, old leaf, new leaf per path update | new root]: move j is updates 2 j
    and 2 j + 1 of a's block and update j of b's"""
    ua, ub, out = public_a, public_b, [int(index_root_old), int(a), int(b)]
    for j in range((len(ub) - 2) // 3):
        out += [int(ua[1 + 6 * j]), int(ua[2 + 6 * j]), int(ua[4 + 6 * j]), int(ua[3 + 6 * j]), int(ub[1 + 3 * j]), int(ub[2 + 3 * j])]
    return out + [int(index_root_new)]


def _move_info(lay, m, upa, upb):
    """what both forms report about E', S and E_b: carried / moved_old (the delete's own move copy inside a), removed (the assigned
    old-leaf cell of E''s update 2 j: the removed leaf), arrived (the carried-leaf cell of E_b's update j, tied to it), z0, and each
    block's own roots"""
    u, base, ub, base_b = lay["update_layout"], lay["update"], lay["update_b_layout"], lay["update_b"]
    return dict(carried=[base + u["block"][2 * j] for j in range(m)], moved_old=[base + u["old_leaf"] + 2 * j + 1 for j in range(m)],
                removed=[base + u["old_leaf"] + 2 * j for j in range(m)], arrived=[base_b + ub["block"][j] for j in range(m)],
                z0=lay["shrink"] + 1 if lay["s"] else None, old_root=upa[0], new_root=upa[-1], old_root_b=upb[0], new_root_b=upb[-1])


def _indicator_b_lay(lay):
    """the keys _trace_ann_head / _build_ann_head's indicator and select read, for blocks B_b and C_b"""
    return dict(lay, c=lay["b"], indicator=lay["indicator_b"], select=lay["select_b"])


def _trace_indicators(t, lay, roots):
    """idx_to_indicator(lay.c, K) as select_from_idx unrolls it and select_by_indicator(roots, indicators) on a _CellTrace
    -> (inds, picked)"""
    c = lay["c"]
    inds = [t.is_zero(lay["indicator"], c)]
    for j in range(1, len(roots)):
        at = _indicator_at(lay, j)
        t.put(at, [None, ("k", j), ("k", 1), ("c", c)], [1, 0, 0, 0])      # is_equal(c, Constant(j)) = sub [d, j, 1, c] + is_zero(d)
        inds.append(t.is_zero(at + 4, at))
    cells, gates = [("k", 0)], [1]
    for j in range(len(roots)):
        cells += [("c", roots[j]), ("c", inds[j]), None]
        gates += [0, 0, j + 1 < len(roots)]
    return inds, t.put(lay["select"], cells, gates) - 1


def trace_ann_move(K, m, depth_a, shrink, depth_b, grow, fetch_flags, fetch_values):
    """The closure of m moves from cluster a to cluster b of a committed index cell by cell (the ground truth of build_ann_move): the
    header, B_a, C_a, D, the delete's blocks E' and S on a's tree, F_a mid_j = select(a's new root, cluster_root_j, ind_a_j), B_b, C_b
    over mid, E_b m carried appends on b's grown tree, F_b out_j = select(b's new root, mid_j, ind_b_j), G.  Ties: picked_a to E''s old
    root, picked_b to E_b's, the carried leaf of E_b's update j to the removed leaf of E''s update 2 j.
    -> (CopyMap, public cells, dict(indicators, indicators_b, picked, picked_b, mids, outs, index_root_old, index_root_new, s0,
    shrink_top, layout and _move_info's keys))"""
    lay = ann_move_layout(K, m, depth_a, shrink, depth_b, grow)
    t = _CellTrace(lay["total"], fetch_flags, fetch_values)
    roots = [lay["roots"] + j for j in range(K)]
    inds, picked = _trace_indicators(t, lay, roots)
    root_old, at = t.leaf(lay["sponge_old"], lay["sponge"], None, [lay["centroids_root"]] + roots)
    assert at == lay["update"]
    upa = _trace_update_block(t, lay["update_layout"], lay["update"])
    t.copy_of[upa[0]] = picked                               # ctx.constrain_equal(picked_a, E''s old root)
    info = _move_info(lay, m, upa, [None, None])
    for x, y in zip(info["carried"], info["moved_old"]):
        t.copy_of[x] = y                                     # the delete's move: what left the last slot is what arrived in slot_j
    s0, top, new_root = None, None, upa[-1]
    if shrink:
        s0 = top = lay["shrink"]                             # S_0 = ctx.load_witness, Z_0 = ctx.load_constant(0)
        at = t.put(s0 + 1, [("k", 0)], [0])
        z = [s0 + 1]
        for l in range(depth_a - 1):
            z.append(t.node(at, z[l], z[l]))
            at += lay["update_layout"]["node_cells"]
        for i in range(shrink):
            top = t.node(at, top, z[depth_a - shrink + i])
            at += lay["update_layout"]["node_cells"]
        assert at == lay["mid"]
        t.copy_of[top] = upa[-1]                             # ctx.constrain_equal(S_s, E''s final root)
        new_root = s0
    mids = [t.select(lay["mid"] + 8 * j, new_root, roots[j], inds[j]) for j in range(K)]
    inds_b, picked_b = _trace_indicators(t, _indicator_b_lay(lay), mids)
    upb = _trace_update_block(t, lay["update_b_layout"], lay["update_b"])
    t.copy_of[upb[0]] = picked_b                             # ctx.constrain_equal(picked_b, E_b's old root)
    info = _move_info(lay, m, upa, upb)
    for x, y in zip(info["arrived"], info["removed"]):
        t.copy_of[x] = y                                     # THE MOVE: what arrived in b is what left a
    outs = [t.select(lay["new_roots"] + 8 * j, upb[-1], mids[j], inds_b[j]) for j in range(K)]
    root_new, at = t.leaf(lay["sponge_new"], lay["sponge"], None, [lay["centroids_root"]] + outs)
    assert at == lay["total"]
    info = dict(info, indicators=inds, indicators_b=inds_b, picked=picked, picked_b=picked_b, mids=mids, outs=outs, index_root_old=root_old,
                index_root_new=root_new, s0=s0, shrink_top=top, layout=lay)
    return t.finish(), ann_move_instances(root_old, lay["a"], lay["b"], upa, upb, root_new), info


def _build_indicators(B, lay, roots):
    """_trace_indicators from unit blocks on builder B (the blocks _build_ann_head places) -> (inds, picked)"""
    K, c = len(roots), lay["c"]
    s = Sym(0, 0)
    iz = Block(s, [s.g_is_zero(ext(0))])
    inds = [int(B.place(iz, [lay["indicator"]], [0], [[c]])[0, 0])]
    if K > 1:
        s = Sym(0, 0)
        d = s.push(None, True)                               # is_equal(c, Constant(j)) = sub [d, j, 1, c] + is_zero(d)
        s.push(None); s.push(C(1)); s.push(ext(0))
        ie = Block(s, [s.g_is_zero(d)])
        at = np.asarray([_indicator_at(lay, j) for j in range(1, K)], dtype=np.int64)
        inds += [int(x) for x in B.place(ie, at, np.zeros(K - 1, dtype=np.int64), np.full((K - 1, 1), c, dtype=np.int64))[:, 0]]
        for j in range(1, K):
            B.constant_cell(int(at[j - 1]) + 1, j)
    inds = np.asarray(inds, dtype=np.int64)
    s = Sym(0, 0)
    sb = Block(s, [s.g_select_by_indicator([ext(i) for i in range(K)], [ext(K + i) for i in range(K)])])
    return inds, int(B.place(sb, [lay["select"]], [0], np.concatenate([np.asarray(roots, dtype=np.int64), inds])[None, :])[0, 0])


def _build_selects(B, at, new_root, olds, inds):
    """out_j = select(new_root, olds_j, inds_j) at at + 8 j, placed at once -> the out cells"""
    K = len(inds)
    s = Sym(0, 0)
    sl = Block(s, [s.g_select(ext(0), ext(1), ext(2))])
    return B.place(sl, at + 8 * np.arange(K, dtype=np.int64), np.zeros(K, dtype=np.int64),
                   np.stack([np.full(K, new_root, dtype=np.int64), np.asarray(olds, dtype=np.int64), np.asarray(inds, dtype=np.int64)], axis=1))[:, 0]


def build_ann_move(K, m, depth_a, shrink, depth_b, grow, fetch_flags, fetch_values, builder=None):
    """trace_ann_move's map assembled from unit blocks, as build_ann_delete: the two update blocks are place_merkle_update at their bases
    with the carried kind, block S's hashes are placed one after the other (`builder`: as build_kmeans).  -> as trace_ann_move"""
    lay = ann_move_layout(K, m, depth_a, shrink, depth_b, grow)
    if np.asarray(fetch_flags(0, lay["n_in"])).any():
        raise ValueError("the assigned header carries no gate or constant flag")
    B = (builder or _Builder)(lay["total"], 0)
    roots = lay["roots"] + np.arange(K, dtype=np.int64)
    inds, picked = _build_indicators(B, lay, roots)
    root_old, end = place_sponge(B, lay["sponge_old"], [lay["centroids_root"]] + [int(r) for r in roots], fetch_flags, fetch_values)
    assert end == lay["update"]
    upa = place_merkle_update(B, 2 * m, 1, depth_a, fetch_flags, fetch_values, lay["update"], [2, 1] * m, 0, carried=True)
    B.tie(upa[0], picked)                                    # ctx.constrain_equal(picked_a, E''s old root)
    info = _move_info(lay, m, upa, [None, None])
    for x, y in zip(info["carried"], info["moved_old"]):
        B.tie(x, y)                                          # the delete's move
    s0, top, new_root = None, None, upa[-1]
    if shrink:
        one = lambda x: np.asarray([x], dtype=np.int64)
        perm = _perm_placer(B, fetch_flags, fetch_values)
        s0 = lay["shrink"]
        B.constant_cell(s0 + 1, 0)                           # Z_0 = ctx.load_constant(0)
        z, top, at = [one(s0 + 1)], one(s0), s0 + 2
        for l in range(depth_a - 1):
            z.append(_node(perm, one(at), z[l], z[l]))
            at += lay["update_layout"]["node_cells"]
        for i in range(shrink):
            top = _node(perm, one(at), top, z[depth_a - shrink + i])
            at += lay["update_layout"]["node_cells"]
        assert at == lay["mid"]
        top = int(top[0])
        B.tie(top, upa[-1])                                  # ctx.constrain_equal(S_s, E''s final root)
        new_root = s0
    mids = _build_selects(B, lay["mid"], new_root, roots, inds)
    inds_b, picked_b = _build_indicators(B, _indicator_b_lay(lay), mids)
    upb = place_merkle_update(B, m, 1, depth_b, fetch_flags, fetch_values, lay["update_b"], [2] * m, grow, carried=True)
    B.tie(int(upb[0]), picked_b)                             # ctx.constrain_equal(picked_b, E_b's old root)
    info = _move_info(lay, m, upa, upb)
    for x, y in zip(info["arrived"], info["removed"]):
        B.tie(x, y)                                          # THE MOVE: what arrived in b is what left a
    outs = _build_selects(B, lay["new_roots"], upb[-1], mids, inds_b)
    root_new, end = place_sponge(B, lay["sponge_new"], [lay["centroids_root"]] + [int(o) for o in outs], fetch_flags, fetch_values)
    if end != lay["total"]:
        raise ValueError("the trace does not end where the circuit does")
    info = dict(info, indicators=[int(i) for i in inds], indicators_b=[int(i) for i in inds_b], picked=picked, picked_b=picked_b,
                mids=[int(x) for x in mids], outs=[int(o) for o in outs], index_root_old=root_old, index_root_new=root_new, s0=s0, shrink_top=top,
                layout=lay)
    return B.finish(), ann_move_instances(root_old, lay["a"], lay["b"], upa, upb, root_new), info


# ---------------------------------------------------------------------------------------------------------------------------
# The cluster frame of the routing audit and the mean audit below, one circuit around a block of their own: A - D the frame's head, I
# [centroids | members] assigned, the own block, MC and MM the two merkle_commitments; public [index_root | c]
def _ann_cluster_layout(K, n_c, dim):
    """the head's keys of _ann_frame_layout (c, centroids_root, roots, n_in, indicator, select, sponge_old, sponge; `update`: where the head
    ends) and centroids, members: the assigned block I, the own block behind it; zero_c: the centroids' padding loads the zero cell"""
    head = _ann_frame_layout(K, merkle_leaf_layout(K + 1), 0)
    lay = {k: head[k] for k in ("c", "centroids_root", "roots", "n_in", "indicator", "sponge", "select", "sponge_old", "update")}
    lay.update(zero_c=(1 << (K - 1).bit_length()) > K, centroids=lay["update"], members=lay["update"] + K * dim)
    return lay


def _ann_cluster_close(lay, K, n_c, dim, own_end):
    """the two trees behind the audit's own block, which ends at `own_end`: merkle_c, merkle_m, total"""
    lay["merkle_c"] = own_end
    lay["merkle_m"] = lay["merkle_c"] + merkle_cells(K, dim)
    lay["total"] = lay["merkle_m"] + merkle_cells(n_c, dim, lay["zero_c"])
    return lay


def ann_audit_instances(index_root, c):
    """the public cells in make_public order: [index_root | c]"""
    return [int(index_root), int(c)]


ann_mean_instances = ann_audit_instances


def _build_ann_cluster(lay, K, n_c, dim, fetch_flags, fetch_values, builder, place_own):
    """The circuit of `lay` (an audit's layout over _ann_cluster_layout) in one map: the frame's head (_build_ann_head: the header
    [c | centroids_root | cluster roots], idx_to_indicator(c, K), select_by_indicator(cluster roots, ind) -> picked, the sponge ->
    index_root), [centroids | members] assigned, place_own(B, members (n_c, dim), centroids (K, dim), indicators) -> (pairs, its info
    keys): the audit's own block, tied as B.tie(a, b) for every pair; merkle_commitment(centroids), tied to the header's centroids_root,
    and merkle_commitment(members), tied to picked.  -> (CopyMap, public cells [index_root, c], dict(indicators, picked, the own keys,
    centroids_root, members_root, index_root, layout))"""
    B, inds, picked, index_root = _build_ann_head(lay, fetch_flags, fetch_values, builder)
    if np.asarray(fetch_flags(lay["centroids"], lay["members"] + n_c * dim)).any():
        raise ValueError("the assigned centroids and members carry no gate or constant flag")
    cent = lay["centroids"] + np.arange(K * dim, dtype=np.int64).reshape(K, dim)
    mem = lay["members"] + np.arange(n_c * dim, dtype=np.int64).reshape(n_c, dim)
    pairs, own_info = place_own(B, mem, cent, inds)
    for a, b in pairs:
        B.tie(a, b)
    croot, end = place_merkle(B, K, dim, lay["merkle_c"], lay["centroids"], fetch_flags, fetch_values)
    assert end == lay["merkle_m"]
    B.tie(croot, lay["centroids_root"])                      # ctx.constrain_equal(centroids_root, croot)
    zero = lay["merkle_c"] + K * merkle_leaf_layout(dim)["leaf_cells"] if lay["zero_c"] else None
    mroot, end = place_merkle(B, n_c, dim, lay["merkle_m"], lay["members"], fetch_flags, fetch_values, zero_cell=zero)
    if end != lay["total"]:
        raise ValueError("the trace does not end where the circuit does")
    B.tie(mroot, picked)                                     # ctx.constrain_equal(picked, mroot)
    info = dict(indicators=[int(i) for i in inds], picked=picked, **own_info, centroids_root=croot, members_root=mroot, index_root=index_root, layout=lay)
    return B.finish(), ann_audit_instances(index_root, lay["c"]), info


# ---------------------------------------------------------------------------------------------------------------------------
# The audit of one cluster's routing (include/vdb.h vdb_wit_ann_audit; pipeline.AnnAuditHotPath)
def ann_audit_layout(metric, K, n_c, dim, P, L):
    """where the blocks of the audit circuit start: _ann_cluster_layout's keys; routed: block R, per_member / per_member_l: cells and
    lookup cells of one member's sub-block, chain_off, pick_off: where its qmin chain and its select_by_indicator start; merkle_c,
    merkle_m; total, total_l; units: nearest_units over the K centroids"""
    if n_c < 1 or dim < 1:
        raise ValueError("at least one member and one word")
    lay = _ann_cluster_layout(K, n_c, dim)
    u = lay["units"] = nearest_units(metric, K, dim, 1, P, L)
    lay["routed"] = lay["members"] + n_c * dim
    lay["chain_off"] = K * u["db"].n
    lay["pick_off"] = lay["chain_off"] + (K - 1) * u["qm"].n
    lay["per_member"] = lay["pick_off"] + u["sb"].n
    lay["per_member_l"] = K * u["db"].n_lk + (K - 1) * u["qm"].n_lk
    lay["total_l"] = n_c * lay["per_member_l"]
    return _ann_cluster_close(lay, K, n_c, dim, lay["routed"] + n_c * lay["per_member"])


def place_routed(B, u, members, centroids, ind, base, lbase):
    """The routed block placed into builder `B` from the unit blocks of `u` = nearest_units over the K centroids: per member i, at
    base + i per_member, the K distance(centroid_j, member_i) (the centroid in the vector role, as nearest_vector has it), the K - 1 qmin
    of the chain and select_by_indicator(d_i0 .., `ind`); member i's lookup cells from lbase + i per_member_l on.  `members` (n_c, dim) /
    `centroids` (K, dim) / `ind` (K,): stream cells.  -> (own (n_c,), m (n_c,)): the selection's outputs and the chains' minima (d_i0 at
    K = 1); the caller ties them."""
    K, dim = u["n"], u["dim"]
    db, qm, sb = u["db"], u["qm"], u["sb"]
    members, centroids = np.asarray(members, dtype=np.int64).reshape(-1, dim), np.asarray(centroids, dtype=np.int64).reshape(K, dim)
    ind = np.asarray(ind, dtype=np.int64).reshape(K)
    n_c = members.shape[0]
    chain_off, chain_loff = K * db.n, K * db.n_lk
    pick_off = chain_off + (K - 1) * qm.n
    per, per_l = pick_off + sb.n, chain_loff + (K - 1) * qm.n_lk
    ii, jj = np.repeat(np.arange(n_c, dtype=np.int64), K), np.tile(np.arange(K, dtype=np.int64), n_c)
    d = B.place(db, base + ii * per + jj * db.n, lbase + ii * per_l + jj * db.n_lk, np.concatenate([centroids[jj], members[ii]], axis=1))[:, 0].reshape(n_c, K)
    acc = np.empty((n_c, K), dtype=np.int64)
    acc[:, 0] = d[:, 0]
    if K > 1:
        il, l = np.repeat(np.arange(n_c, dtype=np.int64), K - 1), np.tile(np.arange(K - 1, dtype=np.int64), n_c)
        bases = base + il * per + chain_off + l * qm.n
        acc[:, 1:] = (bases + qm.outs[0]).reshape(n_c, K - 1)
        B.place(qm, bases, lbase + il * per_l + chain_loff + l * qm.n_lk, np.stack([acc[:, :-1].reshape(-1), d[:, 1:].reshape(-1)], axis=1))
    own = B.place(sb, base + np.arange(n_c, dtype=np.int64) * per + pick_off, np.zeros(n_c, dtype=np.int64),
                  np.concatenate([d, np.broadcast_to(ind[None, :], (n_c, K))], axis=1))[:, 0]
    return own, acc[:, K - 1].copy()


def build_ann_audit(metric, K, n_c, dim, P, L, fetch_flags, fetch_values, builder=None):
    """The audit of one cluster's routing in one circuit (pipeline.AnnAuditHotPath): the cluster frame (_build_ann_cluster) around the
    routed block (place_routed) with every own_i TIED to m_i — centroid c attains the minimum of member i's K distances.
    fetch_flags / fetch_values: as place_merkle; `builder`: as build_kmeans.
    -> (CopyMap, public cells [index_root, c], dict(indicators, picked, own, m, centroids_root, members_root, index_root, layout))"""
    lay = ann_audit_layout(metric, K, n_c, dim, P, L)

    def own_block(B, mem, cent, inds):
        own, m = (x.tolist() for x in place_routed(B, lay["units"], mem, cent, inds, lay["routed"], 0))
        return zip(own, m), dict(own=own, m=m)               # ctx.constrain_equal(m_i, own_i)
    return _build_ann_cluster(lay, K, n_c, dim, fetch_flags, fetch_values, builder, own_block)


# ---------------------------------------------------------------------------------------------------------------------------
# The mean audit of one cluster (include/vdb.h vdb_wit_ann_mean; pipeline.AnnMeanHotPath)
def mean_units(K, P, L):
    """the unit blocks of the mean audit: dict(sb: select_by_indicator over K cells, add: qadd, qd: qdiv)"""
    s = Sym(P, L)
    u = dict(sb=Block(s, [s.g_select_by_indicator([ext(k) for k in range(K)], [ext(K + k) for k in range(K)])]))
    s = Sym(P, L)
    u["add"] = Block(s, [s.g_add(ext(0), ext(1))])
    s = Sym(P, L)
    u["qd"] = Block(s, [s.qdiv(ext(0), ext(1))])
    return u


def ann_mean_layout(K, n_c, dim, P, L):
    """where the blocks of the mean audit circuit start: _ann_cluster_layout's keys; own: block S (dim select_by_indicator over K
    cells); len: the constant quantization(n_c), block M's first cell; chain: the qadd cells; div: the dim qdiv blocks; merkle_c,
    merkle_m; total, total_l; units: mean_units"""
    if n_c < 1 or dim < 1:
        raise ValueError("at least one member and one word")
    if n_c >= 1 << P:
        raise ValueError("quantization(n_c) must stay below qdiv's divisor bound 2^(2P)")
    lay = _ann_cluster_layout(K, n_c, dim)
    u = lay["units"] = mean_units(K, P, L)
    lay["own"] = lay["members"] + n_c * dim
    lay["len"] = lay["own"] + dim * u["sb"].n
    lay["chain"] = lay["len"] + 1
    lay["div"] = lay["chain"] + (n_c - 1) * dim * u["add"].n
    lay["total_l"] = dim * u["qd"].n_lk
    return _ann_cluster_close(lay, K, n_c, dim, lay["div"] + dim * u["qd"].n)


def place_mean(B, u, members, centroids, ind, n_c_quantized, own_base, len_cell, lbase):
    """Blocks S and M placed into builder `B` from the unit blocks of `u` = mean_units: per word j select_by_indicator(centroids[:, j],
    `ind`) at own_base + j sb.n; the constant `n_c_quantized` at `len_cell`; from len_cell + 1 on the qadd(member_i[j], running sum) of
    members i = 1 .. n_c - 1, member-major (kmeans' order and stride), then per word qdiv(sum_j, len), its lookup cells from lbase +
    j qd.n_lk on.  `members` (n_c, dim) / `centroids` (K, dim) / `ind` (K,): stream cells.  -> (own (dim,), mean (dim,)): the selection's
    outputs and the quotients; the caller ties them."""
    sb = u["sb"]
    members, centroids = np.asarray(members, dtype=np.int64), np.asarray(centroids, dtype=np.int64)
    (n_c, dim), K = members.shape, centroids.shape[0]
    ind = np.asarray(ind, dtype=np.int64).reshape(K)
    j = np.arange(dim, dtype=np.int64)
    own = B.place(sb, own_base + j * sb.n, np.zeros(dim, dtype=np.int64), np.concatenate([centroids.T, np.broadcast_to(ind[None, :], (dim, K))], axis=1))[:, 0]
    return own, place_mean_quotients(B, u, members, n_c_quantized, len_cell, lbase)


def place_mean_quotients(B, u, members, n_c_quantized, len_cell, lbase):
    """Block M alone (place_mean's second half; the recentre has no block S): the constant `n_c_quantized` at `len_cell`, the qadd chain
    from len_cell + 1 on, then per word qdiv(sum_j, len).  `u` needs add and qd.  -> mean (dim,): the quotients' cells"""
    add, qd = u["add"], u["qd"]
    members = np.asarray(members, dtype=np.int64)
    n_c, dim = members.shape
    j = np.arange(dim, dtype=np.int64)
    B.constant_cell(len_cell, n_c_quantized)                 # ctx.load_constant(quantization(n_c))
    chain = len_cell + 1
    sum_cells = members[0].copy()
    if n_c > 1:
        vv, jj = np.repeat(np.arange(1, n_c, dtype=np.int64), dim), np.tile(j, n_c - 1)
        bases = chain + (vv - 1) * add.n * dim + add.n * jj
        outs = bases + add.outs[0]
        prev = np.where(vv == 1, members[0][jj], outs - add.n * dim)
        B.place(add, bases, np.zeros_like(bases), np.stack([members[vv, jj], prev], axis=1))    # qadd(member's word, running sum)
        sum_cells = outs.reshape(n_c - 1, dim)[-1]
    div = chain + (n_c - 1) * dim * add.n
    return B.place(qd, div + j * qd.n, lbase + j * qd.n_lk, np.stack([sum_cells, np.full(dim, len_cell)], axis=1))[:, 0]


def build_ann_mean(K, n_c, dim, P, L, fetch_flags, fetch_values, builder=None):
    """The mean audit of one cluster in one circuit (pipeline.AnnMeanHotPath): the cluster frame (_build_ann_cluster) around blocks S and
    M (place_mean) with every quotient mean_j TIED to own_j — word j of centroid c is the mean of the members' words j.
    fetch_flags / fetch_values: as place_merkle; `builder`: as build_kmeans.
    -> (CopyMap, public cells [index_root, c], dict(indicators, picked, own, mean, len, centroids_root, members_root, index_root, layout))"""
    lay = ann_mean_layout(K, n_c, dim, P, L)

    def own_block(B, mem, cent, inds):
        own, mean = (x.tolist() for x in place_mean(B, lay["units"], mem, cent, inds, n_c << P, lay["own"], lay["len"], 0))
        return zip(mean, own), dict(own=own, mean=mean, len=lay["len"])    # ctx.constrain_equal(own_j, mean_j)
    return _build_ann_cluster(lay, K, n_c, dim, fetch_flags, fetch_values, builder, own_block)


# ---------------------------------------------------------------------------------------------------------------------------
# The recentre of one cluster, old index root to new (include/vdb.h vdb_wit_ann_recentre; pipeline.AnnRecentreHotPath)
def ann_recentre_layout(K, n_c, dim, P, L):
    """where the blocks of the recentre circuit start: the head's keys of _ann_frame_layout (c, centroids_root, roots, n_in, indicator,
    select, sponge_old, sponge; `update`: where the head ends); members: the assigned block I; len, chain, div: block M as
    ann_mean_layout has it; merkle_m: MM; centroid_update: block U, update_layout: its merkle_update_layout (relative to it), depth;
    sponge_new: G; total, total_l; units: dict(add, qd)"""
    if n_c < 1 or dim < 1:
        raise ValueError("at least one member and one word")
    if n_c >= 1 << P:
        raise ValueError("quantization(n_c) must stay below qdiv's divisor bound 2^(2P)")
    if K == 1:
        raise ValueError("a tree of one leaf has no path (depth 0)")
    sp = merkle_leaf_layout(K + 1)
    head = _ann_frame_layout(K, sp, 0)
    lay = {k: head[k] for k in ("c", "centroids_root", "roots", "n_in", "indicator", "sponge", "select", "sponge_old", "update")}
    mu = mean_units(1, P, L)
    u = lay["units"] = dict(add=mu["add"], qd=mu["qd"])
    depth = (K - 1).bit_length()
    upd = merkle_update_layout(1, dim, depth)
    lay.update(members=lay["update"], depth=depth, update_layout=upd)
    lay["len"] = lay["members"] + n_c * dim
    lay["chain"] = lay["len"] + 1
    lay["div"] = lay["chain"] + (n_c - 1) * dim * u["add"].n
    lay["merkle_m"] = lay["div"] + dim * u["qd"].n
    lay["centroid_update"] = lay["merkle_m"] + merkle_cells(n_c, dim)
    lay["sponge_new"] = lay["centroid_update"] + upd["total"]
    lay["total"] = lay["sponge_new"] + sp["leaf_cells"]
    lay["total_l"] = dim * u["qd"].n_lk
    return lay


def ann_recentre_instances(index_root_old, c, index_root_new):
    """the public cells in make_public order: [index_root_old | c | index_root_new]"""
    return [int(index_root_old), int(c), int(index_root_new)]


def build_ann_recentre(K, n_c, dim, P, L, fetch_flags, fetch_values, builder=None):
    """The recentre of one cluster in one circuit (pipeline.AnnRecentreHotPath), from the pieces the other circuits have: the frame's head
    (_build_ann_head), the members assigned, block M (place_mean_quotients), merkle_commitment(members) TIED to picked (place_merkle),
    the update block of the centroids' tree with one write (place_merkle_update at its base) — its old root TIED to the header's
    centroids_root, its idx to c, its assigned new-vector word j to mean_j — and the sponge over [the block's new root | the header's
    cluster roots] (place_sponge).  fetch_flags / fetch_values: as place_merkle; `builder`: as build_kmeans.
    -> (CopyMap, public cells [index_root_old, c, index_root_new], dict(indicators, picked, mean, len, members_root, update_public,
    new_vector, index_root_old, index_root_new, layout))"""
    lay = ann_recentre_layout(K, n_c, dim, P, L)
    B, inds, picked, root_old = _build_ann_head(lay, fetch_flags, fetch_values, builder)
    if np.asarray(fetch_flags(lay["members"], lay["members"] + n_c * dim)).any():
        raise ValueError("the assigned members carry no gate or constant flag")
    mem = lay["members"] + np.arange(n_c * dim, dtype=np.int64).reshape(n_c, dim)
    mean = [int(x) for x in place_mean_quotients(B, lay["units"], mem, n_c << P, lay["len"], 0)]
    mroot, end = place_merkle(B, n_c, dim, lay["merkle_m"], lay["members"], fetch_flags, fetch_values)
    assert end == lay["centroid_update"]
    B.tie(mroot, picked)                                     # ctx.constrain_equal(picked, mroot)
    ub = lay["centroid_update"]
    upub = place_merkle_update(B, 1, dim, lay["depth"], fetch_flags, fetch_values, ub)
    new_vector = [ub + j for j in range(dim)]
    for j in range(dim):
        B.tie(new_vector[j], mean[j])                        # ctx.constrain_equal(mean_j, the block's new-vector word j)
    B.tie(upub[0], lay["centroids_root"])                    # ctx.constrain_equal(centroids_root, the block's old root)
    B.tie(upub[1], lay["c"])                                 # ctx.constrain_equal(c, the block's idx)
    root_new, end = place_sponge(B, lay["sponge_new"], [upub[-1]] + [lay["roots"] + j for j in range(K)], fetch_flags, fetch_values)
    if end != lay["total"]:
        raise ValueError("the trace does not end where the circuit does")
    info = dict(indicators=[int(i) for i in inds], picked=picked, mean=mean, len=lay["len"], members_root=mroot, update_public=upub, new_vector=new_vector,
                index_root_old=root_old, index_root_new=root_new, layout=lay)
    return B.finish(), ann_recentre_instances(root_old, lay["c"], root_new), info


# ---------------------------------------------------------------------------------------------------------------------------
# The cover of the database by the index (include/vdb.h vdb_wit_ann_cover; pipeline.AnnCoverHotPath)
def place_tree(perm, digest, pos, node_cells):
    """the nodes of a tree over the digest cells `digest` (a power of two of them: the padding already filled in) placed from stream
    cell `pos` on, level-major (place_merkle's loop; perm: _perm_placer's) -> (the root's cell: the digest itself where there is one
    leaf, the first cell after the nodes)"""
    digest = np.asarray(digest, dtype=np.int64)
    while digest.size > 1:
        bases = pos + np.arange(digest.size // 2, dtype=np.int64) * node_cells
        digest = _node(perm, bases, digest[0::2], digest[1::2])
        pos += bases.size * node_cells
    return int(digest[0]), pos


def ann_cover_layout(sizes):
    """where the blocks of the cover circuit start, for the K cluster sizes `sizes`: dict(K, n, lp, sizes, lps: the clusters' padded leaf
    counts, header (0), a, b: the assigned digests, n_in, zero: the load_zero cell or None, tree_d, tree_c: the K + 1 trees' nodes,
    tree_c_at: where cluster c's nodes start, sponge: D, gamma: G, sub_a, mul_a, sub_b, mul_b, total, total_l = 0, node_cells)"""
    sizes = [int(x) for x in sizes]
    K, n = len(sizes), sum(sizes)
    if K < 1 or min(sizes) < 1:
        raise ValueError("at least one cluster, and no empty one")
    sp = merkle_leaf_layout(K + 1)
    node = sp["node_cells"]
    lp, lps = 1 << (n - 1).bit_length(), [1 << (x - 1).bit_length() for x in sizes]
    lay = dict(K=K, n=n, lp=lp, sizes=sizes, lps=lps, header=0, a=K + 1, b=K + 1 + n, n_in=K + 1 + 2 * n, node_cells=node, total_l=0)
    padded = lp > n or any(l > x for l, x in zip(lps, sizes))
    lay["zero"] = lay["n_in"] if padded else None
    lay["tree_d"] = lay["n_in"] + (1 if padded else 0)
    lay["tree_c"] = lay["tree_d"] + (lp - 1) * node
    at, lay["tree_c_at"] = lay["tree_c"], []
    for l in lps:
        lay["tree_c_at"].append(at)
        at += (l - 1) * node
    lay["sponge"] = at
    lay["gamma"] = at + sp["leaf_cells"]
    lay["sub_a"] = lay["gamma"] + node
    lay["mul_a"] = lay["sub_a"] + 4 * n
    lay["sub_b"] = lay["mul_a"] + 4 * (n - 1)
    lay["mul_b"] = lay["sub_b"] + 4 * n
    lay["total"] = lay["mul_b"] + 4 * (n - 1)
    return lay


def ann_cover_instances(database_root, index_root):
    """the public cells in make_public order: [database_root | index_root]"""
    return [int(database_root), int(index_root)]


def build_ann_cover(sizes, fetch_flags, fetch_values, builder=None):
    """The cover of the database by the index in one circuit (pipeline.AnnCoverHotPath): the header [centroids_root | cluster roots] and
    the 2 n leaf digests assigned, the zero cell, the database tree over a and the K cluster trees over their stretches of b (place_tree;
    root_c TIED to the header's cluster_root_c), the sponge over the header (index_root), the sponge over [droot, index_root] (gamma),
    then per side g_sub(gamma, x_i) and the g_mul chain; the last accumulator of b TIED to the last of a.  fetch_flags / fetch_values:
    as place_merkle; `builder`: as build_kmeans.
    -> (CopyMap, public cells [database_root, index_root], dict(roots: the K root cells, gamma, last_a, last_b, layout))"""
    lay = ann_cover_layout(sizes)
    K, n, node = lay["K"], lay["n"], lay["node_cells"]
    if np.asarray(fetch_flags(0, lay["n_in"])).any():
        raise ValueError("the assigned header and digests carry no gate or constant flag")
    B = (builder or _Builder)(lay["total"], 0)
    if lay["zero"] is not None:
        B.constant_cell(lay["zero"], 0)                      # ctx.load_zero(), once: every tree's padding copies it
    perm = _perm_placer(B, fetch_flags, fetch_values)

    def padded(first, count, lp):
        d = np.full(lp, lay["zero"] if lay["zero"] is not None else -1, dtype=np.int64)
        d[:count] = first + np.arange(count, dtype=np.int64)
        return d

    droot, at = place_tree(perm, padded(lay["a"], n, lay["lp"]), lay["tree_d"], node)
    assert at == lay["tree_c"]
    roots, off = [], 0
    for c in range(K):
        assert at == lay["tree_c_at"][c]
        root, at = place_tree(perm, padded(lay["b"] + off, lay["sizes"][c], lay["lps"][c]), at, node)
        B.tie(root, lay["header"] + 1 + c)                   # ctx.constrain_equal(cluster_root_c, root_c)
        roots.append(root)
        off += lay["sizes"][c]
    assert at == lay["sponge"]
    iroot, at = place_sponge(B, lay["sponge"], [lay["header"] + j for j in range(K + 1)], fetch_flags, fetch_values)
    assert at == lay["gamma"]
    gamma, at = place_sponge(B, lay["gamma"], [droot, iroot], fetch_flags, fetch_values)
    assert at == lay["sub_a"]
    s = Sym(0, 0)
    sub = Block(s, [s.g_sub(ext(0), ext(1))])
    s = Sym(0, 0)
    mul = Block(s, [s.g_mul(ext(0), ext(1))])
    i, last = np.arange(n, dtype=np.int64), []
    for x, sb, mb in ((lay["a"], lay["sub_a"], lay["mul_a"]), (lay["b"], lay["sub_b"], lay["mul_b"])):
        t = B.place(sub, sb + 4 * i, np.zeros(n, dtype=np.int64), np.stack([np.full(n, gamma, dtype=np.int64), x + i], axis=1))[:, 0]
        if n > 1:
            bases = mb + 4 * i[:-1]
            outs = bases + int(mul.outs[0])
            acc = np.concatenate([t[:1], outs[:-1]])         # acc_0 = t_0; acc_i = the product before it
            B.place(mul, bases, np.zeros(n - 1, dtype=np.int64), np.stack([acc, t[1:]], axis=1))
            last.append(int(outs[-1]))
        else:
            last.append(int(t[0]))
    B.tie(last[1], last[0])                                  # ctx.constrain_equal(prod_a, prod_b)
    if lay["mul_b"] + 4 * (n - 1) != lay["total"]:
        raise ValueError("the trace does not end where the circuit does")
    info = dict(roots=roots, gamma=gamma, droot=droot, index_root=iroot, last_a=last[0], last_b=last[1], layout=lay)
    return B.finish(), ann_cover_instances(droot, iroot), info


# ---------------------------------------------------------------------------------------------------------------------------
# Merkle openings (include/vdb.h vdb_wit_merkle_open; pipeline.ReadHotPath)
def merkle_open_layout(m, dim, depth, with_vectors):
    """where the cells of m openings lie: dict(nperm, n_ins, sizes, leaf_cells, node_cells, level_cells, ip_cells, per_read, n_lead,
    bits, sibs, n_in, total) — stream cells [vectors m * dim (vector mode) or leaves m (leaf mode) | bits | siblings], then read j's
    block at n_in + j * per_read: its leaf sponge (vector mode only), per level [assert_bit 4 | select lo 8 | select ro 8 | H], the
    index inner product"""
    if m < 1 or depth < 1 or dim < 1:
        raise ValueError("a call opens at least one slot of a tree with at least two leaves")
    lay = _path_layout(dim, depth, 1)
    if not with_vectors:
        lay.update(nperm=0, n_ins=[], sizes=[], leaf_cells=0)
    n_lead = m * dim if with_vectors else m
    lay.update(n_lead=n_lead, bits=n_lead, sibs=n_lead + m * depth, n_in=n_lead + 2 * m * depth)
    lay["per_read"] = lay["leaf_cells"] + depth * lay["level_cells"] + lay["ip_cells"]
    lay["total"] = lay["n_in"] + m * lay["per_read"]
    return lay


def merkle_open_instances(m, top0, idx, leaf, vector_cells=()):
    """the public cells in make_public order: the root (the top of read 0), per read (idx, leaf), then in vector mode the m vectors word
    by word"""
    out = [int(top0)]
    for j in range(m):
        out += [int(idx[j]), int(leaf[j])]
    return out + [int(c) for c in vector_cells]


def trace_merkle_open(m, dim, depth, with_vectors, fetch_flags, fetch_values):
    """The closure of m openings cell by cell (the ground truth of build_merkle_open): assign the three witness groups, then per read the
    leaf sponge (vector mode), the levels and the index, the top of every read after the first tied to the top of read 0.
    fetch_flags / fetch_values: as trace_merkle_update.  -> (CopyMap, public cells)"""
    lay = merkle_open_layout(m, dim, depth, with_vectors)
    t = _CellTrace(lay["total"], fetch_flags, fetch_values)
    idx_cells, leaves, top0 = [], [], None
    for j in range(m):
        at = lay["n_in"] + j * lay["per_read"]
        cur, at = t.leaf(at, lay, j * dim) if with_vectors else (j, at)      # the squeeze cell, or the assigned leaf
        leaves.append(cur)
        (cur,), idx_cell, at = t.path(at, [cur], range(lay["bits"] + j * depth, lay["bits"] + (j + 1) * depth),
                                      range(lay["sibs"] + j * depth, lay["sibs"] + (j + 1) * depth))
        idx_cells.append(idx_cell)
        assert at == lay["n_in"] + (j + 1) * lay["per_read"]
        if top0 is None:
            top0 = cur
        else:
            t.copy_of[cur] = top0                            # ctx.constrain_equal(cur, root)
    return t.finish(), merkle_open_instances(m, top0, idx_cells, leaves, range(m * dim) if with_vectors else ())


def build_merkle_open(m, dim, depth, with_vectors, fetch_flags, fetch_values, builder=None):
    """trace_merkle_open's map assembled from unit blocks — one per kind of permutation, the bit with its two selects, the index inner
    product — each placed for all m reads at once, level after level (`builder`: as build_kmeans).  -> (CopyMap, public cells)"""
    lay = merkle_open_layout(m, dim, depth, with_vectors)
    B = (builder or _Builder)(lay["total"], 0)
    j = np.arange(m, dtype=np.int64)
    base = lay["n_in"] + j * lay["per_read"]
    perm = _perm_placer(B, fetch_flags, fetch_values)
    leaf = _place_leaf_sponge(perm, base, lay, [j * dim + k for k in range(dim)])[0] if with_vectors else j
    path = j[:, None] * depth + np.arange(depth, dtype=np.int64)[None, :]
    (cur,), idx = _place_path(B, perm, lay, base + lay["leaf_cells"], lay["bits"] + path, lay["sibs"] + path, [leaf])
    for k in range(1, m):
        B.tie(int(cur[k]), int(cur[0]))                      # ctx.constrain_equal(cur, root)
    return B.finish(), merkle_open_instances(m, cur[0], idx, leaf, range(m * dim) if with_vectors else ())
