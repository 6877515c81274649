"""Python-integer model of the nine-limb lazy field arithmetic (halo2_vectordb_amd/csrc/limb9.hpp, the product cores of field.hpp, the
MSM accumulator of ec_l9.hpp) and the case generator shared by tests/test_l9_cpu.py and tests/test_gpu_l9.py.

Everything here is written from the definitions: a limb array stands for the integer sum l_k 2^(29 k), a product core returns
(T + m p) / 2^261 for the one m < 2^261 that makes the division exact, a subtraction adds an offset K p limb by limb.  No tolerance
anywhere: the probe (tools/l9_probe.hip) must return these integers bit for bit.

A case is (tag, input words); `expect(op, mod, tag, words)` first asserts the documented preconditions of the op on the inputs (so a
generator bug cannot move cases into the comfortable middle), computes the exact result, asserts the op's contract on it, and returns
the output words.  Tags starting with "ood:" mark operands outside the domain (host mode only: an overflow is just a wrong number
there); for those the model returns what 32-bit arithmetic gives and asserts that it is NOT the integer result."""
import os
import random
import shutil
import struct
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

R = 0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001
Q = 0x30644E72E131A029B85045B68181585D97816A916871CA8D3C208C16D87CFD47
P = (R, Q)
B29 = 1 << 29
M29 = B29 - 1
U32 = 1 << 32
T261 = 1 << 261
LIM61 = (61 * B29) // 10          # floor(6.1 * 2^29): the largest first-operand limb of a product (field.hpp)
MAGIC = 0x4C395042
CHAIN = 64

(MUL, MUL2, SQR, SHOUP, FROM_MONT, MONT_MUL, SPLIT, SPLIT32, PACK, RENORM, CARRY, ADD, SUB, NEG, CANON, IS_ZERO, CANON_WIDE, OFFSET,
 SHOUP_PAIR, MADD, MDBL, GATE, MADD_CHAIN) = range(23)
NAMES = ["mont_core29", "mont_core29_2", "mont_sqr_core29", "shoup_core29", "from_mont", "mont_mul", "l9_split", "l9_split32", "l9_pack",
         "l9_renorm", "l9_carry", "l9_add", "l9_sub", "l9_neg", "l9_canon", "l9_is_zero_mod", "l9_canon_wide", "l9_offset_limbs",
         "shoup_pair29", "madd_l9", "mdbl_l9", "gate_step", "madd_l9_chain"]
NIN = [18, 36, 9, 27, 8, 16, 8, 8, 9, 9, 9, 18, 27, 18, 9, 9, 9, 1, 8, 54, 18, 67, 37 + CHAIN * 17]
NOUT = [9, 9, 9, 9, 8, 8, 9, 9, 8, 9, 9, 9, 9, 9, 8, 1, 8, 11, 18, 37, 37, 17, CHAIN * 37]
DEVICE_ONLY = {CANON_WIDE, MADD, MDBL, MADD_CHAIN}
HOST_ONLY = {OFFSET, SHOUP_PAIR}
OFFSETS_IN_USE = {0: (2, 9, 14, 34), 1: (2, 8)}


# ---- integers <-> limbs -------------------------------------------------------------------------------------------------------------
def val(l):
    assert len(l) == 9
    return sum(x << (29 * k) for k, x in enumerate(l))


def norm(v):
    """the exactly normalised limbs of v (the top limb keeps all remaining bits)"""
    l = [(v >> (29 * k)) & M29 for k in range(8)] + [v >> 232]
    assert l[8] < U32
    return l


def words8(v):
    assert 0 <= v < 1 << 256
    return [(v >> (32 * i)) & 0xFFFFFFFF for i in range(8)]


def from_words(w):
    return sum(x << (32 * i) for i, x in enumerate(w))


def is_norm(l):
    return all(x < B29 for x in l[:8])


def reps(v, lim):
    """several limb arrays of the same integer, every limb below `lim`: exactly normalised, and with one unit of 2^29 moved from limb
    k + 1 into limb k, for each k where that keeps limb k below `lim`, and for all such k at once (the shape a parallel carry pass
    leaves when lim = 2^29 + 8)"""
    n = norm(v)
    out = [n]
    alls = list(n)
    for k in range(8):
        if n[k + 1] >= 1 and n[k] + B29 < lim:
            m = list(n)
            m[k] += B29
            m[k + 1] -= 1
            out.append(m)
        if alls[k + 1] >= 1 and alls[k] + B29 < lim:
            alls[k] += B29
            alls[k + 1] -= 1
    if alls != n and alls not in out:
        out.append(alls)
    assert all(val(x) == v and max(x) < max(lim, n[8] + 1) for x in out)
    return out


def edge_values(p, bound, js=()):
    """0, 1, p - 1, p, p + 1, 2p - 1, 2p and j p + {0, 1, p - 1} for the given j, below `bound`"""
    s = [0, 1, p - 1, p, p + 1, 2 * p - 1, 2 * p]
    for j in js:
        s += [j * p, j * p + 1, j * p + p - 1]
    return sorted({v for v in s if v < bound})


# ---- the models ---------------------------------------------------------------------------------------------------------------------
def core(T, p):
    """(T + m p) / 2^261 with m = -T / p mod 2^261: what every Montgomery core returns for the integer T its columns add up to"""
    m = (-T * pow(p, -1, T261)) % T261
    out, rem = divmod(T + m * p, T261)
    assert rem == 0
    return out


def core_out(T, p):
    out = core(T, p)
    l = norm(out)
    # contract: limbs 0..7 below 2^29 (norm), the top limb fits its word, out < T / 2^261 + p
    assert out * T261 < T + p * T261 and (out * T261 - T) % p == 0
    return l


def shoup(V, W, WQ, p):
    """the issue's definition: q from the columns 7 .. 17 of WQ * V, t from the low nine columns of W V + q (2^261 - p)"""
    q = sum(WQ[i] * V[j] << (29 * (i + j - 7)) for i in range(9) for j in range(9) if i + j >= 7) >> 58
    v, w = val(V), val(W)
    out = (w * v + q * (T261 - p)) % T261
    return out, q, w * v // p - q


def offset_limbs(K, p):
    v = norm(K * p)
    c = [v[0] + B29] + [v[k] + B29 - 1 for k in range(1, 8)] + [v[8] - 1]
    assert val(c) == K * p
    return c


def sub_limbs(a, t, c):
    """(limbs as 32-bit arithmetic gives them, wrapped?): limb k is a_k + c_k - t_k when that lies in [0, 2^32) — the header's promise
    for ANY minuend a is t_k <= c_k"""
    exact = [a[k] + c[k] - t[k] for k in range(9)]
    wrapped = any(not 0 <= x < U32 for x in exact)
    return [x % U32 for x in exact], wrapped


# BN254 G1 over Python integers: y^2 = x^3 + 3, None is the identity
def ec_add(A, Bp):
    if A is None:
        return Bp
    if Bp is None:
        return A
    (x1, y1), (x2, y2) = A, Bp
    if x1 == x2:
        if (y1 + y2) % Q == 0:
            return None
        lam = 3 * x1 * x1 * pow(2 * y1, -1, Q) % Q
    else:
        lam = (y2 - y1) * pow(x2 - x1, -1, Q) % Q
    x3 = (lam * lam - x1 - x2) % Q
    return x3, (lam * (x1 - x3) - y1) % Q


def ec_neg(A):
    return None if A is None else (A[0], -A[1] % Q)


def ec_mul(k, A):
    acc = None
    while k:
        if k & 1:
            acc = ec_add(acc, A)
        A = ec_add(A, A)
        k >>= 1
    return acc


def ec_point(rng):
    while True:
        x = rng.randrange(Q)
        y2 = (x * x * x + 3) % Q
        y = pow(y2, (Q + 1) // 4, Q)
        if y * y % Q == y2:
            return x, (y if rng.random() < 0.5 else Q - y)


RP = T261 % Q       # coordinates inside the accumulator carry the factor 2^261
ACC_BOUNDS = (15 * Q // 2, 18 * Q // 5, 11 * Q // 10, 11 * Q // 10)   # x < 7.5 q, y < 3.6 q, zz, zzz < 1.1 q (AccL9)


def acc_affine(words):
    """(X, Y, ZZ, ZZZ limbs, ident) -> the affine point the accumulator stands for (X / ZZ, Y / ZZZ: the 2^261 factors cancel)"""
    if words[36]:
        return None
    X, Y, ZZ, ZZZ = (val(words[9 * i: 9 * i + 9]) for i in range(4))
    zz, zzz = ZZ * pow(RP, -1, Q) % Q, ZZZ * pow(RP, -1, Q) % Q
    assert zz and zzz and pow(zz, 3, Q) == pow(zzz, 2, Q)
    return X * pow(ZZ, -1, Q) % Q, Y * pow(ZZZ, -1, Q) % Q


def acc_check_bounds(words):
    """AccL9's stated invariant: exactly normalised, x < 7.5 q, y < 3.6 q, zz, zzz < 1.1 q (nothing is promised about an identity)"""
    if words[36]:
        return
    for i in range(4):
        l = words[9 * i: 9 * i + 9]
        assert is_norm(l) and val(l) < ACC_BOUNDS[i], (i, val(l) / Q)


def acc_words(pt, rng, js=(0, 0, 0, 0)):
    """an accumulator that stands for the affine point `pt`: random zz, coordinates x + j q"""
    if pt is None:
        return [0] * 36 + [1]
    z = rng.randrange(1, Q)
    zz, zzz = z * z % Q, z * z * z % Q
    cs = (pt[0] * zz * RP % Q, pt[1] * zzz * RP % Q, zz * RP % Q, zzz * RP % Q)
    w = []
    for c, j in zip(cs, js):
        w += norm(c + j * Q)
    return w + [0]


def point_words(pt, neg):
    return words8(pt[0] * RP % Q) + words8(pt[1] * RP % Q) + [1 if neg else 0]


def canon_wide_estimate(l):
    """the quotient estimate of l9_canon_wide as its comment defines it, and its error against the true quotient"""
    top = l[8] + (l[7] >> 29)
    qe = top // (0x30644E + 1)
    return qe, val(l) // R - qe


def expect(op, mod, tag, w):
    p = P[mod]
    ood = tag.startswith("ood:")
    if op == MUL:
        A, Bv = w[0:9], w[9:18]
        assert max(A) <= LIM61 and max(Bv) < B29
        return core_out(val(A) * val(Bv), p)
    if op == MUL2:
        A1, B1, A2, B2 = w[0:9], w[9:18], w[18:27], w[27:36]
        assert all(A1[k] + A2[k] < 6 * B29 for k in range(9)) and max(B1) < B29 and max(B2) < B29
        return core_out(val(A1) * val(B1) + val(A2) * val(B2), p)
    if op == SQR:
        assert max(w) < B29 + 8
        return core_out(val(w) ** 2, p)
    if op == SHOUP:
        V, W, WQ = w[0:9], w[9:18], w[18:27]
        assert max(V) <= LIM61 and val(V) < T261 and val(W) < p and is_norm(W) and is_norm(WQ) and val(WQ) == (val(W) << 261) // p
        out, q, err = shoup(V, W, WQ, p)
        assert out == val(W) * val(V) - q * p and out < 3 * p and err in (0, 1, 2), (tag, err)
        l = norm(out)
        assert l[8] < B29
        return l
    if op == FROM_MONT:
        a = from_words(w)
        assert a < p
        return words8(a * pow(2, -256, p) % p)
    if op == MONT_MUL:
        a, b = from_words(w[:8]), from_words(w[8:])
        assert a < p and b < p
        return words8(a * b * pow(2, -256, p) % p)
    if op == SPLIT:
        l = norm(from_words(w))
        assert l[8] < 1 << 24
        return l
    if op == SPLIT32:
        l = norm(32 * from_words(w))
        assert l[8] < B29
        return l
    if op == PACK:
        assert is_norm(w) and val(w) < 1 << 256
        return words8(val(w))
    if op == RENORM:
        # limbs below 2^32 in; the top limb needs room for the carry it takes (at most 7)
        assert max(w[:8]) < U32 and w[8] + 7 < U32
        out = [w[0] & M29] + [(w[k] & M29) + (w[k - 1] >> 29) for k in range(1, 8)] + [w[8] + (w[7] >> 29)]
        assert val(out) == val(w) and max(out[:8]) < B29 + 8
        return out
    if op == CARRY:
        # every limb must have room for the carry of the one below (at most 7 when limbs stay below 2^32 - 7)
        assert max(w) + 7 < U32
        out = norm(val(w))
        return out
    if op == ADD:
        a, b = w[:9], w[9:]
        out = [a[k] + b[k] for k in range(9)]
        assert max(out) < U32 and val(out) == val(a) + val(b)
        return out
    if op == SUB:
        a, t, c = w[0:9], w[9:18], w[18:27]
        out, wrapped = sub_limbs(a, t, c)
        assert wrapped == ood, tag
        assert (val(out) == val(a) - val(t) + val(c)) == (not ood)
        return out
    if op == NEG:
        t, c = w[0:9], w[9:18]
        out, wrapped = sub_limbs([0] * 9, t, c)
        assert wrapped == ood, tag
        assert (val(out) == val(c) - val(t)) == (not ood)
        return out
    if op == CANON:
        assert is_norm(w) and val(w) < 2 * p
        return words8(val(w) % p)
    if op == IS_ZERO:
        assert is_norm(w) and val(w) < 2 * p
        return [1 if val(w) in (0, p) else 0]
    if op == CANON_WIDE:
        assert mod == 0 and max(w) < U32 and val(w) < 1 << 259
        qe, err = canon_wide_estimate(w)
        assert 0 <= err <= 3
        return words8(val(w) % R)
    if op == OFFSET:
        c = offset_limbs(w[0], p)
        v = norm(w[0] * p)
        assert c[0] == v[0] + B29 and all(c[k] == v[k] + B29 - 1 for k in range(1, 8)) and c[8] == v[8] - 1
        cmax = max(c[:8]) / B29
        return c + list(struct.unpack("<2I", struct.pack("<d", cmax)))
    if op == SHOUP_PAIR:
        a = from_words(w)
        assert mod == 0 and a < R
        return norm(a) + norm((a << 261) // R)
    if op == GATE:
        h = w[0:9]
        y32, a, b, c, d, sel = (from_words(w[9 + 8 * i: 17 + 8 * i]) for i in range(6))
        c2, n = w[57:66], w[66]
        # k_gate_eval's comment: h below 2 r and exactly normalised, every loaded value canonical
        assert is_norm(h) and val(h) < 2 * p and max(y32, a, b, c, d, sel) < p and c2 == offset_limbs(2, p) and 1 <= n <= 64
        for _ in range(n):
            bc = core_out(val(norm(b)) * 32 * c, p)
            g, wrapped = sub_limbs([x + y for x, y in zip(norm(a), bc)], norm(d), c2)
            assert not wrapped and val(g) < 5 * p and all(h[k] + g[k] < 6 * B29 for k in range(9))
            h = core_out(val(h) * y32 + val(g) * 32 * sel, p)
            assert val(h) < 2 * p     # the invariant l9_canon at the end of the kernel relies on
        return h + words8(val(h) % p)
    raise AssertionError(op)


def expect_ec(op, tag, w):
    """madd_l9 / mdbl_l9 / the chain: returns a list of expected affine points (None: identity), one per output record"""
    if op == MDBL:
        x, y = w[0:9], w[9:18]
        assert is_norm(x) and is_norm(y) and val(x) < Q and val(y) <= 2 * Q
        if val(y) % Q == 0:
            return [None]
        pt = (val(x) * pow(RP, -1, Q) % Q, val(y) * pow(RP, -1, Q) % Q)
        return [ec_add(pt, pt)]
    acc = list(w[:37])
    acc_check_bounds(acc)
    cur = acc_affine(acc)
    steps = [w[37:54]] if op == MADD else [w[37 + 17 * s: 54 + 17 * s] for s in range(CHAIN)]
    out = []
    for s in steps:
        px, py = from_words(s[0:8]), from_words(s[8:16])
        assert px < Q and py < Q and (px, py) != (0, 0) and s[16] in (0, 1)
        pt = (px * pow(RP, -1, Q) % Q, py * pow(RP, -1, Q) % Q)
        assert (pt[0] ** 3 + 3 - pt[1] ** 2) % Q == 0
        cur = ec_add(cur, ec_neg(pt) if s[16] else pt)
        out.append(cur)
    return out


def check_ec_output(want_pts, words, tag):
    assert len(words) == 37 * len(want_pts)
    for i, want in enumerate(want_pts):
        rec = words[37 * i: 37 * i + 37]
        assert rec[36] in (0, 1)
        acc_check_bounds(rec)
        assert acc_affine(rec) == want, (tag, i)


# ---- case files ---------------------------------------------------------------------------------------------------------------------
class Block:
    def __init__(self, op, mod, cases, nin=NIN, names=NAMES):
        self.op, self.mod, self.cases = op, mod, cases
        assert cases and all(len(w) == nin[op] and all(0 <= x < U32 for x in w) for _, w in cases), names[op]

    def classes(self):
        c = {}
        for tag, _ in self.cases:
            key = tag.split("/")[0]
            c[key] = c.get(key, 0) + 1
        return c


def write_cases(path, blocks, magic=MAGIC):
    with open(path, "wb") as f:
        f.write(struct.pack("<2I", magic, len(blocks)))
        for b in blocks:
            f.write(struct.pack("<3I", b.op, b.mod, len(b.cases)))
            for _, w in b.cases:
                f.write(struct.pack(f"<{len(w)}I", *w))


def read_results(path, blocks, nout=NOUT, names=NAMES, magic=MAGIC):
    """-> per block, one list of output words per case; asserts that the probe returned exactly one record per case.  `nout` / `names` /
    `magic`: the result widths, op names and file magic of the probe that wrote the file (tests/u256_model.py and tests/ec_model.py share
    the format)"""
    data = open(path, "rb").read()
    assert len(data) % 4 == 0
    words = struct.unpack(f"<{len(data) // 4}I", data)
    assert words[0] == magic and words[1] == len(blocks)
    pos, res = 2, []
    for b in blocks:
        assert words[pos: pos + 3] == (b.op, b.mod, len(b.cases)), names[b.op]
        pos += 3
        n = nout[b.op]
        res.append([list(words[pos + i * n: pos + (i + 1) * n]) for i in range(len(b.cases))])
        pos += n * len(b.cases)
        assert len(res[-1]) == len(b.cases) and all(len(x) == n for x in res[-1])
    assert pos == len(words)
    return res


# ---- generators ---------------------------------------------------------------------------------------------------------------------
N_RANDOM = 2000
JS_WIDE = (2, 3, 4, 5, 6, 7, 8, 13, 14, 32, 33, 34, 64, 168, 169, 500, 1031)


def one_at_a_time(hi, lo=0):
    return [[hi if k == j else lo for k in range(9)] for j in range(9)]


def gen_mul(mod, rng):
    p = P[mod]
    full = [M29] * 9
    cs = [("corner/all", [LIM61] * 9 + full)]
    cs += [("corner/one-a", a + full) for a in one_at_a_time(LIM61)]
    cs += [("corner/one-b", [LIM61] * 9 + b) for b in one_at_a_time(M29)]
    cs += [("corner/one-low", a + full) for a in one_at_a_time(0, LIM61)]
    bound = LIM61 << 232
    for va in edge_values(p, bound, JS_WIDE):
        for ra in reps(va, LIM61 + 1):
            for vb in (0, 1, p - 1, p, 2 * p - 1, T261 - 1):
                cs.append(("value", ra + norm(vb)))
    for _ in range(N_RANDOM):
        cs.append(("random", [rng.randint(0, LIM61) for _ in range(9)] + [rng.randint(0, M29) for _ in range(9)]))
    return Block(MUL, mod, cs)


def gen_mul2(mod, rng):
    p = P[mod]
    full = [M29] * 9
    tot = 6 * B29 - 1
    cs = []
    for name, a1 in (("0/6", 0), ("3/3", 3 * B29), ("5/1", 5 * B29), ("6/0", tot)):
        cs.append((f"corner/all {name}", [a1] * 9 + full + [tot - a1] * 9 + full))
        for j in range(9):
            A1 = [a1 if k == j else 0 for k in range(9)]
            A2 = [tot - a1 if k == j else 0 for k in range(9)]
            cs.append((f"corner/one {name}", A1 + full + A2 + full))
    for va in edge_values(p, (3 * B29 - 1) << 232, JS_WIDE):
        for ra in reps(va, 3 * B29):
            for vb in (0, 1, p - 1, 2 * p - 1):
                cs.append(("value", ra + norm(vb) + norm(vb) + norm(p - 1)))
                cs.append(("value", norm(p - 1) + norm(vb) + ra + norm(T261 - 1)))
    for _ in range(N_RANDOM):
        t = [rng.randint(0, tot) for _ in range(9)]
        a1 = [rng.randint(0, x) for x in t]
        cs.append(("random", a1 + [rng.randint(0, M29) for _ in range(9)] + [x - y for x, y in zip(t, a1)] + [rng.randint(0, M29) for _ in range(9)]))
    return Block(MUL2, mod, cs)


def gen_sqr(mod, rng):
    p = P[mod]
    top = B29 + 7
    cs = [("corner/all", [top] * 9)] + [("corner/one", a) for a in one_at_a_time(top)] + [("corner/one-low", a) for a in one_at_a_time(0, top)]
    for va in edge_values(p, top << 232, JS_WIDE):
        for ra in reps(va, B29 + 8):
            cs.append(("value", ra))
    for _ in range(N_RANDOM):
        cs.append(("random", [rng.randint(0, top) for _ in range(9)]))
    return Block(SQR, mod, cs)


def shoup_v_top():
    """limbs 0..7 at floor(6.1 * 2^29), limb 8 the largest that keeps the value below 2^261"""
    low = val([LIM61] * 8 + [0])
    l8 = (T261 - 1 - low) >> 232
    v = [LIM61] * 8 + [l8]
    assert val(v) < T261 <= val(v) + (1 << 232)
    return v


def gen_shoup(mod, rng):
    p = P[mod]
    ws = [0, 1, p - 1, (p - 1) // 2] + [rng.randrange(p) for _ in range(4)]
    pair = lambda w: norm(w) + norm((w << 261) // p)
    cs = []
    vtop = shoup_v_top()
    for w in ws:
        cs.append(("corner/all", vtop + pair(w)))
        for j in range(8):
            cs.append(("corner/one", [LIM61 if k == j else 0 for k in range(9)] + pair(w)))
        cs.append(("corner/one", [0] * 8 + [M29] + pair(w)))
    for v in edge_values(p, T261, tuple(range(2, 170))) + [T261 - 1]:
        for rv in reps(v, LIM61 + 1):
            for w in ws[:5]:
                cs.append(("value", rv + pair(w)))
    for _ in range(N_RANDOM):
        v = [rng.randint(0, LIM61) for _ in range(8)]
        v.append(rng.randint(0, (T261 - 1 - val(v + [0])) >> 232))
        cs.append(("random", v + pair(rng.randrange(p))))
    return Block(SHOUP, mod, cs)


def gen_u256_ops(mod, rng):
    p = P[mod]
    canon = [0, 1, 2, p - 1, p - 2, (p - 1) // 2, (1 << 253), (1 << 232) - 1, 1 << 232] + [rng.randrange(p) for _ in range(N_RANDOM)]
    wide = canon + [p, p + 1, 2 * p - 1, 2 * p, (1 << 256) - 1, (1 << 255), M29, B29] + [rng.randrange(1 << 256) for _ in range(N_RANDOM)]
    tag = lambda i, n: "edge" if i < n else "random"
    blocks = [Block(FROM_MONT, mod, [(tag(i, 9), words8(a)) for i, a in enumerate(canon)])]
    mm = [("edge", words8(a) + words8(b)) for a in canon[:9] for b in canon[:9]]
    mm += [("random", words8(rng.randrange(p)) + words8(rng.randrange(p))) for _ in range(N_RANDOM)]
    blocks.append(Block(MONT_MUL, mod, mm))
    blocks.append(Block(SPLIT, mod, [(tag(i, 9), words8(a)) for i, a in enumerate(wide)]))
    blocks.append(Block(SPLIT32, mod, [(tag(i, 9), words8(a)) for i, a in enumerate(wide)]))
    blocks.append(Block(PACK, mod, [(tag(i, 9), norm(a)) for i, a in enumerate(wide)]))
    return blocks


def gen_limb_ops(mod, rng):
    p = P[mod]
    blocks = []
    big = U32 - 8
    # l9_renorm: limbs below 2^32, the top limb with room for its carry
    cs = [("corner/all", [U32 - 1] * 8 + [big])] + [("corner/one", a[:8] + [min(a[8], big)]) for a in one_at_a_time(U32 - 1)]
    cs += [("corner/seven", [7 * B29] * 9), ("corner/zero", [0] * 9)]
    for v in edge_values(p, 1 << 264, JS_WIDE):
        cs += [("value", x) for x in reps(v, U32)]
    cs += [("random", [rng.randint(0, U32 - 1) for _ in range(8)] + [rng.randint(0, big)]) for _ in range(N_RANDOM)]
    blocks.append(Block(RENORM, mod, cs))
    # l9_carry: every limb with room for the carry from below
    cs = [("corner/all", [big] * 9)] + [("corner/one", a) for a in one_at_a_time(big)]
    cs += [("corner/seven", [7 * B29] * 9), ("corner/ripple", [M29] * 8 + [0]), ("corner/ripple", [B29] + [M29] * 7 + [0]), ("corner/zero", [0] * 9)]
    for v in edge_values(p, 1 << 264, JS_WIDE):
        cs += [("value", x) for x in reps(v, big + 1)]
    cs += [("random", [rng.randint(0, big) for _ in range(9)]) for _ in range(N_RANDOM)]
    blocks.append(Block(CARRY, mod, cs))
    # l9_add: no limb sum reaches 2^32
    cs = [("corner/all", [U32 - 1] * 9 + [0] * 9), ("corner/all", [1 << 31] * 9 + [(1 << 31) - 1] * 9), ("corner/seven", [6 * B29] * 9 + [M29] * 9)]
    for va in edge_values(p, 1 << 260, JS_WIDE):
        for ra in reps(va, 2 * B29):
            cs += [("value", ra + norm(vb)) for vb in (0, 1, p - 1, 2 * p)]
    for _ in range(N_RANDOM):
        s = [rng.randint(0, U32 - 1) for _ in range(9)]
        a = [rng.randint(0, x) for x in s]
        cs.append(("random", a + [x - y for x, y in zip(s, a)]))
    blocks.append(Block(ADD, mod, cs))
    # l9_canon and l9_is_zero_mod: exactly normalised, below 2 p
    vs = [0, 1, p - 1, p, p + 1, 2 * p - 1, p ^ 1, p ^ (1 << 232), p ^ (1 << 116), 1 << 232, 1 << 29]
    cs = [("edge", norm(v)) for v in vs] + [("random", norm(rng.randrange(2 * p))) for _ in range(N_RANDOM)]
    blocks.append(Block(CANON, mod, cs))
    cs = [("edge", norm(v)) for v in vs] + [("edge/one-limb-off", norm(p ^ (1 << (29 * k)))) for k in range(9)]
    cs += [("edge/one-limb-set", norm(1 << (29 * k))) for k in range(9)] + [("random", norm(rng.randrange(2 * p))) for _ in range(N_RANDOM)]
    blocks.append(Block(IS_ZERO, mod, cs))
    return blocks


# the largest subtrahend each use site documents, in units of p / 10, with the offset it is subtracted from and the largest minuend
# limb (units of 2^29 / 100) the site documents:  (field, K, subtrahend bound * 10, minuend limb bound * 100, where)
# (field, K, subtrahend bound * 10, minuend limb bound * 100 — None: what ntt_dev's carry schedule allows, 7.95 units less the offset's
#  largest limb —, the limb bound * 100 the site states for the difference, where)
SUB_SITES = [
    (1, 8, 75, 100, 300, "madd_l9: acc.x and x3 (< 7.5 q) from a product"),
    (1, 8, 36, 100, 300, "madd_l9: acc.y (< 3.6 q) from a product"),
    (1, 8, 51, 100, 300, "mdbl_l9: x3 (< 5.1 q) from a product"),
    (1, 2, 11, 100, 300, "madd_l9 / mdbl_l9: a product (< 1.1 q) from a product"),
    (0, 34, 320, 100, 300, "polyops: 32 a for a canonical a (l9_split32) from a product or another such value"),
    (0, 9, 71, 100, 300, "polyops: a product of two loaded values (< 6.1 r + r) from another"),
    (0, 2, 10, 200, 410, "k_gate_eval: a canonical value from a + b c"),
    (0, 14, 130, None, 800, "k_ntt_pass: a value below 13 r from a minuend at the carry schedule's limit"),
    (0, 14, 30, None, 800, "k_ntt_pass: a Shoup product (< 3 r) from a minuend at the carry schedule's limit"),
]


def gen_sub(mod, rng, host):
    p = P[mod]
    sub, neg = [], []
    for K in OFFSETS_IN_USE[mod]:
        c = offset_limbs(K, p)
        # the exact edge of the domain, derived from the offset's limbs: t_k <= c_k for every k.  Limbs 0..7 of c are at least 2^29 - 1,
        # so any t with limbs 0..7 below 2^29 passes there and the condition is on the top limb alone: t_8 <= c_8 = floor(K p / 2^232) - 1
        assert min(c[:8]) >= M29
        edge = [M29] * 8 + [c[8]]
        for a in ([0] * 9, [M29] * 9, norm(p - 1)):
            sub.append((f"edge-in/K={K}", a + edge + c))
            sub.append((f"edge-in/K={K}", a + norm(c[8] << 232) + c))
        neg.append((f"edge-in/K={K}", edge + c))
        for k in range(9):
            t = [c[j] if j == k else 0 for j in range(9)]
            sub.append((f"edge-in-limb/K={K}", [0] * 9 + t + c))
        if host:
            sub.append((f"ood:edge-out/K={K}", [0] * 9 + [0] * 8 + [c[8] + 1] + c))
            neg.append((f"ood:edge-out/K={K}", [0] * 8 + [c[8] + 1] + c))
            for k in range(9):
                t = [c[j] + 1 if j == k else 0 for j in range(9)]
                sub.append((f"ood:edge-out-limb/K={K}", [0] * 9 + t + c))
        # the header's old statement "value below (K - 1) p" lies inside the domain, and so do j p + {0, 1, p - 1}
        for j in range(K):
            for v in (j * p, j * p + 1, j * p + p - 1):
                if v >> 232 <= c[8]:
                    sub.append((f"value/K={K}", norm(p - 1) + norm(v) + c))
                    sub.append((f"value/K={K}", [0] * 9 + norm(v) + c))
                    neg.append((f"value/K={K}", norm(v) + c))
        for _ in range(N_RANDOM // 4):
            t = [rng.randint(0, M29) for _ in range(8)] + [rng.randint(0, c[8])]
            a = [rng.randint(0, U32 - 1 - c[k] + t[k]) for k in range(9)]
            sub.append((f"random/K={K}", a + t + c))
            neg.append((f"random/K={K}", t + c))
        # a subtrahend as one parallel carry pass leaves it (limbs of 2^29 + 7) against a minuend limb of 0: in the domain exactly
        # when every c_k reaches 2^29 + 7, i.e. for no limb k with v_k < 8 (k > 0) resp. v_0 < 7
        ren = [B29 + 7] * 8 + [0]
        wraps = [k for k in range(8) if c[k] < B29 + 7]
        if not wraps:
            sub.append((f"renormalised-in/K={K}", [0] * 9 + ren + c))
        elif host:
            sub.append((f"ood:renormalised-out/K={K}", [0] * 9 + ren + c))
    for m, K, t10, a100, o100, _ in SUB_SITES:
        if m != mod:
            continue
        c = offset_limbs(K, p)
        t = norm(t10 * p // 10 - 1)
        amax = (795 * B29 // 100 - max(c[:8])) if a100 is None else a100 * B29 // 100 - 1
        out, wrapped = sub_limbs([amax] * 9, t, c)
        # the site's own statement about the difference's limbs (and with it: nothing reaches 2^32; a difference that goes straight
        # into l9_mul2 beside a normalised h stays below 6 * 2^29 together with it)
        assert not wrapped and max(out[:8]) < o100 * B29 // 100 and (K == 14 or max(out[:8]) + B29 < 6 * B29), (K, t10)
        sub.append((f"site/K={K} t<{t10 / 10}p", [amax] * 9 + t + c))
        sub.append((f"site/K={K} t<{t10 / 10}p", [0] * 9 + t + c))
        neg.append((f"site/K={K} t<{t10 / 10}p", t + c))
    return [Block(SUB, mod, sub), Block(NEG, mod, neg)]


def renormalised_wrap_limbs(mod, K):
    c = offset_limbs(K, P[mod])
    return [k for k in range(8) if c[k] < B29 + 7]


def gen_gate(mod, rng):
    p = P[mod]
    c2 = offset_limbs(2, p)
    mk = lambda h, y, a, b, c, d, s, n: norm(h) + words8(y) + words8(a) + words8(b) + words8(c) + words8(d) + words8(s) + c2 + [n]
    cs = [("worst", mk(2 * p - 1, p - 1, p - 1, p - 1, p - 1, 0, p - 1, n)) for n in (1, 2, 3, 64)]
    cs += [("worst", mk(2 * p - 1, p - 1, p - 1, p - 1, p - 1, p - 1, p - 1, 64)), ("worst", mk(0, 0, 0, 0, 0, p - 1, 0, 64))]
    for _ in range(200):
        cs.append(("random", mk(rng.randrange(2 * p), *(rng.randrange(p) for _ in range(6)), rng.randint(1, 64))))
    return Block(GATE, mod, cs)


def gen_host_only(mod, rng):
    blocks = [Block(OFFSET, mod, [(f"K={K}", [K]) for K in OFFSETS_IN_USE[mod]])]
    if mod == 0:
        ws = [0, 1, 2, R - 1, (R - 1) // 2, 1 << 253] + [rng.randrange(R) for _ in range(300)]
        blocks.append(Block(SHOUP_PAIR, 0, [("edge" if i < 6 else "random", words8(w)) for i, w in enumerate(ws)]))
    return blocks


def gen_canon_wide(rng):
    low = val([U32 - 1] * 8 + [0])
    l8 = ((1 << 259) - 1 - low) >> 232
    cs = [("corner/all", [U32 - 1] * 8 + [l8])] + [("corner/one", [U32 - 1 if k == j else 0 for k in range(9)]) for j in range(8)]
    cs.append(("corner/one", [0] * 8 + [(1 << 27) - 1]))
    jmax = ((1 << 259) - 1) // R
    for j in range(jmax + 1):
        for v in (j * R, j * R + 1, j * R + R - 1):
            if v < 1 << 259:
                cs += [("value", x) for x in reps(v, U32)]
    assert (jmax + 1) * R > 1 << 259
    for _ in range(N_RANDOM):
        l = [rng.randint(0, U32 - 1) for _ in range(8)]
        l.append(rng.randint(0, ((1 << 259) - 1 - val(l + [0])) >> 232))
        cs.append(("random", l))
    for _ in range(N_RANDOM // 2):   # the lazy shape the last NTT pass really hands over: limbs of a few units, value below 22 r
        v = rng.randrange(22 * R)
        cs.append(("random", rng.choice(reps(v, 8 * B29))))
    return Block(CANON_WIDE, 0, cs)


def acc_js(cs):
    """every j for which coordinate + j q stays inside AccL9's bound"""
    return [[j for j in range(9) if c + j * Q < b] for c, b in zip(cs, ACC_BOUNDS)]


def gen_ec(rng):
    madd, mdbl, chains = [], [], []
    G = (1, 2)
    pts = [G, ec_mul(2, G), ec_mul(3, G)] + [ec_point(rng) for _ in range(12)]
    # accumulators whose coordinates are x + j q for every j the bounds allow
    for a_pt in pts[:6]:
        base = acc_words(a_pt, rng)
        cs = [val(base[9 * i: 9 * i + 9]) for i in range(4)]
        for i, js in enumerate(acc_js(cs)):
            for j in js:
                w = list(base)
                w[9 * i: 9 * i + 9] = norm(cs[i] + j * Q)
                for neg in (0, 1):
                    madd.append((f"plus-jq/coord {i}", w + point_words(pts[6], neg)))
        allj = [max(js) for js in acc_js(cs)]
        w = []
        for c, j in zip(cs, allj):
            w += norm(c + j * Q)
        for neg in (0, 1):
            madd.append(("plus-jq/all-max", w + [0] + point_words(pts[7], neg)))
    # the exceptional cases
    for a_pt in pts[:8]:
        for js in ((0, 0, 0, 0), (6, 2, 0, 0)):
            acc = acc_words(a_pt, rng, js)
            madd.append(("same-point", acc + point_words(a_pt, 0)))
            madd.append(("same-point", acc + point_words(ec_neg(a_pt), 1)))
            madd.append(("opposite-point", acc + point_words(a_pt, 1)))
            madd.append(("opposite-point", acc + point_words(ec_neg(a_pt), 0)))
        for neg in (0, 1):
            madd.append(("from-identity", acc_words(None, rng) + point_words(a_pt, neg)))
    for _ in range(N_RANDOM // 2):
        a_pt = ec_point(rng)
        js = [rng.choice(x) for x in acc_js([Q - 1] * 4)]
        madd.append(("random", acc_words(a_pt, rng, js) + point_words(ec_point(rng), rng.randint(0, 1))))
    # mdbl_l9 directly: x canonical, y canonical or 2 q - y (a negated input point), and the 2-torsion test at y = 0 and y = q
    for pt in pts + [ec_point(rng) for _ in range(200)]:
        x, y = pt[0] * RP % Q, pt[1] * RP % Q
        mdbl.append(("point", norm(x) + norm(y)))
        mdbl.append(("point-negated", norm(x) + norm(2 * Q - y)))
    mdbl += [("two-torsion", norm(5) + norm(0)), ("two-torsion", norm(5) + norm(Q))]
    # chains: the output accumulator feeds the next addition
    for ci in range(24):
        start = None if ci % 2 == 0 else ec_point(rng)
        cur, steps, w = start, [], acc_words(start, rng, (0, 0, 0, 0))
        pool = [ec_point(rng) for _ in range(4)]
        for s in range(CHAIN):
            kind = rng.random()
            if cur is not None and kind < 0.08:
                pt, neg = cur, 0                       # same point: the doubling path
            elif cur is not None and kind < 0.14:
                pt, neg = cur, 1                       # opposite point: back to the identity
            elif kind < 0.5:
                pt, neg = rng.choice(pool), rng.randint(0, 1)
            else:
                pt, neg = ec_point(rng), rng.randint(0, 1)
            cur = ec_add(cur, ec_neg(pt) if neg else pt)
            w = w + point_words(pt, neg)
        chains.append(("chain", w))
    return [Block(MADD, 1, madd), Block(MDBL, 1, mdbl), Block(MADD_CHAIN, 1, chains)]


def build_blocks(host, seed=20261016):
    """the case file of one mode: every op that exists in that mode, both fields; out-of-domain cases only when `host`"""
    blocks = []
    for mod in (0, 1):
        rng = random.Random(seed + mod)
        blocks += [gen_mul(mod, rng), gen_mul2(mod, rng), gen_sqr(mod, rng), gen_shoup(mod, rng)]
        blocks += gen_u256_ops(mod, rng) + gen_limb_ops(mod, rng) + gen_sub(mod, rng, host) + [gen_gate(mod, rng)]
        if host:
            blocks += gen_host_only(mod, rng)
    if not host:
        rng = random.Random(seed + 2)
        blocks += [gen_canon_wide(rng)] + gen_ec(rng)
    return blocks


def check_block(b, results):
    """every result of a block against the model; returns the number of cases checked"""
    assert len(results) == len(b.cases) > 0
    for (tag, w), got in zip(b.cases, results):
        if b.op in (MADD, MDBL, MADD_CHAIN):
            check_ec_output(expect_ec(b.op, tag, w), got, tag)
        else:
            want = expect(b.op, b.mod, tag, w)
            assert got == want, (NAMES[b.op], "Fq" if b.mod else "Fr", tag, w, got, want)
    return len(results)


# ---- the probe -----------------------------------------------------------------------------------------------------------------------
def compile_probe(dirname, name="l9_probe"):
    exe = os.path.join(str(dirname), name)
    subprocess.run([HIPCC, "-O2", "-std=c++17", "--offload-arch=gfx950", "-Wno-unused-function", "-o", exe, os.path.join(ROOT, "tools", name + ".hip")],
                   check=True, capture_output=True, text=True)
    return exe


def run_probe(exe, mode, blocks, dirname, timeout, nout=NOUT, names=NAMES, magic=MAGIC):
    """one child process; a non-zero or signal exit fails with the child's stderr; nothing is retried"""
    cases, out = os.path.join(str(dirname), f"cases{mode}.bin"), os.path.join(str(dirname), f"out{mode}.bin")
    write_cases(cases, blocks, magic)
    r = subprocess.run([exe, mode, cases, out], capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, f"{os.path.basename(exe)} {mode} exited with {r.returncode}:\n{r.stderr}"
    return read_results(out, blocks, nout, names, magic)
