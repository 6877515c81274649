"""Python-integer model of the layer between the product cores and the kernels — the 256-bit field helpers of
halo2_vectordb_amd/csrc/field.hpp (mod_add .. mont_inv, the shifts and bit helpers, k_from_wide's composition) and the u256 XYZZ group law
of ec.hpp — and the case generator shared by tests/test_ec_cpu.py and tests/test_gpu_ec.py.  The probe is tools/ec_probe.hip; the case
files are those of tests/l9_model.py under a magic of their own.

Expected values are Python integers and nothing else: +, -, *, %, pow, >>, <<, masks, int.bit_length, and the affine chord-and-tangent
law of l9_model (ec_add / ec_neg / ec_mul).  No tolerance anywhere.  `expect` asserts the op's stated domain on the inputs first, so a
generator bug cannot move a case outside it; every case is inside, so the same file goes to the host and to the device.

A group output (x, y, zz, zzz in Montgomery form) is held to the model in three ways (check_xyzz): zz = 0 exactly when the model's result
is the identity; otherwise (x / zz, y / zzz) is the model's affine point, zz^3 = zzz^2 and every coordinate is below q."""
import functools
import random

import l9_model as L

R, Q, P = L.R, L.Q, L.P
U32 = 1 << 32
U256 = 1 << 256
U512 = 1 << 512
MAGIC = 0x45435042
CHAIN = 64

(MOD_ADD, MOD_SUB, MOD_NEG, MOD_DBL, MONT_MUL, TO_MONT, FROM_WIDE, MONT_POW, MONT_INV, SHR, SHL, SHR_SMALL, LOW_BITS, BITS, BIT, EXTRACT, CMP,
 XADD, XADD_MIXED, XDBL, XDBL_AFFINE, XFROM_AFFINE, XTO_AFFINE, XMUL, XCHAIN) = range(25)
NAMES = ["mod_add", "mod_sub", "mod_neg", "mod_dbl", "mont_mul (wide)", "to_mont/from_mont", "from_wide", "mont_pow", "mont_inv", "u256_shr",
         "u256_shl", "u256_shr_small", "u256_low_bits", "u256_bits", "u256_bit", "u256_extract", "u256_geq/eq/add/sub", "xyzz_add",
         "xyzz_add_mixed", "xyzz_double", "xyzz_double_affine", "xyzz_from_affine", "xyzz_to_affine", "xyzz_mul", "xyzz_add_mixed chain"]
NIN = [16, 16, 8, 8, 16, 8, 16, 16, 8, 9, 9, 9, 9, 8, 9, 10, 16, 64, 49, 32, 16, 16, 32, 40, 32 + CHAIN * 17]
NOUT = [8, 8, 8, 8, 8, 16, 8, 8, 8, 8, 8, 8, 8, 1, 1, 1, 20, 32, 32, 32, 32, 48, 16, 32, CHAIN * 32]
FIELD_OPS = (MOD_ADD, MOD_SUB, MOD_NEG, MOD_DBL, MONT_MUL, TO_MONT, MONT_POW, MONT_INV)     # both moduli; FROM_WIDE is Fr only
U256_OPS = (SHR, SHL, SHR_SMALL, LOW_BITS, BITS, BIT, EXTRACT, CMP)                         # no modulus: filed under field 0
GROUP_OPS = (XADD, XADD_MIXED, XDBL, XDBL_AFFINE, XFROM_AFFINE, XTO_AFFINE, XMUL)            # Fq only, and XCHAIN

w8 = L.words8
fw = L.from_words
RINV = tuple(pow(U256, -1, p) for p in P)


def mont(v, p):
    return v * U256 % p


# ---- the field and integer ops --------------------------------------------------------------------------------------------------------
def expect(op, mod, tag, w):
    """the output words of one case of a field or integer op"""
    p = P[mod]
    a = fw(w[:8])
    if op in (MOD_ADD, MOD_SUB):
        b = fw(w[8:])
        assert a < p and b < p
        return w8((a + b) % p if op == MOD_ADD else (a - b) % p)
    if op == MOD_NEG:
        assert a < p
        return w8(-a % p)
    if op == MOD_DBL:
        assert a < p
        return w8(2 * a % p)
    if op == MONT_MUL:
        b = fw(w[8:])
        assert a < U256 and b < p
        return w8(a * b * RINV[mod] % p)
    if op == TO_MONT:
        assert a < p or tag.startswith("wide")
        return w8(a * U256 % p) + w8(a % p)
    if op == FROM_WIDE:
        assert mod == 0
        return w8((a + (fw(w[8:]) << 256)) % R * U256 % R)
    if op == MONT_POW:
        assert a < p
        return w8(pow(a * RINV[mod] % p, fw(w[8:]), p) * U256 % p)
    if op == MONT_INV:
        assert a < p
        x = a * RINV[mod] % p
        inv = pow(x, -1, p) if x else 0
        assert (x * inv % p == 1) if x else inv == 0
        return w8(inv * U256 % p)
    if op == SHR:
        assert 0 <= w[8] <= 255
        return w8(a >> w[8])
    if op == SHL:
        assert 0 <= w[8] <= 255
        return w8((a << w[8]) % U256)
    if op == SHR_SMALL:
        assert 0 < w[8] < 32
        return w8(a >> w[8])
    if op == LOW_BITS:
        return w8(a & ((1 << w[8]) - 1))
    if op == BITS:
        return [a.bit_length()]
    if op == BIT:
        assert 0 <= w[8] <= 255
        return [(a >> w[8]) & 1]
    if op == EXTRACT:
        assert w[9] <= 32
        return [(a >> w[8]) & ((1 << w[9]) - 1)]
    if op == CMP:
        b = fw(w[8:])
        return [int(a >= b), int(a == b)] + w8((a + b) % U256) + [(a + b) >> 256] + w8((a - b) % U256) + [int(a < b)]
    raise AssertionError(op)


# ---- the group ops --------------------------------------------------------------------------------------------------------------------
def on_curve(pt):
    return pt is None or (pt[0] ** 3 + 3 - pt[1] ** 2) % Q == 0


def xyzz_words(pt, lam=1, junk=None):
    """the XYZZ words of the affine point `pt` under the scaling lam: (x lam^2, y lam^3, lam^2, lam^3), Montgomery form.  The identity is
    zz = zzz = 0 with x = y = 0, or with the two `junk` values there (only zz decides)"""
    if pt is None:
        x, y = junk or (0, 0)
        return w8(x) + w8(y) + w8(0) + w8(0)
    assert 0 < lam < Q
    l2, l3 = lam * lam % Q, lam * lam * lam % Q
    return w8(mont(pt[0] * l2, Q)) + w8(mont(pt[1] * l3, Q)) + w8(mont(l2, Q)) + w8(mont(l3, Q))


def affine_words(pt):
    return w8(0) + w8(0) if pt is None else w8(mont(pt[0], Q)) + w8(mont(pt[1], Q))


def affine_point(w):
    """16 words -> the affine point (None for (0, 0)); coordinates below q"""
    x, y = fw(w[:8]), fw(w[8:16])
    assert x < Q and y < Q
    return None if x == 0 and y == 0 else (x * RINV[1] % Q, y * RINV[1] % Q)


def xyzz_point(w):
    """32 words -> the affine point an XYZZ value stands for (None when zz = 0); asserts every coordinate below q and, off the identity,
    zz^3 = zzz^2"""
    X, Y, ZZ, ZZZ = (fw(w[8 * i: 8 * i + 8]) for i in range(4))
    assert max(X, Y, ZZ, ZZZ) < Q
    if ZZ == 0:
        return None
    x, y, zz, zzz = (v * RINV[1] % Q for v in (X, Y, ZZ, ZZZ))
    assert zzz and pow(zz, 3, Q) == pow(zzz, 2, Q)
    return x * pow(zz, -1, Q) % Q, y * pow(zzz, -1, Q) % Q


def check_xyzz(rec, want, tag):
    assert len(rec) == 32
    got = xyzz_point(rec)
    assert (fw(rec[16:24]) == 0) == (want is None), tag
    assert got == want, (tag, got, want)


def signed(pt, neg):
    return L.ec_neg(pt) if neg else pt


def expect_group(op, tag, w):
    """the affine points (None: the identity) the XYZZ records of the output stand for, in order"""
    torsion = tag.startswith("two-torsion")
    if op == XADD:
        A, B = xyzz_point(w[:32]), xyzz_point(w[32:])
        assert on_curve(A) and on_curve(B)
        return [L.ec_add(A, B)]
    if op == XADD_MIXED:
        A, Qp = xyzz_point(w[:32]), affine_point(w[32:48])
        assert on_curve(A) and on_curve(Qp) and w[48] in (0, 1)
        return [L.ec_add(A, signed(Qp, w[48]))]
    if op in (XDBL, XDBL_AFFINE):
        if torsion:
            # y = 0: on no point of this curve; the branch is written to return the identity
            assert fw(w[8:16]) == 0 and fw(w[:8]) != 0 and (op == XDBL_AFFINE or fw(w[16:24]) != 0)
            return [None]
        A = xyzz_point(w) if op == XDBL else affine_point(w)
        assert on_curve(A)
        return [L.ec_add(A, A)]
    if op == XFROM_AFFINE:
        A = affine_point(w)
        assert on_curve(A)
        return [A]
    if op == XTO_AFFINE:
        A = xyzz_point(w)
        assert on_curve(A)
        return [A]
    if op == XMUL:
        A = xyzz_point(w[:32])
        assert on_curve(A)
        return [L.ec_mul(fw(w[32:]), A)]
    if op == XCHAIN:
        cur = xyzz_point(w[:32])
        assert on_curve(cur)
        out = []
        for s in range(CHAIN):
            q = w[32 + 17 * s: 49 + 17 * s]
            Qp = affine_point(q)
            assert on_curve(Qp) and q[16] in (0, 1)
            cur = L.ec_add(cur, signed(Qp, q[16]))
            out.append(cur)
        return out
    raise AssertionError(op)


def check_group(op, tag, w, got):
    want = expect_group(op, tag, w)
    if op == XTO_AFFINE:
        assert got == affine_words(want[0]), (tag, got)         # the canonical affine point, exactly
        return
    assert len(got) == NOUT[op]
    for i, pt in enumerate(want):
        check_xyzz(got[32 * i: 32 * i + 32], pt, (NAMES[op], tag, i))
    if op == XFROM_AFFINE:
        assert got[:32] == xyzz_words(want[0]) and got[32:] == affine_words(want[0]), tag     # zz = zzz = 1, and the round trip


def chain_branches(block, results):
    """(doublings, cancellations) the chains walked, read off the results: a step whose addend is the point the previous accumulator
    stands for took the doubling branch, a step from a point to zz = 0 the cancelling one"""
    dbl = ident = 0
    for (_, w), res in zip(block.cases, results):
        prev = xyzz_point(w[:32])
        for s in range(CHAIN):
            q = w[32 + 17 * s: 49 + 17 * s]
            add = signed(affine_point(q), q[16])
            cur = xyzz_point(res[32 * s: 32 * s + 32])
            if prev is not None and add is not None:
                dbl += prev == add
                ident += cur is None
            prev = cur
    return dbl, ident


# ---- generators -----------------------------------------------------------------------------------------------------------------------
N_RANDOM = 2000


def edges(p):
    e = [0, 1, 2, p - 1, p - 2, (p - 1) // 2, (p + 1) // 2, 1 << 253]
    assert all(v < p for v in e)
    return e


def wide(p):
    v = [p, p + 1, 2 * p - 1, 2 * p, 1 << 255, U256 - 1, 5 * p, 5 * p + 1]
    assert all(p <= x < U256 for x in v)
    return v


def blk(op, mod, cases):
    return L.Block(op, mod, cases, NIN, NAMES)


def gen_field(mod, rng):
    p = P[mod]
    E, W = edges(p), wide(p)
    pairs = [("edge", a, b) for a in E for b in E]
    for a in E[1:] + [rng.randrange(2, p) for _ in range(50)]:
        pairs += [(f"sum/{name}", a, t - a) for name, t in (("p-1", p - 1), ("p", p), ("p+1", p + 1)) if 0 <= t - a < p]
    pairs += [("equal", a, a) for a in E + [rng.randrange(p) for _ in range(50)]]
    pairs += [("random", rng.randrange(p), rng.randrange(p)) for _ in range(N_RANDOM)]
    two = [(t, w8(a) + w8(b)) for t, a, b in pairs]
    one = [("edge", w8(a)) for a in E] + [("random", w8(rng.randrange(p))) for _ in range(N_RANDOM)]
    blocks = [blk(MOD_ADD, mod, two), blk(MOD_SUB, mod, two), blk(MOD_NEG, mod, one), blk(MOD_DBL, mod, one)]
    mm = [("wide-edge", w8(a) + w8(b)) for a in W for b in E + [rng.randrange(p) for _ in range(8)]]
    mm += [("wide-random", w8(rng.getrandbits(256)) + w8(E[i % 8] if i % 4 == 0 else rng.randrange(p))) for i in range(N_RANDOM)]
    blocks.append(blk(MONT_MUL, mod, mm))
    tm = [("edge", w8(a)) for a in E] + [("random", w8(rng.randrange(p))) for _ in range(N_RANDOM)]
    tm += [("wide-edge", w8(a)) for a in W] + [("wide-random", w8(rng.getrandbits(256))) for _ in range(N_RANDOM)]
    blocks.append(blk(TO_MONT, mod, tm))
    if mod == 0:
        blocks.append(gen_from_wide(rng))
    bases = [("zero", 0), ("one", 1), ("minus-one", p - 1), ("two", 2), ("random", rng.randrange(p))]
    exps = [("length/0", 0)]
    for b in range(1, 257):
        exps += [(f"length/{b}", 1 << (b - 1)), (f"length/{b}", (1 << b) - 1), (f"length/{b}", rng.getrandbits(b) | 1 << (b - 1))]
    exps += [("special/p-2", p - 2), ("special/p-1", p - 1), ("special/(q+1)/4", (Q + 1) // 4)]
    blocks.append(blk(MONT_POW, mod, [(f"{te}/{ta}", w8(mont(a, p)) + w8(e)) for ta, a in bases for te, e in exps]))
    inv = [("zero", 0), ("edge", 1), ("edge", p - 1), ("edge", 2)] + [("random", rng.randrange(p)) for _ in range(500)]
    blocks.append(blk(MONT_INV, mod, [(t, w8(mont(a, p))) for t, a in inv]))
    return blocks


def from_wide_values(rng):
    """(tag, lo, hi) of every from_wide case: the 512-bit integer is lo + 2^256 hi"""
    V = [0, 1, R - 1, R, R + 1, 2 * R, 1 << 255, U256 - 1]
    cs = [("edge", lo, hi) for lo in V for hi in V]
    kmax = U512 // R
    ks = [1, 2, kmax] + sorted(rng.randrange(3, kmax) for _ in range(8))
    for k in ks:
        for d in (-1, 0, 1):
            v = k * R + d
            if v < U512:
                cs.append((f"multiple/{d:+d}", v % U256, v >> 256))
    cs += [("random", rng.getrandbits(256), rng.getrandbits(256)) for _ in range(N_RANDOM)]
    return cs


def gen_from_wide(rng):
    return blk(FROM_WIDE, 0, [(t, w8(lo) + w8(hi)) for t, lo, hi in from_wide_values(rng)])


def patterns(rng):
    alt = sum((0xA5A5A5A5 if i % 2 == 0 else 0x5A5A5A5A) << (32 * i) for i in range(8))
    return [("ones", U256 - 1), ("one", 1), ("top", 1 << 255), ("alternating", alt)] + [("random", rng.getrandbits(256)) for _ in range(4)]


def gen_u256(rng):
    pats = patterns(rng)
    shifts = [(t, w8(v) + [s]) for s in range(256) for t, v in pats]
    small = [(t, w8(v) + [s]) for s in range(1, 32) for t, v in pats]
    low = [(t, w8(v) + [n]) for n in list(range(257)) + [300, U32 - 1] for t, v in pats]
    vals = [("bit", 1 << i) for i in range(256)] + [("ones", (1 << b) - 1) for b in range(257)]
    bits = [(t, w8(v)) for t, v in vals]
    bit = [(t, w8(v) + [i]) for t, v in vals for i in range(256)]
    ext = [(t, w8(v) + [pos, n]) for pos in (0, 1, 28, 31, 32, 33, 63, 224, 225, 250, 255, 256, 300) for n in (0, 1, 4, 13, 31, 32) for t, v in pats]
    cmp_ = []
    for a in [rng.getrandbits(256) for _ in range(6)] + [0, U256 - 1]:
        for k in range(8):
            limb = (a >> (32 * k)) & (U32 - 1)
            for other in {(limb + 1) % U32, (limb - 1) % U32, limb ^ (1 << 31), rng.getrandbits(32)} - {limb}:
                b = a ^ ((limb ^ other) << (32 * k))
                cmp_ += [(f"one-limb/{k}", a, b), (f"one-limb/{k}", b, a)]
    cmp_ += [("equal", a, a) for a in [0, 1, U256 - 1, 1 << 255, R, Q] + [rng.getrandbits(256) for _ in range(20)]]
    cmp_ += [("wrap", U256 - 1, 1), ("wrap", 0, 1)]
    cmp_ += [("random", rng.getrandbits(256), rng.getrandbits(256)) for _ in range(500)]
    return [blk(SHR, 0, shifts), blk(SHL, 0, shifts), blk(SHR_SMALL, 0, small), blk(LOW_BITS, 0, low), blk(BITS, 0, bits), blk(BIT, 0, bit),
            blk(EXTRACT, 0, ext), blk(CMP, 0, [(t, w8(a) + w8(b)) for t, a, b in cmp_])]


MUL_SCALARS = (0, 1, 2, 3, R - 1, R, R + 1, 1 << 253, (1 << 254) - 1)
JUNK = (5, 7)


def gen_group(rng):
    G = (1, 2)
    pts = [G, L.ec_mul(2, G), L.ec_mul(3, G)] + [L.ec_point(rng) for _ in range(5)]
    lam = lambda: rng.randrange(2, Q)
    idents = [xyzz_words(None), xyzz_words(None, junk=JUNK)]

    def lams(name):
        """(tag, lambda_A, lambda_B): 1 and random on either side; never equal when `name` needs two scalings of one point"""
        out = [("1,r", 1, lam()), ("r,1", lam(), 1), ("r,r", lam(), lam())]
        if name == "random":
            out.append(("1,1", 1, 1))
        assert all(a != b for t, a, b in out if t != "1,1")
        return out

    add = []
    for i, Pt in enumerate(pts):
        Qt = pts[(i + 1) % len(pts)]
        for name, other in (("random", Qt), ("same-point", Pt), ("opposite-point", L.ec_neg(Pt))):
            add += [(f"{name}/{t}", xyzz_words(Pt, la) + xyzz_words(other, lb)) for t, la, lb in lams(name)]
        for t, l in (("1", 1), ("r", lam())):
            for z in idents:
                add += [(f"identity-left/{t}", z + xyzz_words(Pt, l)), (f"identity-right/{t}", xyzz_words(Pt, l) + z)]
    add += [("both-identity", a + b) for a in idents for b in idents]

    mixed = []
    for i, Pt in enumerate(pts):
        Qt = pts[(i + 1) % len(pts)]
        for t, l in (("1", 1), ("r", lam())):
            A = xyzz_words(Pt, l)
            for neg in (0, 1):
                mixed.append((f"random/{t}", A + affine_words(Qt) + [neg]))
                mixed.append((f"same-point/{t}", A + affine_words(signed(Pt, neg)) + [neg]))
                mixed.append((f"opposite-point/{t}", A + affine_words(signed(Pt, 1 - neg)) + [neg]))
                mixed.append((f"identity-right/{t}", A + affine_words(None) + [neg]))
        for z in idents:
            for neg in (0, 1):
                mixed.append(("identity-left", z + affine_words(Pt) + [neg]))
    mixed += [("both-identity", z + affine_words(None) + [neg]) for z in idents for neg in (0, 1)]

    dbl, dbl_aff, frm, to = [], [], [], []
    for Pt in pts + [L.ec_point(rng) for _ in range(24)]:
        Nt = L.ec_neg(Pt)
        dbl += [("point/1", xyzz_words(Pt)), ("point/r", xyzz_words(Pt, lam())), ("point-negated/1", xyzz_words(Nt)), ("point-negated/r", xyzz_words(Nt, lam()))]
        dbl_aff += [("point", affine_words(Pt)), ("point-negated", affine_words(Nt))]
        frm += [("point", affine_words(Pt)), ("point", affine_words(Nt))]
        to += [("point", xyzz_words(Pt)), ("scaled", xyzz_words(Pt, lam())), ("scaled", xyzz_words(Nt, lam()))]
    one = w8(mont(1, Q))
    dbl += [("identity", z) for z in idents] + [("two-torsion", w8(mont(x, Q)) + w8(0) + one + one) for x in (5, Q - 1)]
    dbl_aff += [("identity", affine_words(None))] + [("two-torsion", w8(mont(x, Q)) + w8(0)) for x in (5, Q - 1)]
    frm.append(("identity", affine_words(None)))
    to += [("identity", z) for z in idents]

    mul = []
    scalars = [("edge", s) for s in MUL_SCALARS] + [("random", rng.getrandbits(254)) for _ in range(64)]
    for j, (t, s) in enumerate(scalars):
        Pt = pts[j % len(pts)]
        mul += [(f"point-{t}", xyzz_words(Pt) + w8(s)), (f"scaled-{t}", xyzz_words(Pt, lam()) + w8(s)), (f"identity-{t}", idents[j % 2] + w8(s))]

    # chains over four points and their negatives: half the steps are drawn to cancel a point the sum holds, so the walk stays near the
    # origin and keeps meeting a single pool point (the doubling branch) and its negative (back to the identity)
    chains = []
    for ci in range(16):
        pool = [L.ec_point(rng) for _ in range(4)]
        coef = [0, 0, 0, 0]
        if ci % 2:
            coef[ci % 4] = 1
        start = pool[ci % 4] if ci % 2 else None
        w = xyzz_words(start, lam()) if ci % 4 == 3 else xyzz_words(start)
        for s in range(CHAIN):
            held = [i for i in range(4) if coef[i]]
            if held and rng.random() < 0.5:
                i = rng.choice(held)
                sign = -1 if coef[i] > 0 else 1
            else:
                i, sign = rng.randrange(4), rng.choice((-1, 1))
            coef[i] += sign
            # the same group element either as (Q, neg) or as (-Q, not neg)
            neg = rng.randint(0, 1)
            w = w + affine_words(signed(pool[i], (sign < 0) != bool(neg))) + [neg]
        chains.append(("chain", w))
    return [blk(XADD, 1, add), blk(XADD_MIXED, 1, mixed), blk(XDBL, 1, dbl), blk(XDBL_AFFINE, 1, dbl_aff), blk(XFROM_AFFINE, 1, frm),
            blk(XTO_AFFINE, 1, to), blk(XMUL, 1, mul), blk(XCHAIN, 1, chains)]


# the classes every block must hold (the tag up to the first "/"); asserted by both test files
CLASSES = {
    MOD_ADD: ("edge", "sum", "equal", "random"), MOD_SUB: ("edge", "sum", "equal", "random"), MOD_NEG: ("edge", "random"), MOD_DBL: ("edge", "random"),
    MONT_MUL: ("wide-edge", "wide-random"), TO_MONT: ("edge", "random", "wide-edge", "wide-random"), FROM_WIDE: ("edge", "multiple", "random"),
    MONT_POW: ("length", "special"), MONT_INV: ("zero", "edge", "random"),
    SHR: ("ones", "one", "top", "alternating", "random"), SHL: ("ones", "one", "top", "alternating", "random"),
    SHR_SMALL: ("ones", "one", "top", "alternating", "random"), LOW_BITS: ("ones", "one", "top", "alternating", "random"),
    BITS: ("bit", "ones"), BIT: ("bit", "ones"), EXTRACT: ("ones", "one", "top", "alternating", "random"), CMP: ("one-limb", "equal", "wrap", "random"),
    XADD: ("random", "same-point", "opposite-point", "identity-left", "identity-right", "both-identity"),
    XADD_MIXED: ("random", "same-point", "opposite-point", "identity-left", "identity-right", "both-identity"),
    XDBL: ("point", "point-negated", "identity", "two-torsion"), XDBL_AFFINE: ("point", "point-negated", "identity", "two-torsion"),
    XFROM_AFFINE: ("point", "identity"), XTO_AFFINE: ("point", "scaled", "identity"),
    XMUL: ("point-edge", "point-random", "scaled-edge", "scaled-random", "identity-edge", "identity-random"), XCHAIN: ("chain",),
}


def check_classes(b):
    """every named class of the block has a case, and the finer lists the cases are specified by are complete"""
    have = b.classes()
    assert all(have.get(c, 0) > 0 for c in CLASSES[b.op]), (NAMES[b.op], have)
    tags = {t for t, _ in b.cases}
    if b.op == XADD:
        for name in ("random", "same-point", "opposite-point"):
            assert {f"{name}/{t}" for t in ("1,r", "r,1", "r,r")} <= tags, name
        assert "random/1,1" in tags and {f"identity-{side}/{t}" for side in ("left", "right") for t in ("1", "r")} <= tags
    if b.op == XADD_MIXED:
        for name in ("random", "same-point", "opposite-point", "identity-right"):
            assert {f"{name}/1", f"{name}/r"} <= tags, name
            assert {w[48] for t, w in b.cases if t.startswith(name)} == {0, 1}, name
    if b.op == XDBL:
        assert {"point/1", "point/r", "point-negated/1", "point-negated/r"} <= tags
    if b.op == XMUL:
        assert {fw(w[32:]) for t, w in b.cases if t.endswith("-edge")} == set(MUL_SCALARS)
    if b.op == XCHAIN:
        assert len(b.cases) == 16
    if b.op in (SHR, SHL):
        assert {w[8] for _, w in b.cases} == set(range(256))
    if b.op == SHR_SMALL:
        assert {w[8] for _, w in b.cases} == set(range(1, 32))
    if b.op == LOW_BITS:
        assert {w[8] for _, w in b.cases} == set(range(257)) | {300, U32 - 1}
    if b.op == BIT:
        assert {w[8] for _, w in b.cases} == set(range(256))
    if b.op == MONT_POW:
        assert {t.split("/")[1] for t in tags if t.startswith("length/")} == {str(n) for n in range(257)}
        assert {fw(w[8:]).bit_length() for _, w in b.cases} == set(range(257))
        assert {t.split("/")[-1] for t in tags} == {"zero", "one", "minus-one", "two", "random"}
    if b.op == CMP:
        assert {f"one-limb/{k}" for k in range(8)} <= tags
    if b.op == FROM_WIDE:
        assert {"multiple/-1", "multiple/+0", "multiple/+1"} <= tags and have["edge"] == 64 and have["multiple"] >= 32


@functools.lru_cache(maxsize=None)
def build_blocks(seed=20261018):
    """every op, both fields where the op has a modulus; every case is inside its op's domain, so host and device get the same file"""
    blocks = []
    for mod in (0, 1):
        blocks += gen_field(mod, random.Random(seed + mod))
    blocks += gen_u256(random.Random(seed + 2))
    blocks += gen_group(random.Random(seed + 3))
    return blocks


def check_block(b, results):
    """every result of a block against the model; returns the number of cases checked"""
    assert len(results) == len(b.cases) > 0
    for (tag, w), got in zip(b.cases, results):
        if b.op >= XADD:
            check_group(b.op, tag, w, got)
        else:
            want = expect(b.op, b.mod, tag, w)
            assert got == want, (NAMES[b.op], "Fq" if b.mod else "Fr", tag, [hex(x) for x in w], [hex(x) for x in got], [hex(x) for x in want])
    return len(results)


def compile_probe(dirname):
    return L.compile_probe(dirname, "ec_probe")


def run_probe(exe, mode, blocks, dirname, timeout):
    return L.run_probe(exe, mode, blocks, dirname, timeout, NOUT, NAMES, MAGIC)
