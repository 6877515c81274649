"""Python-integer model of the 256-bit integer layer under the witness kernels (the u256_* functions of halo2_vectordb_amd/csrc/field.hpp,
Gadgets::divmod_u256 and Gadgets::mont_small of gadgets.hpp) and the case generator shared by tests/test_u256_cpu.py,
tests/test_gpu_u256.py and tests/test_gpu_fp_edges.py.  The probe is tools/u256_probe.hip; the case files are those of tests/l9_model.py.

Expected values are Python integers and nothing else: a // b, a % b, v * 2**256 % r, pow(x, -1, r), >>, <<, masks, int.bit_length.
`classify` mirrors divmod_u256's control flow ONLY to tell which branch each quotient digit takes; no result is compared with it.

Domains, from the comments on the functions (a case outside is not generated):
  u256_shr, u256_shl        s in [0, 255]
  u256_shr_small            0 < s < 32
  u256_low_bits             any bit count; 256 and above keep the value
  u256_bits                 any value (0 for zero)
  u256_extract              len <= 32; any pos, 256 and above give 0
  u256_add, u256_sub        any operands; the carry / borrow out is returned
  divmod_u256               b != 0 (a zero divisor returns q = r = 0 and is the caller's error: not generated)
  mont_small                v < 2^24
  from_mont, to_mont, mont_inv   canonical operands (below r); mont_inv(0) = 0"""
import functools
import random

import l9_model as L

R = L.R
U32 = 1 << 32
M32 = U32 - 1
U256 = 1 << 256
C256 = U256 % R                     # Montgomery form of 1
MU = (C256 << 32) // R              # the constant of mont_small: floor(c 2^32 / r)

(SHR, SHL, SHR_SMALL, LOW_BITS, BITS, EXTRACT, ADD, SUB, DIVMOD, MONT_SMALL, MONT_ROUND, MONT_INV) = range(12)
NAMES = ["u256_shr", "u256_shl", "u256_shr_small", "u256_low_bits", "u256_bits", "u256_extract", "u256_add", "u256_sub", "divmod_u256",
         "mont_small", "from_mont/to_mont", "mont_inv"]
NIN = [9, 9, 9, 9, 8, 10, 16, 16, 16, 1, 8, 8]
NOUT = [8, 8, 8, 8, 1, 1, 9, 9, 16, 8, 16, 8]

w8 = L.words8
fw = L.from_words


# ---- the model ----------------------------------------------------------------------------------------------------------------------
def expect(op, w):
    """the output words of one case; asserts the op's stated domain on the inputs first"""
    a = fw(w[:8]) if op != MONT_SMALL else None
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
    if op == EXTRACT:
        assert w[9] <= 32
        return [(a >> w[8]) & ((1 << w[9]) - 1)]
    if op == ADD:
        s = a + fw(w[8:])
        return w8(s % U256) + [s >> 256]
    if op == SUB:
        d = a - fw(w[8:])
        return w8(d % U256) + [1 if d < 0 else 0]
    if op == DIVMOD:
        b = fw(w[8:])
        assert b != 0
        return w8(a // b) + w8(a % b)
    if op == MONT_SMALL:
        assert w[0] < 1 << 24
        return w8(w[0] * U256 % R)
    if op == MONT_ROUND:
        assert a < R
        c = a * pow(U256, -1, R) % R
        assert c * U256 % R == a
        return w8(c) + w8(a)
    if op == MONT_INV:
        assert a < R
        y = a * pow(U256, -1, R) % R       # the value the Montgomery form a stands for
        inv = pow(y, -1, R) if y else 0
        assert (y * inv % R == 1) if y else inv == 0
        return w8(inv * U256 % R)
    raise AssertionError(op)


def classify(a, b):
    """Which branch every quotient digit of divmod_u256(a, b) takes: None for the early exit (a < 2^(bits of b - 1), or b == 0), else
    dict(skipped, estimated, clamped, fix1, fix2) counting the eight digits.  A mirror of the control flow, never a reference."""
    na, nb = a.bit_length(), b.bit_length()
    if nb == 0 or na < nb:
        return None
    s = 256 - nb
    bn = b << s
    lo = (a << s) % U256
    rem = a >> nb if s else 0
    bt = bn >> 224
    c = dict(skipped=0, estimated=0, clamped=0, fix1=0, fix2=0)
    for _ in range(8):
        full = (rem << 32) | (lo >> 224)      # R8 : R, 288 bits
        lo = (lo << 32) % U256
        top = full >> 224
        if top >= bt:
            e = top // bt
            qh = min(e, M32)
            c["clamped" if e > M32 else "estimated"] += 1
            fixes = qh - full // bn
            assert 0 <= fixes <= 2, (a, b, fixes)
            if fixes:
                c["fix%d" % fixes] += 1
            rem = full % bn
        else:
            c["skipped"] += 1
            rem = full
    return c


@functools.lru_cache(maxsize=None)
def mont_small_one_below():
    """the v < 2^24 where mont_small's quotient estimate floor(v MU / 2^32) is one below floor(v c / r), sorted; asserts that no
    estimate is above or two below (so one conditional subtraction is enough and, for these v, needed)"""
    return _mont_small_scan()[0]


def mont_small_tight():
    """the v < 2^24 whose estimate is exact only just: with MU one larger it would be ABOVE floor(v c / r) (a negative difference)"""
    return _mont_small_scan()[1]


@functools.lru_cache(maxsize=None)
def _mont_small_scan():
    below, tight = [], []
    for v in range(1 << 24):
        m = v * MU
        d = v * C256 // R - (m >> 32)
        if d:
            assert d == 1, v
            below.append(v)
        elif (m + v) >> 32 != m >> 32:
            tight.append(v)
    return below, tight


# ---- generators ---------------------------------------------------------------------------------------------------------------------
def patterns(rng):
    """all-ones, a single set bit at every position, alternating words (both phases), random values"""
    alt = sum(M32 << (64 * i) for i in range(4))
    return ([("ones", U256 - 1)] + [("bit", 1 << i) for i in range(256)] + [("alternating", alt), ("alternating", alt << 32)]
            + [("random", rng.getrandbits(256)) for _ in range(4)])


def gen_shifts(rng):
    pats = patterns(rng)
    shr = [(t, w8(v) + [s]) for s in range(256) for t, v in pats]
    shl = [(t, w8(v) + [s]) for s in range(256) for t, v in pats]
    small = [(t, w8(v) + [s]) for s in range(1, 32) for t, v in pats]
    low = [(t, w8(v) + [n]) for n in range(257) for t, v in pats]
    ext = [(t, w8(v) + [p, n]) for p in (0, 1, 31, 32, 33, 223, 224, 225, 254, 255, 256, 300) for n in (0, 1, 31, 32) for t, v in pats]
    bits = [("zero", w8(0))] + [("bit", w8(1 << i)) for i in range(256)] + [("ones", w8((1 << i) - 1)) for i in range(1, 257)]
    bits += [("random", w8(rng.getrandbits(rng.randrange(1, 257)))) for _ in range(64)]
    return [blk(SHR, shr), blk(SHL, shl), blk(SHR_SMALL, small), blk(LOW_BITS, low), blk(EXTRACT, ext), blk(BITS, bits)]


def gen_add_sub(rng):
    edge = [0, 1, M32, U32, U256 - 1, U256 - 2, 1 << 255, (1 << 255) - 1, R, R - 1] + [(1 << (32 * i)) - 1 for i in range(1, 8)]
    edge += [U256 - (1 << (32 * i)) for i in range(1, 8)]
    pairs = [("edge", a, b) for a in edge for b in edge]
    pairs += [("random", rng.getrandbits(256), rng.getrandbits(256)) for _ in range(1000)]
    pairs += [("carry-chain", x, U256 - x + d) for x in (rng.getrandbits(256) for _ in range(200)) for d in (-1, 0, 1) if 0 <= U256 - x + d < U256]
    cases = [(t, w8(a) + w8(b)) for t, a, b in pairs]
    return [blk(ADD, cases), blk(SUB, cases)]


DIVTEST_SIZES = (1, 2, 31, 32, 33, 63, 64, 65, 95, 96, 97, 100, 127, 128, 129, 148, 160, 191, 192, 193, 224, 250, 255, 256)


def divtest_cases():
    """the 6,912 operand pairs of tools/divtest.hip: its xorshift generator restated (tests/test_u256_cpu.py compares with its output)"""
    st = [0x9E3779B97F4A7C15]
    m64 = (1 << 64) - 1

    def rnd():
        s = st[0]
        s ^= (s << 13) & m64
        s ^= s >> 7
        s ^= (s << 17) & m64
        st[0] = s
        return (s >> 16) & M32

    def rnd_bits(bits):
        v = fw([rnd() for _ in range(8)]) & ((1 << bits) - 1)
        return v | 1 << (bits - 1)

    out = []
    for sa in DIVTEST_SIZES:
        for sb in DIVTEST_SIZES:
            for rep in range(12):
                a, b = rnd_bits(sa), rnd_bits(sb)
                if rep == 1:
                    a = b
                if rep == 2:
                    a = U256 - 1
                if rep == 3:
                    b = 1 << (sb - 1)
                if rep == 4:
                    b = (1 << sb) - 1
                if rep == 5:
                    a = 0
                out.append((a, b))
    return out


def near_top(b, rng):
    """a remainder below b whose top 32 bits (counted from b's top bit) equal b's: the next quotient digit's estimate is clamped.
    None if b has none (32 bits or fewer, or nothing below its top word)"""
    nb = b.bit_length()
    if nb <= 32:
        return None
    low = b & ((1 << (nb - 32)) - 1)
    if low == 0:
        return None
    return b - 1 - rng.randrange(low)


def rand_divisor(rng, nb, bias):
    """a divisor of exactly nb bits; `bias`: a top word of 0x80000000 + small after normalisation followed by ones, where the estimate
    from the top word alone is most often two too large"""
    if bias and nb > 40:
        return (1 << (nb - 1)) | (rng.getrandbits(3) << (nb - 32)) | (((1 << (nb - 32)) - 1) ^ rng.getrandbits(max(nb - 48, 1)))
    return (1 << (nb - 1)) | rng.getrandbits(nb - 1)


def clamp_free(rng):
    """a = ((qh b + rem) << 32 j) + low with rem = near_top(b): digit j - 1 is clamped"""
    while True:
        nb = rng.randrange(33, 225)
        b = rand_divisor(rng, nb, rng.random() < 0.7)
        rem = near_top(b, rng)
        if rem is None:
            continue
        j = rng.randrange(1, (256 - nb) // 32 + 1)
        room = 256 - 32 * j - nb
        qh = rng.getrandbits(room) if room > 0 and rng.random() < 0.8 else 0
        a = ((qh * b + rem) << (32 * j)) | rng.getrandbits(32 * j)
        if a < U256:
            return a, b


def clamp_shifted(rng, P):
    """the chip's shape: a = x << P with x, b < 2^(2P) (qdiv's dividend |a| 2^P), a clamped digit.  The low P bits of the dividend are
    zero, so the remainder in front of digit 0 is (x << (P - 32)) mod b and in front of digit 1 (P = 48) it is (x >> 16) mod b"""
    while True:
        nb = rng.randrange(33, 2 * P + 1)
        b = rand_divisor(rng, nb, rng.random() < 0.7) | 1
        rem = near_top(b, rng)
        if rem is None:
            continue
        if P == 48 and rng.random() < 0.5:
            room = 2 * P - 16 - nb
            if room < 0:
                continue
            x = ((rng.getrandbits(room) * b + rem) << 16) | rng.getrandbits(16)       # digit 1
        else:
            x = rem * pow(1 << (P - 32), -1, b) % b                                     # digit 0: x << (P - 32) == rem mod b
            room = 2 * P - nb
            x += rng.getrandbits(room) * b if room > 0 else 0
        if x < 1 << (2 * P):
            c = classify(x << P, b)
            assert c and c["clamped"], (x, b, P)
            return x << P, b


def fix2_shifted(rng, P):
    """the same shape with a digit that takes the second add-back (found by trying biased divisors; a few tries each)"""
    while True:
        nb = rng.randrange(41, 2 * P + 1)
        b = rand_divisor(rng, nb, True)
        x = rng.getrandbits(2 * P)
        c = classify(x << P, b)
        if c and c["fix2"]:
            return x << P, b


def gen_divmod(rng):
    cases = [("divtest", a, b) for a, b in divtest_cases() if b]
    # early exits and the trivial quotients
    some = [1, 2, 3, M32, U32, U32 + 1, (1 << 64) - 1, 1 << 64, (1 << 128) + 1, 1 << 255, (1 << 255) + 1, U256 - 1, U256 - 2, R]
    some += [rng.getrandbits(n) | 1 << (n - 1) for n in (17, 40, 64, 100, 200, 256)]
    for b in some:
        cases += [("early", 0, b), ("early", b, b), ("early", b, 1), ("early", b - 1, b), ("early", b >> 1, b)]
        cases += [("shift0", a, b) for a in (U256 - 1, 1 << 255, rng.getrandbits(256) | 1 << 255) if b >> 255]
        if b + 1 < U256:
            cases.append(("early", b + 1, b))
    # q b + rem with chosen quotient digits, divisors with all-ones / all-zero low words, lengths on both sides of every word boundary
    lens = sorted({32 * k + d for k in range(8) for d in (-1, 0, 1, 2, 17)} - {-1, 0} | {256, 255})
    for nb in lens:
        if not 1 <= nb <= 256:
            continue
        divs = [(1 << (nb - 1)) | rng.getrandbits(nb - 1), (1 << nb) - 1, 1 << (nb - 1)]
        if nb > 32:
            divs += [(rng.getrandbits(32) | 1 << 31) << (nb - 32), ((rng.getrandbits(32) | 1 << 31) << (nb - 32)) | ((1 << (nb - 32)) - 1)]
        for b in divs:
            nq = (256 - nb) // 32 + 1
            for _ in range(6):
                digits = [rng.choice((0, 1, 0xFFFFFFFE, M32, rng.getrandbits(32))) for _ in range(nq)]
                q = fw(digits + [0] * (8 - nq)) if nq <= 8 else 0
                for rem in {0, 1 % b, b - 1, max(b - 2, 0), rng.randrange(b)}:
                    a = q * b + rem
                    while a >= U256:
                        q >>= 1
                        a = q * b + rem
                    cases.append(("qb+rem", a, b))
    cases += [("clamp",) + clamp_free(rng) for _ in range(1500)]
    for P in (32, 48):
        cases += [("xshl%d-clamp" % P,) + clamp_shifted(rng, P) for _ in range(120)]
        cases += [("xshl%d-fix2" % P,) + fix2_shifted(rng, P) for _ in range(60)]
        cases += [("xshl%d-random" % P, rng.getrandbits(2 * P) << P, rng.getrandbits(rng.randrange(1, 2 * P + 1)) | 1) for _ in range(200)]
    return [blk(DIVMOD, [(t, w8(a) + w8(b)) for t, a, b in cases])]


def gen_mont(rng):
    below = mont_small_one_below()
    vs = [("all16", v) for v in range(1 << 16)]
    vs += [(t, v + d) for v in below for t, d in (("one-below", 0), ("neighbour", -1), ("neighbour", 1)) if v + d < 1 << 24]
    tight = mont_small_tight()
    vs += [("tight", v) for v in tight[:: max(len(tight) // 2000, 1)]]
    vs += [("edge", (1 << 24) - 1)] + [("width", (1 << n) - d) for n in range(2, 21) for d in (1, 2)]
    small = blk(MONT_SMALL, [(t, [v]) for t, v in vs])
    xs = [("edge", v) for v in (0, 1, 2, R - 1, R - 2, (R + 1) // 2, C256, U256 % R * U256 % R)] + [("random", rng.randrange(R)) for _ in range(500)]
    rt = blk(MONT_ROUND, [(t, w8(v)) for t, v in xs])
    ys = [("edge", y) for y in (0, 1, R - 1, 2, (R + 1) // 2)] + [("random", rng.randrange(R)) for _ in range(200)]
    inv = blk(MONT_INV, [(t, w8(y * U256 % R)) for t, y in ys])
    return [small, rt, inv]


def blk(op, cases):
    return L.Block(op, 0, cases, NIN, NAMES)


@functools.lru_cache(maxsize=None)
def build_blocks(seed=20261016):
    rng = random.Random(seed)
    return gen_shifts(rng) + gen_add_sub(rng) + gen_divmod(rng) + gen_mont(rng)


def divmod_pairs(blocks=None):
    """(tag, a, b) of every divmod_u256 case"""
    b = next(x for x in (blocks or build_blocks()) if x.op == DIVMOD)
    return [(t, fw(w[:8]), fw(w[8:])) for t, w in b.cases]


def check_block(b, results):
    assert len(results) == len(b.cases) > 0
    for (tag, w), got in zip(b.cases, results):
        want = expect(b.op, w)
        assert got == want, (NAMES[b.op], tag, [hex(x) for x in w], [hex(x) for x in got], [hex(x) for x in want])
    return len(results)


def compile_probe(dirname):
    return L.compile_probe(dirname, "u256_probe")


def run_probe(exe, mode, blocks, dirname, timeout):
    return L.run_probe(exe, mode, blocks, dirname, timeout, NOUT, NAMES)
