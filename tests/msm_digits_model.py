"""Python-integer model of the MSM sort's digit code (halo2_vectordb_amd/csrc/msm_digits.hpp) and the scalar families shared by
tests/test_msm_digits_cpu.py and tests/test_gpu_msm_scaled_records.py.

Written from the definitions: a scalar v < r stands for the folded magnitude s = min(v, r - v) with the sign of v > (r - 1) / 2; its signed
window digits are the one sequence d_j in (-2^(c-1), 2^(c-1)] with sum d_j 2^(c j) = s; it is short iff s = s' 2^(c j0) with j0 = (trailing
zero bits of s) // c, s' < 2^32 and bit length of s' <= min(3 c - 1, 32)."""
import l9_model as L

R = L.R
HALF = (R - 1) // 2
MAGIC = 0x4D534444
CS = (2, 5, 8, 11, 14)
REC_VALID = 1 << 63
ZERO, SHORT, LONG = range(3)


def windows(c):
    return -(-254 // c)


def short_bits(c):
    return min(3 * c - 1, 32)


def nout(c):
    return 2 * (windows(c) + 1) + 6


def fold(v):
    assert 0 <= v < R
    return (R - v, True) if v > HALF else (v, False)


def digits(v, c):
    """[(window, |digit|, negative)] of every non-zero signed digit, windows ascending"""
    s, neg = fold(v)
    half, full, out, j, acc = 1 << (c - 1), 1 << c, [], 0, 0
    while s:
        d = s & (full - 1)
        if d > half:
            d -= full
        s = (s - d) >> c
        if d:
            out.append((j, abs(d), neg != (d < 0)))
            acc += d << (c * j)
        j += 1
    assert j <= windows(c) and acc == fold(v)[0] and all(1 <= d <= half for _, d, _ in out)
    return out


def classify(v, c):
    """(kind, j0, nb', s') as the probe prints them: j0 and nb' for every non-zero scalar, s' for a short one"""
    s, _ = fold(v)
    if s == 0:
        return ZERO, 0, 0, 0
    tz = (s & -s).bit_length() - 1
    j0 = tz // c
    sp = s >> (c * j0)
    assert sp << (c * j0) == s and sp % (1 << c) != 0
    is_short = sp < 1 << 32 and sp.bit_length() <= short_bits(c)
    return (SHORT if is_short else LONG), j0, sp.bit_length(), (sp if is_short else 0)


def record(v, c):
    kind, j0, nbp, sp = classify(v, c)
    if kind != SHORT:
        return 0
    assert j0 < 128 and nbp < 256
    return REC_VALID | nbp << 40 | j0 << 33 | int(fold(v)[1]) << 32 | sp


def expect(v, c):
    """the probe's output words for one scalar"""
    W = windows(c)
    word = lambda t: t[0] << 16 | int(t[2]) << 15 | t[1]
    lst = [word(t) for t in digits(v, c)]
    full = [len(lst)] + lst + [0] * (W - len(lst))
    kind, j0, nbp, sp = classify(v, c)
    rec = record(v, c)
    dec = full if kind == SHORT else [0] * (W + 1)
    return full + [kind, j0, nbp, sp, rec & 0xFFFFFFFF, rec >> 32] + dec


# ---- scalars -------------------------------------------------------------------------------------------------------------------------
def mantissas(c):
    return [1, 3, 1 << (c - 1), (1 << (c - 1)) + 1, (1 << c) - 1, 1 << c, 1 << 31, (1 << 32) - 1, 1 << 32, (1 << 32) + 1]


def families(c, rng, n_random=2000):
    """{family: [scalars below r]}; every family but "edge" and the random ones also holds r - v for each of its v"""
    W = windows(c)
    fam = {"edge": [0, 1, HALF, HALF + 1, R - 1]}
    fam["pow"] = [a << e for a in mantissas(c) for e in range(254) if a << e < R]
    # all-ones mantissas: every digit of s' takes the carry of the one below, and the last carry leaves through the top of s'
    ms = sorted({c - 1, c, c + 1, 2 * c, 3 * c - 2, 3 * c - 1, 3 * c, 31, 32, 33, 47, 64} | set(range(1, 8)))
    fam["ones"] = [((1 << m) - 1) << e for m in ms for j0 in range(W) for e in {c * j0, c * j0 + 1, c * j0 + c - 1} if ((1 << m) - 1) << e < R]
    # j0 + (windows the walk gives s') reaches W exactly, and would pass it: the walk's  min(nb' / c + 2, W - j0)
    reach = []
    for j0 in range(W):
        for nbp in range(1, short_bits(c) + 2):
            a = rng.getrandbits(nbp) | 1 << (nbp - 1) | 1
            if j0 + nbp // c + 2 >= W and a << (c * j0) <= HALF:
                reach.append(a << (c * j0))
    fam["reach-W"] = reach
    for k in ("pow", "ones", "reach-W"):
        fam[k] = fam[k] + [R - v for v in fam[k] if v]
    fam["random"] = [rng.randrange(R) for _ in range(n_random)]
    sparse = []
    for _ in range(n_random):
        v = 0
        for _ in range(rng.randint(1, 4)):
            v |= rng.getrandbits(rng.randint(1, 2 * c)) << rng.randrange(254)
        sparse.append(v % R if rng.random() < 0.5 else (R - v % R) % R)
    fam["sparse"] = sparse
    assert all(0 <= v < R for vs in fam.values() for v in vs)
    return fam
