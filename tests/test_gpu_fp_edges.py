"""The rare branches of the witness path's 256-bit integer layer THROUGH THE C ABI (vdb_wit_fp_op, vdb_wit_distance), against the oracle
(`O.Ctx.op`: bit-serial division, table-free limbs), cells, lookup cells and flags bit for bit as tests/test_gpu_fp_ops.py does:
  * qdiv / qmod on operand pairs from the `x << P` classes of tests/u256_model.py (a clamped quotient digit of Gadgets::divmod_u256, a
    second add-back), both signs of both operands; the classifier asserts on the CPU that the pairs the oracle accepts reach them;
  * every operation at the ends of its domain: zero, +-1 ulp, +- the largest magnitude the oracle accepts (bisection on the oracle,
    per op), one ulp beyond, quotients on and next to an integer, perfect squares +-1 ulp, integer arguments and powers of two;
  * lookup widths L = 16 .. 20, where Gadgets::mont_small's final subtraction is live: operands whose range-check limbs are among
    the 4,566 limbs whose quotient estimate is one below.
A case the oracle refuses (c.err != 0) must be refused by the library with VDB_ERR_DOMAIN (-5), alone in its call."""
import random

import numpy as np
import pytest

import u256_model as U
from test_gpu_fp_ops import BINARY, UNARY
from test_gpu_witness import assert_streams

pytestmark = pytest.mark.gpu
R = U.R
PL = [(48, 13), (32, 9)]


@pytest.fixture(scope="module")
def api():
    from halo2_vectordb_amd import api as a
    a.init()
    return a


# ---- the CPU side: cases, the oracle's verdict, what is actually divided --------------------------------------------------------------
def accepts(O, op, a, b, P, L):
    c = O.Ctx(store=False)
    c.op(op, O.fr_from_ints([a])[0], None if b is None else O.fr_from_ints([b])[0], P=P, L=L)
    return c.err == 0


def split_by_oracle(O, op, cases, P, L):
    """-> (accepted cases, refused cases, context holding the accepted ones' streams, their results)"""
    ok, bad = [], []
    for a, b in cases:
        (ok if accepts(O, op, a, b, P, L) else bad).append((a, b))
    c = O.Ctx(store=True, keygen=True)
    qa = O.fr_from_ints([a for a, _ in ok])
    qb = None if op in UNARY else O.fr_from_ints([b for _, b in ok])
    want = np.stack([c.op(op, qa[i], None if qb is None else qb[i], P=P, L=L) for i in range(len(ok))])
    assert c.err == 0
    return ok, bad, c, (qa, qb, want)


def run_and_compare(api, O, op, cases, P, L):
    ok, bad, c, (qa, qb, want) = split_by_oracle(O, op, cases, P, L)
    assert ok
    got = api.wit_fp_op(op, qa, qb, P=P, L=L, selectors=True)
    assert np.array_equal(got["result"], want), op
    assert_streams(got, c)
    for a, b in bad:
        with pytest.raises(api.VdbError) as e:
            api.wit_fp_op(op, O.fr_from_ints([a]), None if b is None else O.fr_from_ints([b]), P=P, L=L)
        assert e.value.code == -5, (op, a, b)
    return ok, bad, c


def divided(op, a, b, P):
    """the canonical (dividend, divisor) that qdiv / qmod hand to divmod_u256 (fixed_point.rs:606-656): magnitudes by the chip's sign
    convention (negative from 2^(2P+1)); qdiv scales the dividend by 2^P, qmod divides by b as it stands"""
    neg = lambda v: v >= 1 << (2 * P + 1)
    aa = R - a if neg(a) else a
    if op == "qdiv":
        return aa * (1 << P) % R, (R - b if neg(b) else b)
    return aa, b


def clamp_cases(op, P):
    """pairs of the model's x << P classes as operands: qdiv divides |a| 2^P by |b|, so a = +-x; qmod divides |a| by b, so
    a = +-(x << P) (the negative one is the dividend x << P)"""
    pairs = [(t, a, b) for t, a, b in U.divmod_pairs() if t in ("xshl%d-clamp" % P, "xshl%d-fix2" % P)]
    cl = [p for p in pairs if p[0].endswith("clamp")][:40] + [p for p in pairs if p[0].endswith("fix2")][:30]
    out = []
    for _, a, b in cl:
        x = a >> P if op == "qdiv" else a
        out += [(x, b), ((R - x) % R, b), (x, R - b), ((R - x) % R, R - b)]
    return out


def branch_counts(op, cases, P):
    n = dict(clamped=0, fix2=0)
    for a, b in cases:
        num, den = divided(op, a, b, P)
        c = U.classify(num, den) if den else None
        if c:
            n["clamped"] += c["clamped"] > 0
            n["fix2"] += c["fix2"] > 0
    return n


def largest_accepted(O, op, P, L, second, top):
    """the largest magnitude in [0, top] the oracle accepts as the first (second) operand, the other one being 1.0: bisection between an
    accepted and a refused magnitude (acceptance taken as monotone in the magnitude; the ends found are cases either way)"""
    one = 1 << P
    acc = lambda m: accepts(O, op, *((one, m) if second else (m, None if op in UNARY else one)), P, L)
    if acc(top):
        return top
    lo = 1
    if not acc(lo):
        return 0
    hi = top
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if acc(mid):
            lo = mid
        else:
            hi = mid
    return lo


def edge_cases(O, op, P, L):
    """(a, b) canonical field values, b None for a unary op"""
    one = 1 << P
    sgn = lambda v: v % R
    if op == "bit_xor":
        return [(a, b) for a in (0, 1) for b in (0, 1)]          # its domain is the four pairs of bits
    top = (1 << 252) if op == "signed_div_scale" else (1 << (2 * P + 1)) - 1   # the sign boundaries: a > 2^252 resp. a >= 2^(2P+1) is negative
    m1 = largest_accepted(O, op, P, L, False, top)
    firsts = [0, 1, -1, m1, -m1, m1 + 1, -(m1 + 1), one, -one]
    if op == "signed_div_scale":
        firsts += [top - 1, 5 * one, 5 * one + 1, 6 * one - 1, -(5 * one), -(5 * one + 1), -(6 * one - 1), one * one, -(one * one) + 1]
    if op == "qsqrt":
        for s in (2, 3, 1.5):
            q = int(s * s * one)
            firsts += [q - 1, q, q + 1]
    if op in ("qexp2", "qexp"):
        firsts += [k * one for k in (-3, -2, 2, 3, 10)] + [3 * one + 1, 3 * one - 1]
    if op in ("qlog2", "qlog", "qsqrt"):
        firsts += [one << k for k in (1, 3, 10)] + [one >> k for k in (1, 3, 10)] + [(one << 3) - 1, (one << 3) + 1, (one >> 3) - 1, (one >> 3) + 1]
    if op in UNARY:
        return [(sgn(a), None) for a in firsts]
    if op == "cond_neg":
        return [(sgn(a), f) for a in firsts for f in (0, 1)]
    m2 = largest_accepted(O, op, P, L, True, top)
    seconds = [0, 1, -1, m2, -m2, m2 + 1, -(m2 + 1)]
    cases = [(sgn(a), one) for a in firsts] + [(one, sgn(b)) for b in seconds] + [(sgn(m1), sgn(m2)), (sgn(-m1), sgn(m2)), (sgn(m1), sgn(-m2))]
    if op in ("qdiv", "qmod"):          # quotient exactly on an integer and one ulp either side, both signs of the dividend
        for k, d in ((3, 2 * one), (7, one // 4), (1, 3 * one + 1), (1 << 20, 5)):
            cases += [(sgn(s * (k * d + e)), d) for s in (1, -1) for e in (-1, 0, 1)]
    return cases


def limb_operands(L, P, rng, n):
    """values below 2^(2P) whose L-bit limbs are all among the limbs mont_small estimates one below (there are few below 2^16: the
    first is 46,183)"""
    pool = [v for v in U.mont_small_one_below() if v < 1 << L]
    assert pool
    k = (2 * P) // L
    return [sum(rng.choice(pool) << (L * i) for i in range(k)) for _ in range(n)], set(pool)


def count_limbs(O, c, pool):
    return sum(1 for v in O.fr_to_ints(c.lookup()) if v in pool)


# ---- the tests -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("op", ["qdiv", "qmod"])
@pytest.mark.parametrize("P,L", PL)
def test_division_reaches_the_clamp_and_the_second_add_back(api, O, op, P, L):
    cases = clamp_cases(op, P)
    ok, bad, c = run_and_compare(api, O, op, cases, P, L)
    n = branch_counts(op, ok, P)
    print(op, P, "accepted", len(ok), "refused", len(bad), n)
    assert n["clamped"] >= 20 and n["fix2"] >= 20, n


@pytest.mark.parametrize("op", UNARY + BINARY)
@pytest.mark.parametrize("P,L", PL)
def test_every_operation_at_the_ends_of_its_domain(api, O, op, P, L):
    cases = edge_cases(O, op, P, L)
    ok, bad, c = run_and_compare(api, O, op, cases, P, L)
    print(op, P, "accepted", len(ok), "refused", len(bad))
    assert 3 * len(bad) <= len(cases), (op, len(bad), len(cases))


@pytest.mark.parametrize("L", [16, 17, 18, 19, 20])
def test_lookup_widths_where_mont_small_subtracts(api, O, L):
    """L = 16 .. 20 (every other test uses L <= 15, where the final subtraction of mont_small is dead): qmul, qdiv, is_neg and one
    distance per metric at dim = 5, on operands whose limbs are among the one-below limbs"""
    P = 48
    rng = random.Random(1000 + L)
    vals, pool = limb_operands(L, P, rng, 12)
    one = 1 << P
    total = 0
    for op, cases in (("is_neg", [(v, None) for v in vals] + [((R - v) % R, None) for v in vals[:3]]),
                      ("qmul", [(v, one) for v in vals] + [(v, R - one) for v in vals[:3]]),
                      ("qdiv", [(v, one) for v in vals] + [(v, 3 * one) for v in vals[:3]])):
        ok, bad, c = run_and_compare(api, O, op, cases, P, L)
        assert not bad and c.check_gates(L) == 0
        k = count_limbs(O, c, pool)
        print(L, op, "one-below limbs in the lookup stream:", k)
        assert k > 0
        total += k
    for metric in ("euclidean", "cosine", "manhattan", "hamming"):
        b = [one] * 5
        a = [(v + one) % R for v in vals[:5]]              # a - b has the chosen limbs
        qa, qb = O.fr_from_ints(a)[None], O.fr_from_ints(b)[None]
        c = O.Ctx(store=True, keygen=True)
        want = c.distance(metric, qa[0], qb[0], P=P, L=L)
        assert c.err == 0
        got = api.wit_distance(metric, qa, qb, P=P, L=L, selectors=True)
        assert np.array_equal(got["result"][0], want), metric
        assert_streams(got, c)
        total += count_limbs(O, c, pool)
    print(L, "one-below limbs in all lookup streams:", total)
    assert total >= 50
