"""The 256-bit integer layer under every fixed-point gadget (the u256_* shifts, masks and bit counts of halo2_vectordb_amd/csrc/field.hpp,
Gadgets::divmod_u256 and Gadgets::mont_small of gadgets.hpp) held to Python integers at its rare branches: the host compilation,
through `tools/u256_probe.hip --host`.  The model, the branch classifier and the case generator are tests/u256_model.py;
tests/test_gpu_u256.py runs the device compilation on the same cases.

What the cases reach (asserted below on the case list itself, with the classifier):
  * divmod_u256: the clamp of the quotient estimate (the remainder's top word equals the divisor's), the second add-back, both in one
    division, every number of skipped digits, every early exit, the dividends x << P the chip produces; and the 6,912 operand pairs
    of tools/divtest.hip, whose generator is restated in Python and compared with that program's own output here.
  * mont_small: all 4,566 limbs below 2^24 whose quotient estimate is one below (the first is 46,183: the final conditional
    subtraction is dead for every lookup width up to 15), with both neighbours, and every limb below 2^16.
  * A clamped digit never takes the second add-back: with the divisor normalised the clamped estimate 2^32 - 1 exceeds the true digit
    by less than 2^32 delta / bn + 1 < 2 for a remainder bn - delta, delta < 2^224.  "Both" below means two digits of one division."""
import os
import re
import subprocess

import pytest

import l9_model as L
import u256_model as U

CSRC = os.path.join(L.ROOT, "halo2_vectordb_amd", "csrc")


@pytest.fixture(scope="module")
def host_run(tmp_path_factory):
    d = tmp_path_factory.mktemp("u256")
    exe = U.compile_probe(d)
    blocks = U.build_blocks()
    results = U.run_probe(exe, "--host", blocks, d, timeout=600)
    return {b.op: (b, r) for b, r in zip(blocks, results)}


def say(capsys, *args, **kw):
    """case counts go to the terminal even when the run captures output"""
    with capsys.disabled():
        print(*args, **kw)


def check(host_run, capsys, op, classes):
    b, res = host_run[op]
    have = b.classes()
    say(capsys, "\n ", U.NAMES[op], len(b.cases), have, end="")
    for c in classes:
        assert have.get(c, 0) > 0, (U.NAMES[op], c, have)
    assert U.check_block(b, res) == len(b.cases) == sum(have.values())
    return b


def test_shifts(host_run, capsys):
    """every s in 0 .. 255 (1 .. 31 for u256_shr_small) on all-ones, every single bit, alternating words, random values"""
    for op, amounts in ((U.SHR, range(256)), (U.SHL, range(256)), (U.SHR_SMALL, range(1, 32))):
        b = check(host_run, capsys, op, ["ones", "bit", "alternating", "random"])
        assert {w[8] for _, w in b.cases} == set(amounts)
        for s in amounts:
            assert sum(1 for t, w in b.cases if w[8] == s and t == "bit") == 256


def test_masks_and_bit_counts(host_run, capsys):
    b = check(host_run, capsys, U.LOW_BITS, ["ones", "bit", "alternating", "random"])
    assert {w[8] for _, w in b.cases} == set(range(257))
    b = check(host_run, capsys, U.EXTRACT, ["ones", "bit", "alternating", "random"])
    assert {(w[8], w[9]) for _, w in b.cases} == {(p, n) for p in (0, 1, 31, 32, 33, 223, 224, 225, 254, 255, 256, 300) for n in (0, 1, 31, 32)}
    b = check(host_run, capsys, U.BITS, ["zero", "bit", "ones", "random"])
    vals = {U.fw(w) for _, w in b.cases}
    assert 0 in vals and all(1 << i in vals and (1 << (i + 1)) - 1 in vals for i in range(256))


def test_add_sub_carry_out(host_run, capsys):
    for op in (U.ADD, U.SUB):
        b, res = host_run[op]
        check(host_run, capsys, op, ["edge", "random", "carry-chain"])
        assert {r[8] for r in res} == {0, 1}          # both values of the carry / borrow out occur


def test_divtest_cases_are_restated_exactly(tmp_path):
    """the generator of tools/divtest.hip in Python gives the pairs that program prints, in order"""
    exe = str(tmp_path / "divtest")
    subprocess.run([L.HIPCC, "-O2", "-std=c++17", "--offload-arch=gfx950", "-Wno-unused-function", "-o", exe, os.path.join(L.ROOT, "tools", "divtest.hip")],
                   check=True, capture_output=True, text=True)
    out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.splitlines()
    printed = [tuple(int(x, 16) for x in line.split()[:2]) for line in out]
    assert len(printed) == 6912 and printed == U.divtest_cases()


def divmod_coverage(pairs):
    """-> counts over (tag, a, b): divisions with a clamped digit, a second add-back, both; per dividend shape; skipped digits seen"""
    n = dict(clamped=0, fix2=0, both=0, early=0, fix1=0)
    shape = {}
    skipped = set()
    for tag, a, b in pairs:
        c = U.classify(a, b)
        if c is None:
            n["early"] += 1
            continue
        skipped.add(c["skipped"])
        n["clamped"] += c["clamped"] > 0
        n["fix1"] += c["fix1"] > 0
        n["fix2"] += c["fix2"] > 0
        n["both"] += c["clamped"] > 0 and c["fix2"] > 0
        for P in (32, 48):
            if tag.startswith("xshl%d" % P):
                assert a % (1 << P) == 0 and a >> P < 1 << (2 * P) and b < 1 << (2 * P), tag
                k = shape.setdefault(P, dict(clamped=0, fix2=0))
                k["clamped"] += c["clamped"] > 0
                k["fix2"] += c["fix2"] > 0
    return n, shape, skipped


def test_divmod_u256(host_run, capsys):
    b = check(host_run, capsys, U.DIVMOD, ["divtest", "early", "shift0", "qb+rem", "clamp", "xshl32-clamp", "xshl48-clamp", "xshl32-fix2", "xshl48-fix2"])
    pairs = U.divmod_pairs()
    assert [(a, d) for t, a, d in pairs if t == "divtest"] == [p for p in U.divtest_cases() if p[1]]
    n, shape, skipped = divmod_coverage(pairs)
    say(capsys, "\n  divmod_u256 branches:", n, "x << P:", shape, "skipped digits:", sorted(skipped), end="")
    assert n["clamped"] >= 200 and n["fix2"] >= 50 and n["both"] >= 10 and n["early"] > 0 and n["fix1"] > 0
    for P in (32, 48):
        assert shape[P]["clamped"] >= 20 and shape[P]["fix2"] >= 20, (P, shape)
    assert skipped >= set(range(8))
    # the early exits by name
    ab = {(a, d) for _, a, d in pairs}
    assert any(a < d for a, d in ab) and any(a == 0 for a, d in ab) and any(d == 1 and a > 1 for a, d in ab) and any(a == d for a, d in ab)
    assert any(d == 1 << 255 for a, d in ab) and any(d == U.U256 - 1 for a, d in ab)


def test_divtest_alone_never_clamps():
    """why the cases above are needed: the 6,912 pairs of tools/divtest.hip (tests/test_divmod_cpu.py) reach no clamped digit"""
    n, _, _ = divmod_coverage([("divtest", a, b) for a, b in U.divtest_cases() if b])
    assert n["clamped"] == 0 and n["fix2"] > 0


def test_mont_small(host_run, capsys):
    below = U.mont_small_one_below()
    assert len(below) == 4566 and below[0] == 46183
    b = check(host_run, capsys, U.MONT_SMALL, ["all16", "one-below", "neighbour", "tight", "edge", "width"])
    vs = {w[0] for _, w in b.cases}
    assert vs >= set(range(1 << 16)) and (1 << 24) - 1 in vs
    assert all(v in vs and v - 1 in vs and v + 1 in vs for v in below)
    assert all((1 << n) - 1 in vs and (1 << n) - 2 in vs for n in range(2, 21))
    # the constant in the source is the one its comment defines, floor(c 2^32 / r): one less would still give right answers (more
    # estimates one below), one more gives estimates above, which the single conditional subtraction cannot mend
    src = open(os.path.join(CSRC, "gadgets.hpp")).read()
    mu, = re.findall(r"constexpr uint32_t MU = (0x[0-9a-fA-F]+)u;", src)
    assert int(mu, 16) == U.MU == (U.C256 << 32) // U.R


def test_mont_round_trip_and_inverse(host_run, capsys):
    check(host_run, capsys, U.MONT_ROUND, ["edge", "random"])
    b = check(host_run, capsys, U.MONT_INV, ["edge", "random"])
    assert b.cases[0][1] == U.w8(0)               # 0 maps to 0 (the model asserts it)
