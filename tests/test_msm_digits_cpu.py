"""The MSM sort's digit code — fold_scalar, emit_digits, the scaled-short classification, the 8-byte record and emit_digits_short of
halo2_vectordb_amd/csrc/msm_digits.hpp, what k_msm_sort decomposes its scalars with — on the host, through
`tools/msm_digits_probe.hip --host`, held with no tolerance to Python integers (tests/msm_digits_model.py) for window sizes 2, 5, 8, 11
and 14: the digit list of the full 256-bit walk, the classification, the record, and the digit list decoded from the record, which has
to be the full walk's.

Scalars: 0 and 1; a 2^e for every e in 0..253 that stays below r and a in {1, 3, 2^(c-1), 2^(c-1) + 1, 2^c - 1, 2^c, 2^31, 2^32 - 1,
2^32, 2^32 + 1}; all-ones mantissas at and beside every window boundary (the sign carry runs through every window of s' and out of its
top); all of these negated; (r - 1) / 2 and (r - 1) / 2 + 1, the two sides of the fold; r - 1; random full-width and random sparse values;
short values whose first window plus the windows the walk gives s' reaches the number of windows exactly, and would pass it."""
import random

import pytest

import l9_model as L
import msm_digits_model as M


def gen(rng):
    blocks, fams = [], {}
    for op, c in enumerate(M.CS):
        fam = M.families(c, rng)
        fams[c] = fam
        cases = [(name, L.words8(v)) for name, vs in fam.items() for v in vs]
        blocks.append(L.Block(op, c, cases, nin=[8] * len(M.CS), names=[f"c={x}" for x in M.CS]))
    return blocks, fams


@pytest.fixture(scope="module")
def host_run(tmp_path_factory):
    d = tmp_path_factory.mktemp("msm_digits")
    exe = L.compile_probe(d, "msm_digits_probe")
    blocks, fams = gen(random.Random(20261020))
    names = [f"c={x}" for x in M.CS]
    results = L.run_probe(exe, "--host", blocks, d, 600, [M.nout(c) for c in M.CS], names, M.MAGIC)
    return {b.mod: (b, r, fams[b.mod]) for b, r in zip(blocks, results)}


@pytest.mark.parametrize("c", M.CS)
def test_digits_classification_and_record_against_integers(host_run, c):
    b, res, fam = host_run[c]
    W = M.windows(c)
    kinds = {M.ZERO: 0, M.SHORT: 0, M.LONG: 0}
    scaled = exact_w = past_w = carry_out = 0
    for (tag, w), got in zip(b.cases, res):
        v = L.from_words(w)
        want = M.expect(v, c)
        assert got == want, (c, tag, hex(v), got, want)
        kind, j0, nbp, sp = M.classify(v, c)
        kinds[kind] += 1
        if kind == M.SHORT:
            # the record's decoded list is the full walk's (both already equal the model's: stated on its own, it is the point)
            assert got[W + 7:] == got[:W + 1], (c, tag, hex(v))
            scaled += j0 > 0 and M.fold(v)[0].bit_length() > M.short_bits(c)
            exact_w += j0 + nbp // c + 2 == W
            past_w += j0 + nbp // c + 2 > W
            top = M.digits(v, c)[-1][0]
            carry_out += top - j0 == -(-nbp // c)     # a digit one window above the top of s'
    print("c", c, "cases", len(res), "zero / short / long", kinds, "short only by scaling", scaled, "reach W", exact_w, "pass W", past_w,
          "carry out of the top", carry_out)
    assert kinds[M.ZERO] >= 1 and kinds[M.LONG] > 1000 and scaled > 1000 and exact_w > 0 and past_w > 0 and carry_out > 100


@pytest.mark.parametrize("c", M.CS)
def test_families_hold_what_they_promise(host_run, c):
    _, _, fam = host_run[c]
    assert fam["edge"] == [0, 1, M.HALF, M.HALF + 1, M.R - 1]
    pw = set(fam["pow"])
    for a in M.mantissas(c):
        es = [e for e in range(254) if a << e < M.R]
        assert es and all(a << e in pw and M.R - (a << e) in pw for e in es), a
    assert (1 << 253) in pw
    assert len(fam["random"]) >= 2000 and len(fam["sparse"]) >= 2000
    assert any(v.bit_length() > 250 for v in fam["random"])
    # what is short today stays short: j0 = 0 is today's rule
    for vs in fam.values():
        for v in vs:
            s, _ = M.fold(v)
            if 0 < s.bit_length() <= M.short_bits(c):
                assert M.classify(v, c)[0] == M.SHORT
