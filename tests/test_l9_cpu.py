"""The nine-limb lazy field arithmetic (halo2_vectordb_amd/csrc/limb9.hpp on the product cores of field.hpp) held to Python integers
at its stated bounds, primitive by primitive: the host (C++) forms, through `tools/l9_probe.hip --host`.  The model and the case
generator are tests/l9_model.py; tests/test_gpu_l9.py runs the device (inline-asm) forms on the same generator's cases.

What the cases establish about the domains (and what the comments in limb9.hpp / ec_l9.hpp / ntt.hip now say):
  * l9_sub / l9_neg with the offset K p of l9_offset_limbs: exact for every subtrahend with limbs 0..7 below 2^29 and top limb at most
    c_8 = floor(K p / 2^232) - 1, i.e. value below (K - 2^-22) p — not only "below (K - 1) p".  One more in the top limb wraps
    (test_sub_domain_edge).  madd_l9's subtrahends below 7.5 q with the 8 q offset are inside.
  * a subtrahend as l9_renorm leaves it (limbs of 2^29 + 7) is inside the domain of the 9 r, 14 r, 34 r and 8 q offsets and outside
    that of 2 r (limb 0 of 2 r is 2) — test_sub_renormalised_subtrahend.  The NTT's 14 r is safe either way; ntt_dev nevertheless
    refuses a carry schedule that renormalises in front of the step at stage 0, which subtracts its operands as loaded.
  * l9_canon_wide's quotient estimate is 0 or 1 below the true quotient, never more (tests/test_gpu_l9.py asserts the set seen)."""
import os
import subprocess
import sys

import pytest

import l9_model as L

CSRC = os.path.join(L.ROOT, "halo2_vectordb_amd", "csrc")


@pytest.fixture(scope="module")
def host_run(tmp_path_factory):
    d = tmp_path_factory.mktemp("l9")
    exe = L.compile_probe(d)
    blocks = L.build_blocks(host=True)
    results = L.run_probe(exe, "--host", blocks, d, timeout=600)
    return {(b.op, b.mod): (b, r) for b, r in zip(blocks, results)}


def check(host_run, op, mod, classes):
    b, res = host_run[(op, mod)]
    have = b.classes()
    for c in classes:
        assert have.get(c, 0) > 0, (L.NAMES[op], c, have)
    assert L.check_block(b, res) == len(b.cases) == sum(have.values())


MODS = pytest.mark.parametrize("mod", [0, 1], ids=["Fr", "Fq"])


@MODS
def test_mont_core29(host_run, mod):
    check(host_run, L.MUL, mod, ["corner", "value", "random"])


@MODS
def test_mont_core29_2(host_run, mod):
    check(host_run, L.MUL2, mod, ["corner", "value", "random"])


@MODS
def test_mont_sqr_core29(host_run, mod):
    check(host_run, L.SQR, mod, ["corner", "value", "random"])


@MODS
def test_shoup_core29(host_run, mod):
    check(host_run, L.SHOUP, mod, ["corner", "value", "random"])


def test_shoup_pair29(host_run):
    check(host_run, L.SHOUP_PAIR, 0, ["edge", "random"])


@MODS
def test_from_mont_and_mont_mul(host_run, mod):
    check(host_run, L.FROM_MONT, mod, ["edge", "random"])
    check(host_run, L.MONT_MUL, mod, ["edge", "random"])


@MODS
def test_split_pack(host_run, mod):
    for op in (L.SPLIT, L.SPLIT32, L.PACK):
        check(host_run, op, mod, ["edge", "random"])


@MODS
def test_renorm_carry_add(host_run, mod):
    for op in (L.RENORM, L.CARRY, L.ADD):
        check(host_run, op, mod, ["corner", "value", "random"])


@MODS
def test_canon_and_is_zero(host_run, mod):
    check(host_run, L.CANON, mod, ["edge", "random"])
    check(host_run, L.IS_ZERO, mod, ["edge", "random"])
    b, res = host_run[(L.IS_ZERO, mod)]
    assert sum(r[0] for r in res) >= 2   # both representations of zero occur


@MODS
def test_offset_limbs(host_run, mod):
    b, res = host_run[(L.OFFSET, mod)]
    assert [w[0] for _, w in b.cases] == list(L.OFFSETS_IN_USE[mod])
    check(host_run, L.OFFSET, mod, [f"K={K}" for K in L.OFFSETS_IN_USE[mod]])


@MODS
def test_sub_domain_edge(host_run, mod):
    """t_8 == c_8 is exact, t_8 == c_8 + 1 wraps (and so does c_k + 1 in any single limb): the edge is where the model says.  The value
    (K - 1) p + anything below p - 2^232 is inside: the domain is wider than "below (K - 1) p"."""
    ks = L.OFFSETS_IN_USE[mod]
    classes = [f"{c}" for c in ("edge-in", "edge-in-limb", "ood:edge-out", "ood:edge-out-limb", "value", "random", "site")]
    check(host_run, L.SUB, mod, classes)
    check(host_run, L.NEG, mod, ["edge-in", "ood:edge-out", "value", "random", "site"])
    b, res = host_run[(L.SUB, mod)]
    for K in ks:
        tags = [t for t, _ in b.cases if t.endswith(f"/K={K}")]
        assert any(t.startswith("edge-in/") for t in tags) and any(t.startswith("ood:edge-out/") for t in tags), K
    # every use site's documented subtrahend bound lies inside the domain (the model asserts "no wrap" for a "site" case)
    n_sites = sum(1 for s in L.SUB_SITES if s[0] == mod)
    assert sum(1 for t, _ in b.cases if t.startswith("site/")) == 2 * n_sites > 0
    # madd_l9's two lines: 7.5 q against the 8 q offset, beyond the "(K - 1) p" = 7 q the header used to state
    if mod == 1:
        c8 = L.offset_limbs(8, L.Q)
        assert (15 * L.Q // 2) >> 232 <= c8[8] and 7 * L.Q < 15 * L.Q // 2


@MODS
def test_sub_renormalised_subtrahend(host_run, mod):
    """limbs of 2^29 + 7 (l9_renorm's output) subtracted from a minuend limb of 0: which offsets cover it"""
    b, res = host_run[(L.SUB, mod)]
    wraps = {K: L.renormalised_wrap_limbs(mod, K) for K in L.OFFSETS_IN_USE[mod]}
    assert wraps == ({2: [0], 9: [], 14: [], 34: []} if mod == 0 else {2: [], 8: []})
    for K, w in wraps.items():
        tag = f"ood:renormalised-out/K={K}" if w else f"renormalised-in/K={K}"
        hits = [(c, r) for (t, c), r in zip(b.cases, res) if t == tag]
        assert len(hits) == 1
        (c, r), = hits
        exact = [c[18 + k] - c[9 + k] for k in range(9)]
        assert [k for k in range(9) if exact[k] < 0] == w and r == [x % L.U32 for x in exact]


@MODS
def test_gate_step_invariant(host_run, mod):
    """k_gate_eval's accumulator stays below 2 r at the worst operands its comment allows, fed back 64 times (the model asserts the
    bound after every step and that l9_canon of the result is the field value)"""
    check(host_run, L.GATE, mod, ["worst", "random"])
    b, _ = host_run[(L.GATE, mod)]
    assert max(w[66] for t, w in b.cases if t == "worst") == 64


def test_device_only_models_stand():
    """l9_canon_wide, madd_l9 and mdbl_l9 are device functions: their cases are generated and the model's own preconditions and
    contracts are asserted here, the comparison happens in tests/test_gpu_l9.py"""
    blocks = [b for b in L.build_blocks(host=False) if b.op in L.DEVICE_ONLY]
    assert sorted(b.op for b in blocks) == sorted(L.DEVICE_ONLY)
    for b in blocks:
        for tag, w in b.cases:
            if b.op == L.CANON_WIDE:
                L.expect(b.op, b.mod, tag, w)
            else:
                pts = L.expect_ec(b.op, tag, w)
                assert all(p is None or (p[0] ** 3 + 3 - p[1] ** 2) % L.Q == 0 for p in pts)
    cw = next(b for b in blocks if b.op == L.CANON_WIDE)
    assert {L.canon_wide_estimate(w)[1] for _, w in cw.cases} == {0, 1}


def test_generated_cores_match_committed(tmp_path):
    """gen_core29.py writes into the current directory: what it writes is byte for byte what is checked in"""
    subprocess.run([sys.executable, os.path.join(CSRC, "gen_core29.py")], cwd=str(tmp_path), check=True, capture_output=True)
    names = ["core29_mul.inc", "core29_mul2.inc", "core29_sqr.inc", "core29_shoup.inc", "core29_redc.inc"]
    assert sorted(os.listdir(str(tmp_path))) == sorted(names)
    for n in names:
        assert open(os.path.join(str(tmp_path), n), "rb").read() == open(os.path.join(CSRC, n), "rb").read(), n
