"""The device (inline-asm) forms of the nine-limb field arithmetic and the MSM accumulator's mixed addition / doubling, through
`tools/l9_probe.hip --device`: every output equals the Python-integer model of tests/l9_model.py, and — for every op that also has a
host form — the host output byte for byte (field.hpp's "bit-identical", for all five asm cores and both fields).  In-domain cases only.

Each test runs the probe on the GPU as ONE child process under a time limit; a non-zero or signal exit fails the test with the
child's stderr and nothing is retried."""
import pytest

import l9_model as L

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    return L.compile_probe(tmp_path_factory.mktemp("l9_probe"))


@pytest.fixture(scope="module")
def device_blocks():
    blocks = L.build_blocks(host=False)
    assert not any(t.startswith("ood:") for b in blocks for t, _ in b.cases)
    return blocks


def run_both(probe, blocks, tmp_path):
    """device == model for every block, device == host for the blocks that have a host form"""
    assert blocks
    dev = L.run_probe(probe, "--device", blocks, tmp_path, timeout=120)
    n = 0
    for b, res in zip(blocks, dev):
        n += L.check_block(b, res)
    assert n == sum(len(b.cases) for b in blocks)
    both = [i for i, b in enumerate(blocks) if b.op not in L.DEVICE_ONLY]
    host = L.run_probe(probe, "--host", [blocks[i] for i in both], tmp_path, timeout=600)
    for i, res in zip(both, host):
        assert res == dev[i], (L.NAMES[blocks[i].op], blocks[i].mod)
    return n


CORES = (L.MUL, L.MUL2, L.SQR, L.SHOUP, L.FROM_MONT, L.MONT_MUL)


def test_product_cores_device_host_model(probe, device_blocks, tmp_path):
    """mont_core29, mont_core29_2, mont_sqr_core29, shoup_core29, from_mont's reduction-only path, mont_mul: Fr and Fq"""
    blocks = [b for b in device_blocks if b.op in CORES]
    assert sorted((b.op, b.mod) for b in blocks) == sorted((op, m) for op in CORES for m in (0, 1))
    for b in blocks:
        have = b.classes()
        assert all(have.get(c, 0) > 0 for c in (("corner", "value", "random") if b.op <= L.SHOUP else ("edge", "random"))), (L.NAMES[b.op], have)
    print("cases:", run_both(probe, blocks, tmp_path))


def test_limb_ops_device_host_model(probe, device_blocks, tmp_path):
    """split / pack / renorm / carry / add / sub / neg / canon / is_zero_mod, one k_gate_eval step fed back up to 64 times, and
    l9_canon_wide (Fr, device only)"""
    ops = (L.SPLIT, L.SPLIT32, L.PACK, L.RENORM, L.CARRY, L.ADD, L.SUB, L.NEG, L.CANON, L.IS_ZERO, L.GATE)
    blocks = [b for b in device_blocks if b.op in ops or b.op == L.CANON_WIDE]
    assert sorted((b.op, b.mod) for b in blocks) == sorted([(op, m) for op in ops for m in (0, 1)] + [(L.CANON_WIDE, 0)])
    for b in blocks:
        if b.op in (L.SUB, L.NEG):
            have = b.classes()
            assert all(have.get(c, 0) > 0 for c in ("edge-in", "value", "random", "site")), have
    cw = next(b for b in blocks if b.op == L.CANON_WIDE)
    have = cw.classes()
    assert all(have.get(c, 0) > 0 for c in ("corner", "value", "random")), have
    # the quotient estimate is exact or one too small, and both occur among the cases (reachable: top is the value's true top limb
    # or one less, and V / r - top / (r_8 + 1) < 1 for V < 2^259, so the two floors differ by at most 1)
    assert {L.canon_wide_estimate(w)[1] for _, w in cw.cases} == {0, 1}
    print("cases:", run_both(probe, blocks, tmp_path))


def test_msm_accumulator_device_model(probe, device_blocks, tmp_path):
    """madd_l9 / mdbl_l9 against the group law over Python integers: accumulators at x + j q for every j AccL9's bounds allow, both
    signs, same / opposite point, from the identity, and 64-step chains whose every intermediate accumulator is checked against the
    stated bounds (x < 7.5 q, y < 3.6 q, zz, zzz < 1.1 q, exactly normalised): the bounds are closed under the operation"""
    blocks = [b for b in device_blocks if b.op in (L.MADD, L.MDBL, L.MADD_CHAIN)]
    assert [b.op for b in blocks] == [L.MADD, L.MDBL, L.MADD_CHAIN]
    have = blocks[0].classes()
    assert all(have.get(c, 0) > 0 for c in ("plus-jq", "same-point", "opposite-point", "from-identity", "random")), have
    have = blocks[1].classes()
    assert all(have.get(c, 0) > 0 for c in ("point", "point-negated", "two-torsion")), have
    assert len(blocks[2].cases) >= 16
    dev = L.run_probe(probe, "--device", blocks, tmp_path, timeout=120)
    n = sum(L.check_block(b, res) for b, res in zip(blocks, dev))
    assert n == sum(len(b.cases) for b in blocks)
    # the chains did walk the exceptional paths
    idents = sum(r[37 * i + 36] for r in dev[2] for i in range(L.CHAIN))
    assert idents > 0
    print("cases:", n)
