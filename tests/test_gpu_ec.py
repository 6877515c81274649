"""The device compilation of the 256-bit field helpers of field.hpp and of the u256 XYZZ group law of ec.hpp — the functions under the
verifier's MSM, the group DFT of a params file, k_g1_sum, the SRS kernels, the bucket reduction of the prover's MSM and k_from_wide —
through `tools/ec_probe.hip --device`: every output equals the Python-integer model of tests/ec_model.py, and the host output byte for
byte (both run the same formulas).  Every case is inside the domain its function states (shift counts, u256_bit indices, operand ranges:
the header of the probe), on the cases tests/test_ec_cpu.py holds the host forms to.

Each test runs the probe on the GPU as ONE child process under a time limit; a non-zero or signal exit fails the test with the child's
stderr and nothing is retried."""
import pytest

import ec_model as E

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    return E.compile_probe(tmp_path_factory.mktemp("ec_probe"))


@pytest.fixture(scope="module")
def host_results(probe, tmp_path_factory):
    """the host forms on every block, once (no GPU involved): what the device results are compared with byte for byte"""
    blocks = E.build_blocks()
    res = E.run_probe(probe, "--host", blocks, tmp_path_factory.mktemp("ec_host"), timeout=600)
    return {(b.op, b.mod): r for b, r in zip(blocks, res)}


def run_both(probe, host_results, keys, tmp_path):
    """device == model and device == host for the blocks `keys` names; returns (blocks, device results)"""
    blocks = [b for b in E.build_blocks() if (b.op, b.mod) in keys]
    assert sorted((b.op, b.mod) for b in blocks) == sorted(keys)
    for b in blocks:
        E.check_classes(b)
    dev = E.run_probe(probe, "--device", blocks, tmp_path, timeout=120)
    n = 0
    for b, res in zip(blocks, dev):
        n += E.check_block(b, res)
        assert res == host_results[(b.op, b.mod)], (E.NAMES[b.op], b.mod)
    assert n == sum(len(b.cases) for b in blocks)
    print("cases:", n)
    return blocks, dev


def test_field_helpers_device_host_model(probe, host_results, tmp_path):
    """mod_add / sub / neg / dbl, mont_mul with a first operand up to 2^256 - 1, to_mont and from_mont, mont_pow at every exponent
    length (u256_shl by every amount), mont_inv: Fr and Fq; k_from_wide's composition over Fr; the shifts, masks, bit counts, comparisons
    and the carry / borrow out"""
    keys = [(op, m) for op in E.FIELD_OPS for m in (0, 1)] + [(E.FROM_WIDE, 0)] + [(op, 0) for op in E.U256_OPS]
    run_both(probe, host_results, keys, tmp_path)


def test_group_law_device_host_model(probe, host_results, tmp_path):
    """xyzz_add, xyzz_add_mixed, xyzz_double, xyzz_double_affine, xyzz_from_affine, xyzz_to_affine, xyzz_mul: one point in two scalings,
    opposite points, the identity on either side, y = 0"""
    run_both(probe, host_results, [(op, 1) for op in E.GROUP_OPS], tmp_path)


def test_chains_device_host_model(probe, host_results, tmp_path):
    """16 chains of 64 mixed additions over four points and their negatives, every intermediate accumulator against the model; the
    device results themselves show that the doubling and the cancelling branch were walked"""
    blocks, dev = run_both(probe, host_results, [(E.XCHAIN, 1)], tmp_path)
    dbl, ident = E.chain_branches(blocks[0], dev[0])
    print("doublings:", dbl, "cancellations:", ident)
    assert dbl > 0 and ident > 0
