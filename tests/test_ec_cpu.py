"""The layer between the product cores and the kernels held to Python integers, function by function: the host (C++) forms of the
256-bit field helpers of halo2_vectordb_amd/csrc/field.hpp (mod_add, mod_sub, mod_neg, mod_dbl, mont_mul with k_from_wide's wide first
operand, to_mont, mont_pow, mont_inv, the shifts and bit helpers, the carry and borrow of u256_add / u256_sub) and of the u256 XYZZ group
law of ec.hpp (xyzz_add, xyzz_add_mixed, xyzz_double, xyzz_double_affine, xyzz_from_affine, xyzz_to_affine, xyzz_neg's user xyzz_mul),
through `tools/ec_probe.hip --host`.  The model and the case generator are tests/ec_model.py; tests/test_gpu_ec.py runs the device
compilation on the same cases.

The group law's exceptional branches are cases of their own: one point in two (ZZ, ZZZ) scalings (the doubling branch), opposite points
(the identity), the identity on either side, and 64-step chains over four points and their negatives whose every intermediate
accumulator is checked and which are asserted to have walked both branches."""
import pytest

import ec_model as E


@pytest.fixture(scope="module")
def host_run(tmp_path_factory):
    d = tmp_path_factory.mktemp("ec")
    exe = E.compile_probe(d)
    blocks = E.build_blocks()
    results = E.run_probe(exe, "--host", blocks, d, timeout=600)
    return {(b.op, b.mod): (b, r) for b, r in zip(blocks, results)}


def check(host_run, ops, mods):
    n = 0
    for op in ops:
        for mod in mods:
            b, res = host_run[(op, mod)]
            E.check_classes(b)
            assert E.check_block(b, res) == len(b.cases) == sum(b.classes().values())
            n += len(b.cases)
    print("cases:", n)


def test_every_op_has_its_blocks(host_run):
    want = [(op, m) for op in E.FIELD_OPS for m in (0, 1)] + [(E.FROM_WIDE, 0)] + [(op, 0) for op in E.U256_OPS]
    want += [(op, 1) for op in E.GROUP_OPS + (E.XCHAIN,)]
    assert sorted(host_run) == sorted(want) and len(want) == len(E.build_blocks())
    print("blocks:", len(want), "cases:", sum(len(b.cases) for b in E.build_blocks()))


MODS = pytest.mark.parametrize("mod", [0, 1], ids=["Fr", "Fq"])


@MODS
def test_mod_add_sub_neg_dbl(host_run, mod):
    check(host_run, (E.MOD_ADD, E.MOD_SUB, E.MOD_NEG, E.MOD_DBL), (mod,))


@MODS
def test_mont_mul_wide_first_operand_and_to_mont(host_run, mod):
    """a up to 2^256 - 1 (what k_from_wide feeds to_mont): the product is still a b 2^-256 mod p, canonical"""
    check(host_run, (E.MONT_MUL, E.TO_MONT), (mod,))


def test_from_wide(host_run):
    """fr_add(to_mont(lo), to_mont(to_mont(hi))) = (lo + 2^256 hi) mod r in Montgomery form, at the multiples of r and the word edges"""
    check(host_run, (E.FROM_WIDE,), (0,))


@MODS
def test_mont_pow_every_exponent_length(host_run, mod):
    check(host_run, (E.MONT_POW,), (mod,))


@MODS
def test_mont_inv(host_run, mod):
    check(host_run, (E.MONT_INV,), (mod,))
    b, res = host_run[(E.MONT_INV, mod)]
    assert [r for (t, _), r in zip(b.cases, res) if t == "zero"] == [[0] * 8]


def test_shifts_and_bit_helpers(host_run):
    check(host_run, (E.SHR, E.SHL, E.SHR_SMALL, E.LOW_BITS, E.BITS, E.BIT, E.EXTRACT), (0,))


def test_compare_carry_borrow(host_run):
    check(host_run, (E.CMP,), (0,))
    b, res = host_run[(E.CMP, 0)]
    wrap = [r for (t, _), r in zip(b.cases, res) if t == "wrap"]
    assert [(r[10], r[19]) for r in wrap] == [(1, 0), (0, 1)]      # 2^256 - 1 + 1 carries out, 0 - 1 borrows


def test_group_law(host_run):
    check(host_run, E.GROUP_OPS, (1,))


def test_chains_walk_the_doubling_and_cancelling_branches(host_run):
    check(host_run, (E.XCHAIN,), (1,))
    dbl, ident = E.chain_branches(*host_run[(E.XCHAIN, 1)])
    print("doublings:", dbl, "cancellations:", ident)
    assert dbl > 0 and ident > 0
