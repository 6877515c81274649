"""The device compilation of the 256-bit integer layer under the witness kernels (u256_* of field.hpp, Gadgets::divmod_u256 with its
software 64-bit division and conditional-move word shifts, Gadgets::mont_small, to_mont / from_mont / mont_inv over Fr), through
`tools/u256_probe.hip --device`: every output equals the Python-integer model of tests/u256_model.py and the host output byte for byte,
on the cases of tests/test_u256_cpu.py (which asserts what they cover: clamped quotient digits, second add-backs, the 4,566 limbs
whose Montgomery estimate is one below, every shift amount).

The probe runs on the GPU as ONE child process under a time limit; a non-zero or signal exit fails the test with the child's stderr
and nothing is retried."""
import pytest

import u256_model as U

pytestmark = pytest.mark.gpu


def test_integer_layer_device_host_model(tmp_path):
    exe = U.compile_probe(tmp_path)
    blocks = U.build_blocks()
    assert sorted(b.op for b in blocks) == list(range(len(U.NAMES)))
    dev = U.run_probe(exe, "--device", blocks, tmp_path, timeout=120)
    n = 0
    for b, res in zip(blocks, dev):
        n += U.check_block(b, res)
        print(U.NAMES[b.op], len(b.cases), b.classes())
    assert n == sum(len(b.cases) for b in blocks)
    host = U.run_probe(exe, "--host", blocks, tmp_path, timeout=600)
    for b, h, d in zip(blocks, host, dev):
        assert h == d, U.NAMES[b.op]
    print("cases:", n)
