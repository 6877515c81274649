"""bench.py: a plain run prints the headline line and nothing that takes runs of its own; --full adds the whole proof, the
field-product microbenchmark and the CPU baseline to the same line."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(*extra):
    res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--small", *extra],
                         capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-2000:]
    return json.loads(res.stdout.strip().splitlines()[-1])


@pytest.mark.gpu
def test_plain_run_is_the_headline_alone_and_full_adds_the_rest():
    plain = _run()
    assert plain["steps"] == 2 and plain["value"] > 0 and plain["ms_per_step"] > 0
    assert plain["proof"] is None and plain["cpu_baseline"] is None
    assert plain["roofline"]["launches_per_step"] > 0 and "valu" not in plain["roofline"]
    full = _run("--full")
    assert full["steps"] == 2 and full["value"] > 0
    assert "error" not in full["proof"] and full["proof"]["quotient_identity_at_x_holds"] and full["proof"]["mock_prover_violations"] == 0
    assert full["roofline"]["valu"]["fr_mul_per_s_microbench"] > 0
    cpu = full["cpu_baseline"]
    assert cpu["commitment_parity_on_sample"] and cpu["witness_parity_on_sample"] and "error" not in cpu["measured_small_proof"]
    assert full["proof"]["vs_cpu_port_estimate"] > 0
