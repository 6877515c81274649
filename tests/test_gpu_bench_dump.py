"""bench.py --dump-outputs: two runs with the same arguments write the same arrays, float64, within the size bound, and the
result line reports the steps it was asked for."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(out_dir):
    res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--small", "--no-proof",
                          "--no-cpu-baseline", "--dump-outputs", str(out_dir)], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-2000:]
    return json.loads(res.stdout.strip().splitlines()[-1])


@pytest.mark.gpu
def test_dump_outputs_repeat_from_run_to_run(tmp_path):
    line_a = _run(tmp_path / "a")
    line_b = _run(tmp_path / "b")
    assert line_a["steps"] == line_b["steps"] == 2 and line_a["ms_per_step"] > 0
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == sorted(os.listdir(tmp_path / "b"))
    assert {"commitments.npy", "centroids.npy", "coeff_sample.npy", "ext_last_column.npy"} <= set(names)
    total = 0
    for name in names:
        a, b = np.load(tmp_path / "a" / name), np.load(tmp_path / "b" / name)
        assert a.dtype == np.float64 and np.array_equal(a, b), name
        total += a.nbytes
    assert total <= 64 << 20
    assert np.load(tmp_path / "a" / "commitments.npy").shape == (line_a["config"]["advice_columns"] + line_a["config"]["lookup_columns"], 16)
