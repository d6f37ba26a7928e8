"""bench.py on the GPU: a plain run honours --steps and --dump-outputs writes the plan of the last timed get_action, the same
plan on every run with the same arguments (fixed inputs and seeds), so two builds can be compared output for output."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(tmp, tag, steps):
    d = os.path.join(str(tmp), tag)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "1",
                        "--dump-outputs", d], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    return lines[0], d


@pytest.mark.gpu
def test_bench_dump_outputs_is_reproducible(gpu, tmp_path):
    a, da = _bench(tmp_path, "a", 3)
    b, db = _bench(tmp_path, "b", 3)
    for out in (a, b):
        assert out["steps"] == 3 and out["ms_per_step"] > 0 and out["value"] > 0 and "legs" not in out
    assert sorted(os.listdir(da)) == ["plan.npy"]
    pa, pb = np.load(os.path.join(da, "plan.npy")), np.load(os.path.join(db, "plan.npy"))
    assert pa.dtype == np.float32 and pa.shape == (1, 30, 6)
    assert np.isfinite(pa).all() and np.abs(pa).max() <= 1.0
    np.testing.assert_array_equal(pa, pb)
