"""bench.py's plain and --full runs, and --dump-outputs, end to end on the GPU at a small shape.

A plain run times its steps and prints the headline line without the measurements that take runs of their own;
--full adds them (the exact-fp32 arm, the CPU baseline).  --dump-outputs writes what the last timed step computed:
the losses of the result line, the generator's images and its attention masks.  The inputs and the initial weights
are seeded and the step is deterministic (tests/test_gpu_rccl.py pins two models stepping bit-identically), so two
runs with the same arguments write the same arrays bit for bit -- what lets two builds be compared output for
output."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")


def _bench(extra, dump):
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--res", "64", "--batch", "2",
                        "--steps", "2", "--warmup", "1", "--dump-outputs", str(dump)] + extra, env=env,
                       capture_output=True, text=True, timeout=300)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert r.returncode == 0 and len(lines) == 1, f"rc {r.returncode}:\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}"
    return json.loads(lines[0]), {f[:-4]: np.load(dump / f, allow_pickle=False) for f in sorted(os.listdir(dump))}


def test_plain_and_full_runs_dump_the_same_outputs(tmp_path):
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    plain, a = _bench([], tmp_path / "plain")
    full, b = _bench(["--full"], tmp_path / "full")
    for rec in (plain, full):
        assert all(k in rec for k in HEADLINE) and rec["steps"] == 2 and rec["unit"] == "img/s"
        assert abs(rec["value"] - 2 * 1e3 / rec["ms_per_step"]) < 1e-2 * rec["value"]
        assert rec["roofline"]["launches"] == 2 * 18                     # read from the two timed steps
    assert "fp32_math" not in plain and "cpu_baseline" not in plain
    assert full["fp32_math"]["value"] > 0 and full["cpu_baseline"]["value"] > 0
    assert sorted(a) == sorted(b) == ["losses", "mask", "output"]
    assert a["losses"].shape == (4,) and a["output"].shape == (2, 3, 64, 64) and a["mask"].shape[0] == 2
    for k in a:
        assert a[k].dtype == np.float32 and np.isfinite(a[k]).all()
        assert np.array_equal(a[k], b[k]), (k, float(np.abs(a[k] - b[k]).max()))
    assert np.allclose(a["losses"], plain["losses_last_step"], rtol=0, atol=1e-5 * max(1.0, np.abs(a["losses"]).max()))
    assert np.abs(a["output"]).max() <= 1.0 + 1e-6 and a["output"].std() > 0     # tanh-bounded images, not a constant
