"""GPU: a plain single-GPU bench.py run with --dump-outputs.

One small run of the real command line (`--gpus 1 --steps K --warmup W`, batch 2): the plain
line carries the headline fields and none of the --full measurements, and --dump-outputs writes
the loss dict of the step run from the restored initial state (bench.py restores the weights and
Adam state in place under the captured graph, then replays it) as finite float32 arrays."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.timeout(300)
def test_plain_run_is_lean_and_dumps_outputs(gpu, tmp_path):
    out_dir = tmp_path / "dump"
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "LOCAL_WORLD_SIZE")}
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "2",
                        "--batch", "2", "--dump-outputs", str(out_dir)], cwd=REPO, env=env, capture_output=True,
                       text=True, timeout=280)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-3000:]
    out = json.loads(lines[0])
    # the headline fields, as every run reports them
    assert out["steps"] == 2 and out["warmup"] == 2 and out["n_gpus"] == 1
    assert out["unit"] == "faces/s" and out["higher_is_better"] is True and out["dtype"] == "bf16"
    assert out["ms_per_step"] > 0 and out["value"] > 0
    # value is faces per second of the timed steps: batch / step time
    assert abs(out["value"] - 2 / (out["ms_per_step"] * 1e-3)) <= 0.01 * out["value"]
    assert out["config"]["launch"] == "hipGraph (whole step)", out["config"]
    # a plain run: no probes, no CPU baseline
    assert out["full"] is False
    assert not {"roofline", "roofline_kernels", "cpu_baseline"} & set(out), sorted(out)
    # the dumped step's loss dict
    files = sorted(os.listdir(out_dir))
    assert files == ["loss_D.npy", "loss_G.npy"], files
    total = 0
    for f in files:
        a = np.load(out_dir / f)
        assert a.dtype == np.float32 and a.shape == () and np.isfinite(a), (f, a)
        total += a.nbytes
    assert total <= 64 << 20
