"""bench.py's plain run and --dump-outputs on the GPU: a plain run times exactly --steps rollouts
and runs none of the --full legs; the dumped arrays are float32 / float64 .npy files within the
size limit and equal, bit for bit, what one eager Rollout.step() from the reset state leaves
(the timed path replays the same launches in a HIP graph)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL_ONLY = ("cpu_baseline", "cpu_baseline_parallel", "advantage", "toytext", "api_variant", "text_api",
             "eager_ms_per_step", "speedup_vs_cpu_baseline")


def test_plain_run_dumps_the_last_timed_rollout(device, tmp_path):
    import bench
    out = tmp_path / "dump"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "12", "--warmup", "4",
                        "--dump-outputs", str(out)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    lines = [x for x in p.stdout.splitlines() if x.strip()]
    assert len(lines) == 1
    line = json.loads(lines[0])
    assert line["steps"] == 12 and line["full"] is False and line["records_checked"] is True
    assert line["timing"]["trials"] == 1 and line["timing"]["rollouts_timed"] == 12
    assert line["ms_per_step"] > 0 and line["unit"] == "env-steps/s" and line["higher_is_better"] is True
    steps = line["config"]["env_steps_per_rollout_rank0"]
    assert abs(line["value"] - steps / (line["ms_per_step"] * 1e-3)) <= 1e-9 * line["value"]
    for k in FULL_ONLY:
        assert line[k] is None, k
    assert line["roofline"]["achieved"] is None and line["roofline"]["at_scale"] is None

    R = bench.Rollout(device, 0)
    R.step()
    torch.cuda.synchronize()
    want = bench.rollout_outputs(R, R.env.ep)
    files = sorted(os.listdir(out))
    assert files == sorted(k + ".npy" for k in want) == [k + ".npy" for k in line["outputs_dumped"]]
    total = 0
    for k, w in want.items():
        got = np.load(out / (k + ".npy"), allow_pickle=False)
        assert got.dtype in (np.float32, np.float64) and got.dtype == w.dtype and got.shape == w.shape, k
        assert np.isfinite(got).all(), k
        np.testing.assert_array_equal(got, w, err_msg=k)
        total += got.nbytes
    assert total <= 64 << 20
    assert int(want["turn_exec"].sum()) == steps
    # the metrics' NaN cells (the reference divides by zero turns) are dumped as 0 + a code, losslessly
    m, code = R.metrics.cpu().numpy(), want["metrics_nonfinite"]
    np.testing.assert_array_equal(code != 0, ~np.isfinite(m))
    np.testing.assert_array_equal(np.where(code == 1, np.nan, want["metrics"]), m)
