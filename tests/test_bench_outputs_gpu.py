"""A plain `bench.py` run times the steps and nothing else; `--dump-outputs DIR` writes what the last timed step computed
(loss, prob, a seeded sample of the updated parameters and their gradients) as float32 .npy files for build-to-build
comparisons.  Tiny clips: not a measurement."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_prints_the_headline_line_and_dumps_the_last_step(tmp_path):
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "VLFB_BENCH_CHILD", "VLFB_DIST_FORCE"):
        env.pop(k, None)
    out_dir = str(tmp_path / "outputs")
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--clips-per-gpu", "1",
           "--frames", "16", "--crop", "64", "--dump-outputs", out_dir]
    r = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    out = json.loads(lines[0])
    assert out["unit"] == "clips/s" and out["higher_is_better"] is True and out["dtype"] == "mix" and out["steps"] == 3
    assert out["metric"].startswith("clips/sec fwd+bwd") and out["value"] > 0 and out["ms_per_step"] > 0
    assert abs(out["value"] - 1000.0 / out["ms_per_step"]) < 1e-2 * out["value"]          # 1 clip per step
    # nothing beside the timed steps without --full
    assert not {"roofline", "host_enqueue_ms_per_step", "parity", "fp16_path", "cpu_baseline", "allreduce"} & set(out), sorted(out)
    files = sorted(os.listdir(out_dir))
    assert files == ["grads_sample.npy", "loss.npy", "params_sample.npy", "prob.npy"], files
    arrs = {f[:-4]: np.load(os.path.join(out_dir, f)) for f in files}
    assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in arrs.values())
    assert sum(a.nbytes for a in arrs.values()) <= 64 << 20
    assert abs(float(arrs["loss"].reshape(-1)[0]) - out["config"]["final_loss"]) <= 1e-6 * abs(out["config"]["final_loss"])
    assert arrs["params_sample"].shape == arrs["grads_sample"].shape and arrs["params_sample"].size > 1000
    assert np.abs(arrs["grads_sample"]).max() > 0
