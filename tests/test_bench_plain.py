"""bench.py as a plain run (no --full): the timed path alone, --steps timed steps, and under --dump-outputs what its last step computed"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from streams import ROOT, synth

pytestmark = pytest.mark.gpu


def test_plain_run_times_its_steps_and_dumps_the_last_steps_pixels(built, tmp_path):
    import j40_amd
    W, H, B, D, steps = 2048, 1280, 8, 2, 3
    out = tmp_path / "dump"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "1",
           "--width", str(W), "--height", str(H), "--batch", str(B), "--distinct", str(D), "--pipe-batch", str(B), "--dump-outputs", str(out)]
    run = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stderr[-3000:]
    lines = [l for l in run.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, run.stdout[-2000:]
    r = json.loads(lines[0])
    assert r["steps"] == steps and r["warmup"] == 1 and r["unit"] == "Mpixels/s" and r["higher_is_better"] is True and r["dtype"] == "f32"
    assert r["ms_per_step"] > 0 and abs(r["value"] - W * H * B / (r["ms_per_step"] / 1e3) / 1e6) <= 0.02 * r["value"]
    for key in ("device_output", "device_resident", "cpu_baseline", "parity_vs_reference", "latency_mode", "configs", "sharded"):
        assert key not in r, key                          # (--full only)
    files = sorted(os.listdir(out))
    assert files == ["rgba_channel_sums.npy", "rgba_sample.npy", "sample_yx.npy"]
    assert sum(os.path.getsize(out / f) for f in files) <= 64 << 20
    sums, sample, yx = (np.load(out / f) for f in files)
    assert sums.dtype == np.float64 and sample.dtype == np.float32 and yx.dtype == np.float64
    assert sums.shape == (D, 4) and sample.shape[0] == D and sample.shape[2] == 4 and yx.shape == (sample.shape[1], 2)
    y, x = yx[:, 0].astype(np.int64), yx[:, 1].astype(np.int64)
    # landing buffer k holds stream k (frames k, k + D, ...): the same pixels as the stream decoded alone through the public API
    for k in range(D):
        err, rgba = j40_amd.decode(synth("vardct", W, H, 3 + 1000 * k, forward=1))
        assert err == ""
        assert np.array_equal(sums[k], rgba.reshape(-1, 4).sum(axis=0, dtype=np.uint64).astype(np.float64))
        assert np.array_equal(sample[k], rgba[y, x].astype(np.float32))
