"""bench.py's plain run and --dump-outputs: the plain line carries the headline keys and none of the --full legs, --steps
is the number of timed steps, and two runs with the same arguments write the same outputs (float32 / float64 .npy files
within the size limit)."""
import json
import os
import pathlib
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = pathlib.Path(__file__).resolve().parent.parent

HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")
FULL_ONLY = ("one_batch_in_flight", "roofline", "single_stream", "extract_bruteforce_match", "local_ba", "cpu_baseline")


def _run(out_dir):
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    cmd = [sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--batch", "64",
           "--dump-outputs", str(out_dir)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=500, env=env, cwd=str(ROOT))
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])


@pytest.mark.timeout(1100)
def test_plain_run_and_dumped_outputs(tmp_path):
    a, b = tmp_path / "a", tmp_path / "b"
    d = _run(a)
    for k in HEADLINE:
        assert k in d, k
    assert d["steps"] == 3 and d["value"] > 0 and d["ms_per_step"] > 0 and d["unit"] == "frames/s" and d["higher_is_better"]
    assert abs(d["value"] - 64 * 1e3 / d["ms_per_step"]) < 0.01 * d["value"]
    for k in FULL_ONLY:
        assert k not in d, k
    files = sorted(p.name for p in a.glob("*.npy"))
    assert files and sum((a / f).stat().st_size for f in files) <= 64 << 20
    got = {f: np.load(a / f) for f in files}
    for f, x in got.items():
        assert x.dtype in (np.float32, np.float64), f
    assert got["pose.npy"].shape == (64, 6) and np.isfinite(got["pose.npy"]).all()
    assert (got["status.npy"] == 0).all() and got["n_inliers.npy"].min() >= 100
    assert got["keypoint_counts.npy"].min() >= 1000
    _run(b)
    assert sorted(p.name for p in b.glob("*.npy")) == files
    for f in files:
        assert np.array_equal(np.load(b / f), got[f]), f
