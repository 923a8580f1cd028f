"""bench.py --dump-outputs on the device: the last timed frame of the fly path (worker thread and swap-ins included) comes out the
same from two runs with the same arguments, `--steps` is the number of timed frames, and `ms_per_step` is their mean time."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run_bench(out_dir, *args):
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "GSWT_BENCH_FAKE_WORLD", "GSWT_BENCH_FORCE_DIST"):
        env.pop(k, None)
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--workload", "tiny", "--steps", "24", "--warmup", "8",
           "--no-cpu-baseline", "--static-steps", "12", "--dump-outputs", str(out_dir), *args]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=420, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.strip().splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def _load(d):
    return {f: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


@pytest.mark.parametrize("mode", ["flypath", "static"])
def test_dump_outputs_are_reproducible(tmp_path, mode):
    runs = []
    for k in range(2):
        d = tmp_path / f"run{k}"
        res = _run_bench(d, "--mode", mode)
        assert res["steps"] == 24 and res["warmup"] == 8
        assert res["ms_per_step"] > 0 and abs(res["ms_per_step"] * res["value"] - 1e3) < 1e-6 * 1e3
        assert res["dump_outputs"]["frame"] == 8 + 24 - 1
        if mode == "flypath":
            assert res["sort_events"]["swapped_in"] >= 1, res["sort_events"]    # the worker's results were swapped in during the timed steps
        runs.append(_load(d))
    a, b = runs
    assert sorted(a) == ["frame_counts.npy", "image.npy"]
    img = a["image.npy"]
    assert img.dtype == np.float32 and img.shape == (240, 320, 4) and np.isfinite(img).all()
    assert a["frame_counts.npy"].dtype == np.float64 and a["frame_counts.npy"][2] > 0     # n_visible
    assert np.abs(img[..., :3]).max() > 0                                                  # something was drawn
    for f in a:
        assert np.array_equal(a[f], b[f]), f
