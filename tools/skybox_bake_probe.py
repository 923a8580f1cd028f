#!/usr/bin/env python3
"""Times gswt_skybox_configure_equirect at the reference's size: a seeded 4096 x 2048 HDR panorama baked into a 2048^2 x 6
cube (Skybox::CUBEMAP_RESO, skybox.rs:35).  Prints one JSON line: the call's wall time (the panorama upload, the bake and
the waits; the call is synchronous) after warm-up, and the bake's algorithmic bytes (6 n^2 x 16 written + w h x 16 read).

The kernel's own time comes from a separate profiler run of the same probe, e.g.
    timeout -k 10 300 rocprofv3 --kernel-trace --stats -d <dir> -- python tools/skybox_bake_probe.py --iters 20
(k_skybox_bake in the kernel stats); profiles/skybox_bake_2048.txt holds the measured summary.
usage: tools/skybox_bake_probe.py [--width 4096] [--height 2048] [--face 2048] [--iters 10] [--warmup 2]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=4096)
    ap.add_argument("--height", type=int, default=2048)
    ap.add_argument("--face", type=int, default=2048)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    import torch  # noqa: F401  (PyTorch's HIP runtime first, as in the tests)
    from gswt_renderer_amd.renderer import GSWTRenderer

    equi = np.random.default_rng(0).uniform(0.05, 8.0, (a.height, a.width, 4)).astype(np.float32)
    r = GSWTRenderer(0)
    try:
        for _ in range(a.warmup):
            r.skybox_configure_equirect(equi, a.face)
        r.synchronize()
        ts = []
        for _ in range(a.iters):
            t0 = time.perf_counter()
            r.skybox_configure_equirect(equi, a.face)
            r.synchronize()
            ts.append(time.perf_counter() - t0)
        written, read = 6 * a.face * a.face * 16, a.width * a.height * 16
        print(json.dumps({"probe": "skybox_bake", "equi": [a.width, a.height], "face_size": a.face, "iters": a.iters,
                          "call_ms_median": round(float(np.median(ts)) * 1e3, 3), "call_ms_min": round(min(ts) * 1e3, 3),
                          "bytes_written": written, "bytes_read": read, "bytes_total": written + read}))
    finally:
        r.close()


if __name__ == "__main__":
    main()
