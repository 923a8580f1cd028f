#!/usr/bin/env python3
"""Times gswt_proxy_configure_image at the reference's usual proxy size: a seeded 4096 x 4096 RGBA8 image built into the
13-level Lanczos3 chain 4096 .. 1 (upload_proxy_texture, proxy.rs:513-554).  Prints one JSON line: the call's wall time (the
source upload, the staging allocations, the build and the waits; the call is synchronous) after warm-up, and the build's
algorithmic bytes per kernel:
    vertical pass   : the source read once per resampled level + the f32 intermediate (w x n x 16 B) written
    horizontal pass : the intermediate read once + the level (n^2 x 16 B) written
    copy level      : the source read once + the level written
(tap tables and partial sums are left out: under 2 % of the total).

The kernel times come from a separate profiler run of the same probe, e.g.
    timeout -k 10 300 rocprofv3 --kernel-trace --stats -d <dir> -- python tools/proxy_mip_probe.py --iters 20
(k_lanczos_* / k_proxy_mip_copy in the kernel stats); profiles/proxy_mips_4096.txt holds the measured summary.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def algorithmic_bytes(w, h, tex_size, bpp):
    out = {"k_proxy_mip_copy": 0, "k_lanczos_v": 0, "k_lanczos_h": 0}
    n = tex_size
    while n >= 1:
        if (n, n) == (w, h):
            out["k_proxy_mip_copy"] += w * h * bpp + n * n * 16
        else:
            out["k_lanczos_v"] += w * h * bpp + w * n * 16
            out["k_lanczos_h"] += w * n * 16 + n * n * 16
        n //= 2
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=4096)
    ap.add_argument("--height", type=int, default=4096)
    ap.add_argument("--tex", type=int, default=4096)
    ap.add_argument("--u16", action="store_true")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    import torch  # noqa: F401  (PyTorch's HIP runtime first, as in the tests)
    from gswt_renderer_amd.renderer import GSWTRenderer

    dt = np.uint16 if a.u16 else np.uint8
    img = np.random.default_rng(0).integers(0, np.iinfo(dt).max + 1, (a.height, a.width, 4), dtype=np.int64).astype(dt)
    r = GSWTRenderer(0)
    try:
        for _ in range(a.warmup):
            r.proxy_configure_image(img, a.tex)
        r.synchronize()
        ts = []
        for _ in range(a.iters):
            t0 = time.perf_counter()
            r.proxy_configure_image(img, a.tex)
            r.synchronize()
            ts.append(time.perf_counter() - t0)
        by = algorithmic_bytes(a.width, a.height, a.tex, 8 if a.u16 else 4)
        print(json.dumps({"probe": "proxy_mips", "image": [a.width, a.height], "format": "rgba16" if a.u16 else "rgba8",
                          "tex_size": a.tex, "levels": a.tex.bit_length(), "iters": a.iters,
                          "call_ms_median": round(float(np.median(ts)) * 1e3, 3), "call_ms_min": round(min(ts) * 1e3, 3),
                          "bytes_per_kernel": by, "bytes_total": sum(by.values())}))
    finally:
        r.close()


if __name__ == "__main__":
    main()
