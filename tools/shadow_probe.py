#!/usr/bin/env python3
"""What gswt_set_shadow_map costs: stage times (hipEvents, timing level 2) of frames run one at a time in a workload's own perspective
view, with shadows off and with a map of N x N texels (default 2048) from a top-down light over the whole tile map, and the wall time of
the proxy pass (gswt_proxy_render, the bench's proxy_map grid) off and on.  The map is synthetic: 64-texel blocks that alternate
between a depth in front of every splat, one behind every splat and the depth of the plane z = 0, so that the compares go both ways
and the 2 x 2 footprints of neighbouring splats land in different cache lines, as they do for a rendered map.  An A/B against another
build: GSWT_HIP_LIB=<.so> (a library from before the call reports the `off` rows only).  The project stage's event pair spans k_cull and
k_project; for the two kernels apart, run tools/serial_frames.py under `rocprofv3 --kernel-trace --stats`.
Usage: shadow_probe.py [workload, default c3] [frames, default 20] [map size, default 2048]"""
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402  (before the library: conftest.py of the tests explains)

import bench  # noqa: E402
from gswt_renderer_amd import _lib as L  # noqa: E402
from gswt_renderer_amd import ortho, shadows  # noqa: E402
from gswt_renderer_amd.renderer import GSWTRenderer  # noqa: E402

name = sys.argv[1] if len(sys.argv) > 1 else "c3"
n = int(sys.argv[2]) if len(sys.argv) > 2 else 20
size = int(sys.argv[3]) if len(sys.argv) > 3 else 2048
has = hasattr(C.CDLL(L.LIB_PATH), "gswt_set_shadow_map")
if not has:
    L.SYMBOLS.pop("gswt_set_shadow_map")            # a build from before the call
w, wang, cu, vp, sort = bench.build_workload(name)
W, H = w["width"], w["height"]
su = wang.scene_uniforms()
r = GSWTRenderer(0)
r.set_option(L.GSWT_OPT_TIMING, 2)
wang.upload_to(r)
r.configure(wang.height_map() if int(wang.user.surface_type) == 1 else None)
r.set_draws(sort.draws, sort.merged_gs_index, sort.merged_map_id, sort.merged_lod_id)
_, _, pu = bench.make_passes(r, su, cu)
half = 0.5 * float(su.tile_width) * (2 * max(w["half"]) + 1)
centre = (float(su.tile_width) * su.center_coord[0], float(su.tile_width) * su.center_coord[1])
light = ortho.top_down(centre, half, 16.0, -16.0, size, size)
maps = [("off", shadows.OFF)]
if has:
    js, is_ = np.mgrid[0:size, 0:size]
    kind = ((is_ // 64) + (js // 64)) % 3
    Z = np.where(kind == 0, 0.0, np.where(kind == 1, 1.0, 0.5)).astype(np.float32)        # z = 0 is depth 0.5 under this light
    maps.append((f"{size}x{size}", shadows.from_ortho_camera(light, Z, bias=0.002, strength=0.6, shade_color=(0.05, 0.05, 0.15))))
lib = os.path.basename(os.environ.get("GSWT_HIP_LIB", "default"))
out = torch.empty((H, W, 4), dtype=torch.float32, device="cuda")
bg = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
bgd = torch.ones((H, W), dtype=torch.float32, device="cuda")
torch.cuda.synchronize()
base = None
for label, m in maps:
    if has:
        r.set_shadow_map(m)
    acc = {}
    for i in range(n + 3):
        r.render_wait(r.render_async(cu, su, W, H, out.data_ptr(), transmittance_eps=1e-5))
        if i >= 3:
            for k, x in r.timings().items():
                if k.startswith("ms_"):
                    acc[k] = acc.get(k, 0.0) + x / n
    t = r.timings()
    # the proxy pass: wall time of n passes on the ctx stream, one synchronisation
    for _ in range(3):
        r.proxy_render(pu, W, H, bg.data_ptr(), bgd.data_ptr(), True)
    r.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        r.proxy_render(pu, W, H, bg.data_ptr(), bgd.data_ptr(), True)
    r.synchronize()
    proxy_us = (time.perf_counter() - t0) / n * 1e6
    row = dict(project=acc["ms_project"] * 1e3, composite=acc["ms_composite_kernel"] * 1e3, frame=acc["ms_total"] * 1e3, proxy=proxy_us,
               visible=t["n_visible"], pairs=t["n_pairs"])
    rel = "" if base is None else (f"  (x{row['project'] / base['project']:.3f} project stage, x{row['composite'] / base['composite']:.3f} compositor, "
                                   f"x{row['frame'] / base['frame']:.3f} frame, x{row['proxy'] / base['proxy']:.3f} proxy pass vs off)")
    base = base or row
    print(f"{lib} {name} {W}x{H} shadow={label}: project stage (k_cull + k_project) {row['project']:.1f} us, compositor kernel {row['composite']:.1f} us, "
          f"frame {row['frame']:.1f} us, proxy pass (clear + k_proxy, wall) {row['proxy']:.1f} us, n_visible {row['visible']}, n_pairs {row['pairs']}{rel}", flush=True)
