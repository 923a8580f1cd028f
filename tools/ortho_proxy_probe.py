#!/usr/bin/env python3
"""Cost of the orthographic proxy pass (gswt_proxy_render_ortho) beside the perspective gswt_proxy_render of the same frame size and grid:
one pass alone per call (depth clear included, as a frame runs it), median over 30 calls after 5 warm-up calls, timed by events on the
context's stream.  The ground is c5's 129 x 129 tile map (tile_width 4) with the HeightMap surface, as the map grid and as the 2048 full
grid, seen top-down and from one oblique direction; the perspective camera of a row looks along the same axis from where its 45-degree
frustum spans the same footprint.
usage: tools/ortho_proxy_probe.py [calls, default 30]"""
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from gswt_renderer_amd import _lib as L
from gswt_renderer_amd import host, ortho
from gswt_renderer_amd.renderer import GSWTRenderer

n = int(sys.argv[1]) if len(sys.argv) > 1 else 30
HALF, TW = 64, 4.0
EXTENT = (2 * HALF + 1) * TW / 2.0              # 258 world units from the map's centre to its edge
r = GSWTRenderer(0)
stream = torch.cuda.Stream()
r.set_stream(stream.cuda_stream)
r.configure(np.random.default_rng(0).uniform(-1.0, 1.0, (64, 64)).astype(np.float32))
ts = 512
yy, xx = np.mgrid[0:ts, 0:ts]
cur = np.zeros((ts, ts, 4), np.float32)
cur[..., 0] = ((xx // 32 + yy // 32) % 2) * 0.6 + 0.2
cur[..., 1], cur[..., 2], cur[..., 3] = 0.35, 0.25, 1.0
mips = [cur]
while mips[-1].shape[0] > 1:
    p = mips[-1]
    mips.append(p.reshape(p.shape[0] // 2, 2, p.shape[1] // 2, 2, 4).mean((1, 3)).astype(np.float32))
r.proxy_configure(mips, grid_dim=2048)
FIELDS = dict(height_offset=-0.5, tile_width=TW, surface_type=1, width_scale=4.0, brightness=1.0, map_half_wh=(HALF, HALF),
              height_map_scale=(1.0, 1.0, 2.0))
OBLIQUE = np.array([-300.0, -400.0, 300.0])


def blocks(view, size, map_proxy):
    """(orthographic block, perspective block) of one view."""
    if view == "top-down":
        cam = ortho.top_down((0.0, 0.0), EXTENT, 8.0, -4.0, size, size)
        h = EXTENT / math.tan(math.radians(22.5))
        cu, _ = host.camera_uniforms((0.0, 0.0, h), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 45.0, 0.1, 2400.0, size, size)
    else:
        cam = ortho.OrthoCamera(size, size, OBLIQUE, (0.0, 0.0, 0.0), (0.0, 0.0, 1.0), EXTENT, 1.0, 1200.0)
        d = EXTENT / math.tan(math.radians(22.5))
        eye = OBLIQUE / np.linalg.norm(OBLIQUE) * d
        cu, _ = host.camera_uniforms(tuple(eye), (0.0, 0.0, 0.0), (0.0, 0.0, 1.0), 45.0, 0.1, 2400.0, size, size)
    ou = cam.proxy_uniforms(map_proxy=map_proxy, **FIELDS)
    pu = L.ProxyUniforms.from_buffer_copy(bytes(ou))
    pu.view[:] = cu.view[:]; pu.projection[:] = cu.projection[:]; pu.cam_pos[:] = cu.cam_pos[:]
    return ou, pu


def timed(u, size, projection, rgba, depth):
    ms = []
    for i in range(n + 5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        r.proxy_render(u, size, size, rgba.data_ptr(), depth.data_ptr(), True, projection=projection)
        e1.record(stream)
        e1.synchronize()
        if i >= 5:
            ms.append(e0.elapsed_time(e1))
    return float(np.median(ms)), float(np.min(ms)), float((depth < 1.0).float().mean())


print(f"proxy pass alone (depth clear + k_proxy), {n} calls each after 5 warm-up calls, stream events; 129 x 129 map, tile_width 4, HeightMap surface, 64 x 64 height map")
print(f"{'size':>5} {'grid':>10} {'view':>9}   {'ortho median ms':>15} {'min':>8} {'written':>8}   {'perspective median ms':>21} {'min':>8} {'written':>8}")
for size in (1024, 2048):
    rgba = torch.zeros((size, size, 4), dtype=torch.float32, device="cuda")
    depth = torch.zeros((size, size), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    for map_proxy, grid in ((1, "map 129"), (0, "full 2048")):
        for view in ("top-down", "oblique"):
            ou, pu = blocks(view, size, map_proxy)
            o = timed(ou, size, 1, rgba, depth)
            p = timed(pu, size, 0, rgba, depth)
            print(f"{size:>5} {grid:>10} {view:>9}   {o[0]:>15.4f} {o[1]:>8.4f} {o[2]:>8.3f}   {p[0]:>21.4f} {p[1]:>8.4f} {p[2]:>8.3f}")
r.close()
