#!/usr/bin/env python3
"""Cost of the sphere proxy pass (gswt_proxy_render_sphere) at 1920 x 1080 with c3s's camera and radius: one pass alone per call (depth clear
included, as a frame runs it), median over 30 calls after 5 warm-up calls, timed by events on the context's stream.  Perspective (c3s's
camera) and orthographic (the whole planet from the same direction), each with the fog and the sun shade off and on; the shadow map is a
1024^2 orthographic depth-only pass of the same sphere along a sun direction.  For scale, gswt_proxy_render on a flat block (surface_type 0,
the map grid of the same half size) of the same frame size in the same job.
usage: tools/sphere_proxy_probe.py [calls, default 30]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from gswt_renderer_amd import _lib as L
from gswt_renderer_amd import atmosphere as A
from gswt_renderer_amd import host, ortho, shadows
from gswt_renderer_amd.renderer import GSWTRenderer
from gswt_renderer_amd.workloads import WORKLOADS

n = int(sys.argv[1]) if len(sys.argv) > 1 else 30
w = WORKLOADS["c3s"]
W, H, HALF, RAD, TW, OFFSET = w["width"], w["height"], w["half"], w["user"]["sphere_radius"], 4.0, -0.5
cam = w["camera"]
r = GSWTRenderer(0)
stream = torch.cuda.Stream()
r.set_stream(stream.cuda_stream)
r.configure(None)
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
FIELDS = dict(height_offset=OFFSET, tile_width=TW, surface_type=2, map_proxy=1, brightness=1.0, map_half_wh=HALF)
eye = np.array(cam["pos"], np.float64)
ocam = ortho.OrthoCamera(W, H, eye, cam["target"], cam["up"], 1.05 * RAD, 1.0, 2.0 * float(np.linalg.norm(eye)))
ou = ocam.proxy_uniforms(**FIELDS)
cu, _ = host.camera_uniforms(cam["pos"], cam["target"], cam["up"], cam["fovy"], cam["near"], cam["far"], W, H)
pu = L.ProxyUniforms.from_buffer_copy(bytes(ou))
pu.view[:] = cu.view[:]; pu.projection[:] = cu.projection[:]; pu.cam_pos[:] = cu.cam_pos[:]
flat = L.ProxyUniforms.from_buffer_copy(bytes(pu))
flat.surface_type = 0
FOG = A.Atmosphere(fog=(0.01, 40.0, 0.8, (0.6, 0.7, 0.8)))
rgba = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
depth = torch.zeros((H, W), dtype=torch.float32, device="cuda")
# the sun map: the same sphere, depth only, from a sun to the right of the camera
sun = ortho.OrthoCamera(1024, 1024, (95.0, 20.0, 35.0), (0.0, 0.0, 0.0), (0.0, 0.0, 1.0), 1.05 * RAD, 1.0, 220.0)
zmap = torch.zeros((1024, 1024), dtype=torch.float32, device="cuda")
scratch = torch.zeros((1024, 1024, 4), dtype=torch.float32, device="cuda")
torch.cuda.synchronize()
r.proxy_render_sphere(sun.proxy_uniforms(black_background=1, **FIELDS), RAD, 1024, 1024, scratch.data_ptr(), zmap.data_ptr(), True, projection=1)
r.synchronize()
LIGHT = shadows.from_ortho_camera(sun, zmap.cpu().numpy(), bias=0.01, strength=0.7, shade_color=(0.02, 0.03, 0.08))


def timed(call):
    ms = []
    for i in range(n + 5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        call()
        e1.record(stream)
        e1.synchronize()
        if i >= 5:
            ms.append(e0.elapsed_time(e1))
    return float(np.median(ms)), float(np.min(ms)), float((depth < 1.0).float().mean())


print(f"proxy pass alone (depth clear + kernel), {W} x {H}, {n} calls each after 5 warm-up calls, stream events; c3s: radius {RAD}, half {HALF}, "
      f"camera {cam['pos']}")
print(f"{'pass':>28} {'fog':>4} {'shade':>6}   {'median ms':>10} {'min':>8} {'written':>8}")
for fog in (False, True):
    for shade in (False, True):
        r.set_atmosphere(FOG if fog else A.OFF)
        r.set_shadow_map(LIGHT if shade else None)
        rows = [("sphere, perspective", lambda: r.proxy_render_sphere(pu, RAD, W, H, rgba.data_ptr(), depth.data_ptr(), True)),
                ("sphere, orthographic", lambda: r.proxy_render_sphere(ou, RAD, W, H, rgba.data_ptr(), depth.data_ptr(), True, projection=1)),
                ("gswt_proxy_render, flat map", lambda: r.proxy_render(flat, W, H, rgba.data_ptr(), depth.data_ptr(), True))]
        for name, call in rows:
            t = timed(call)
            print(f"{name:>28} {'on' if fog else 'off':>4} {'on' if shade else 'off':>6}   {t[0]:>10.4f} {t[1]:>8.4f} {t[2]:>8.3f}")
r.set_atmosphere(A.OFF)
r.set_shadow_map(None)
r.close()
