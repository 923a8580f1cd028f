#!/usr/bin/env python3
"""Cost of an orthographic frame (GSWT_OPT_PROJECTION = 1): per-stage gswt_timings of a top-down frame of a workload's whole map
beside the workload's own perspective frame, one frame at a time (serial), GSWT_ORDER_DEPTH.
usage: tools/ortho_probe.py [workload, default c3] [frame size, default 1024] [frames, default 30]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import bench
from gswt_renderer_amd import _lib as L
from gswt_renderer_amd import host, ortho, workloads
from gswt_renderer_amd.renderer import GSWTRenderer

name = sys.argv[1] if len(sys.argv) > 1 else "c3"
size = int(sys.argv[2]) if len(sys.argv) > 2 else 1024
n = int(sys.argv[3]) if len(sys.argv) > 3 else 30
w, wang, cu, vp, sort = bench.build_workload(name)
su = wang.scene_uniforms()
cam = workloads.camera_for(name)
r = GSWTRenderer(0)
r.set_option(L.GSWT_OPT_TIMING, 2)
wang.upload_to(r)
r.configure(wang.height_map() if int(wang.user.surface_type) == 1 else None)
r.set_draws(sort.draws, sort.merged_gs_index, sort.merged_map_id, sort.merged_lod_id)
tw = float(su.tile_width)
centre = (su.center_coord[0] * tw, su.center_coord[1] * tw)
half = (2 * w["half"][1] + 1) * tw / 2.0
top = ortho.top_down(centre, half, 8.0, -4.0, size, size, lod_pos=cam["pos"])
cu_sq, _ = host.camera_uniforms(cam["pos"], cam["target"], cam["up"], cam["fovy"], cam["near"], cam["far"], size, size)
STAGES = ("ms_project", "ms_emit", "ms_sort", "ms_composite", "ms_composite_kernel", "ms_total")
out = torch.empty((max(size, w["height"]) * max(size, w["width"]) * 4,), dtype=torch.float32, device="cuda")
torch.cuda.synchronize()


def run(label, cam_block, W, H, projection):
    rows = []
    for i in range(n + 5):
        r.render_wait(r.render_async(cam_block, su, W, H, out.data_ptr(), transmittance_eps=1e-5, order_mode=L.GSWT_ORDER_DEPTH, projection=projection))
        if i >= 5:
            rows.append(r.timings())
    t = rows[-1]
    med = {k: float(np.median([x[k] for x in rows])) for k in STAGES}
    lo = {k: float(np.min([x[k] for x in rows])) for k in STAGES}
    print(f"{label:28s} {W}x{H}  draws {t['n_draws']} instanced {t['n_instanced']} visible {t['n_visible']} pairs {t['n_pairs']} tiles {t['n_tiles']}")
    print("    median ms  " + "  ".join(f"{k[3:]} {med[k]:.4f}" for k in STAGES))
    print("    min ms     " + "  ".join(f"{k[3:]} {lo[k]:.4f}" for k in STAGES))


print(f"workload {name}, {n} serial frames each after 5 warm-up frames, GSWT_ORDER_DEPTH, transmittance_eps 1e-5, hipEvent stage times")
run("perspective (workload frame)", cu, w["width"], w["height"], L.GSWT_PROJECTION_PERSPECTIVE)
run("perspective (square)", cu_sq, size, size, L.GSWT_PROJECTION_PERSPECTIVE)
run("orthographic top-down (map)", top.uniforms(), size, size, L.GSWT_PROJECTION_ORTHO)
r.set_option(L.GSWT_OPT_PROJECTION, L.GSWT_PROJECTION_PERSPECTIVE)
