#!/usr/bin/env python3
"""Cost of the depth output (gswt_render_async_depth): the same fly-path cameras rendered with and without a depth image.
For each of `poses` cameras sampled along the workload's fly path the tile sort runs on the host (outside the timed region), then
`frames` frames are timed with three in flight, depth off and on in alternating blocks, and k_composite's own time is read from its
kernel events (GSWT_OPT_TIMING = 1) in a separate pass.  Prints frames/s and ms_composite_kernel for both and their ratio.
usage: tools/depth_out_probe.py [workload, default c3] [poses, default 24] [frames per pose and mode, default 30]"""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import bench
from gswt_renderer_amd import _lib as L, flypath, host, workloads
from gswt_renderer_amd.renderer import GSWTRenderer

name = sys.argv[1] if len(sys.argv) > 1 else "c3"
n_poses = int(sys.argv[2]) if len(sys.argv) > 2 else 24
n_frames = int(sys.argv[3]) if len(sys.argv) > 3 else 30
w, wang, cu0, vp0, sort0 = bench.build_workload(name)
W, H = w["width"], w["height"]
cam = workloads.camera_for(name)
path_name = name if os.path.exists(os.path.join(ROOT, "gswt_renderer_amd", "flypaths", name + ".json")) else "c3"
poses = flypath.sample(flypath.load(path_name), 240)[::max(1, 240 // n_poses)][:n_poses]
r = GSWTRenderer(0)
wang.upload_to(r)
r.configure(wang.height_map() if int(wang.user.surface_type) == 1 else None)
su = wang.scene_uniforms()
slots = 3
outs = [torch.empty((H, W, 4), dtype=torch.float32, device="cuda") for _ in range(slots)]
zs = [torch.empty((H, W), dtype=torch.float32, device="cuda") for _ in range(slots)]


def run(cu, depth, n):
    tickets = [None] * slots
    for i in range(n):
        k = i % slots
        if tickets[k] is not None:
            r.render_wait(tickets[k])
        tickets[k] = r.render_async(cu, su, W, H, outs[k].data_ptr(), transmittance_eps=1e-5, out_depth_ptr=zs[k].data_ptr() if depth else 0)
    for t in tickets:
        if t is not None:
            r.render_wait(t)


secs = {False: 0.0, True: 0.0}
kern = {False: [], True: []}
for pos, tgt in poses:
    cu, vp = host.camera_uniforms(pos, tgt, cam["up"], cam["fovy"], cam["near"], cam["far"], W, H)
    wang.build_tiles(pos)
    sort = wang.sort_tiles(pos, vp)
    r.set_draws(sort.draws, sort.merged_gs_index, sort.merged_map_id, sort.merged_lod_id)
    r.set_option(L.GSWT_OPT_TIMING, 0)
    run(cu, False, slots)                                  # warm-up (buffers sized for this view)
    run(cu, True, slots)
    for depth in (False, True, True, False):               # alternating blocks: drift affects both modes alike
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        run(cu, depth, n_frames // 2)
        torch.cuda.synchronize()
        secs[depth] += time.perf_counter() - t0
    r.set_option(L.GSWT_OPT_TIMING, 1)
    for depth in (False, True):
        for _ in range(3):
            r.render_wait(r.render_async(cu, su, W, H, outs[0].data_ptr(), transmittance_eps=1e-5, out_depth_ptr=zs[0].data_ptr() if depth else 0))
            kern[depth].append(r.timings()["ms_composite_kernel"])
n = len(poses) * 2 * (n_frames // 2)
fps = {d: n / secs[d] for d in secs}
ms = {d: float(np.median(kern[d])) for d in kern}
print(f"{name} {W}x{H}, {len(poses)} fly-path cameras x {2 * (n_frames // 2)} frames per mode, 3 in flight, transmittance_eps 1e-5")
print(f"  depth off: {fps[False]:8.1f} frames/s   ms_composite_kernel median {ms[False]:.4f}")
print(f"  depth on : {fps[True]:8.1f} frames/s   ms_composite_kernel median {ms[True]:.4f}")
print(f"  depth on / off: frame rate {fps[True] / fps[False]:.3f}, k_composite time {ms[True] / ms[False]:.3f}")
