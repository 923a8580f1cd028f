#!/usr/bin/env python3
"""What gswt_set_clip_volumes costs: stage times (hipEvents, timing level 2) of frames run one at a time in a workload's own perspective
view, with the volumes off, with 1 and with 8 volumes that hide nothing (huge keep boxes: the pure cost of the test on every splat),
and with one keep box around half the tile map (what hiding early saves), then off once more.  Every row is compared with the first `off` row of the same run.
An A/B against another build: GSWT_HIP_LIB=<.so> (a library from before the call reports the `off` row only).  The project stage's event
pair spans k_cull and k_project; for the two kernels apart, run tools/serial_frames.py under `rocprofv3 --kernel-trace --stats`.
Usage: clip_probe.py [workload, default c3] [frames, default 20]"""
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402  (before the library: conftest.py of the tests explains)

import bench  # noqa: E402
from gswt_renderer_amd import _lib as L  # noqa: E402
from gswt_renderer_amd.clip import ClipVolume  # noqa: E402
from gswt_renderer_amd.renderer import GSWTRenderer  # noqa: E402

name = sys.argv[1] if len(sys.argv) > 1 else "c3"
n = int(sys.argv[2]) if len(sys.argv) > 2 else 20
has = hasattr(C.CDLL(L.LIB_PATH), "gswt_set_clip_volumes")
if not has:
    L.SYMBOLS.pop("gswt_set_clip_volumes")          # a build from before the call
w, wang, cu, vp, sort = bench.build_workload(name)
W, H = w["width"], w["height"]
su = wang.scene_uniforms()
r = GSWTRenderer(0)
r.set_option(L.GSWT_OPT_TIMING, 2)
wang.upload_to(r)
r.configure(wang.height_map() if int(wang.user.surface_type) == 1 else None)
r.set_draws(sort.draws, sort.merged_gs_index, sort.merged_map_id, sort.merged_lod_id)
tw = float(su.tile_width)
half = 0.5 * tw * (2 * max(w["half"]) + 1)
centre = (tw * su.center_coord[0], tw * su.center_coord[1], 0.0)
huge = lambda k: ClipVolume.box((centre[0] + k, centre[1], 0.0), (1.0e6, 1.0e6, 1.0e6), keep=True)
sets = [("off", [])]
if has:
    sets += [("1 volume, hides nothing", [huge(0)]), ("8 volumes, hide nothing", [huge(k) for k in range(8)]),
             ("keep box around half the map", [ClipVolume.box((centre[0] - half, centre[1], 0.0), (half, 2.0 * half, 1.0e6), keep=True)]),
             ("off again", [])]             # (the first row of a process reads a few per cent high: this one shows by how much)
lib = os.path.basename(os.environ.get("GSWT_HIP_LIB", "default"))
out = torch.empty((H, W, 4), dtype=torch.float32, device="cuda")
torch.cuda.synchronize()
base = None
for label, vols in sets:
    if has:
        r.set_clip_volumes(vols)
    acc = {}
    for i in range(n + 3):
        r.render_wait(r.render_async(cu, su, W, H, out.data_ptr(), transmittance_eps=1e-5))
        if i >= 3:
            for k, x in r.timings().items():
                if k.startswith("ms_"):
                    acc[k] = acc.get(k, 0.0) + x / n
    t = r.timings()
    row = dict(project=acc["ms_project"] * 1e3, composite=acc["ms_composite_kernel"] * 1e3, frame=acc["ms_total"] * 1e3,
               visible=t["n_visible"], pairs=t["n_pairs"])
    rel = "" if base is None else (f"  (x{row['project'] / base['project']:.3f} project stage, x{row['composite'] / base['composite']:.3f} compositor, "
                                   f"x{row['frame'] / base['frame']:.3f} frame vs off)")
    base = base or row
    print(f"{lib} {name} {W}x{H} clip={label}: project stage (k_cull + k_project) {row['project']:.1f} us, compositor kernel {row['composite']:.1f} us, "
          f"frame {row['frame']:.1f} us, n_visible {row['visible']}, n_pairs {row['pairs']}{rel}", flush=True)
