#!/usr/bin/env python3
"""What GSWT_OPT_ANTIALIAS costs: stage times (hipEvents, timing level 2) of frames run one at a time, with the filter off and at
`value` (default 307, 0.3 px^2), for a workload's own perspective view and for one ortho.top_down minimap of the same scene and
sort event (the whole tile map in a 512 x 512 frame, depth order).  An A/B against another build: GSWT_HIP_LIB=<.so> (a library
that does not know the option reports the `off` rows only).  The project stage's event pair spans k_cull and k_project; for the two
kernels apart, run tools/serial_frames.py under `rocprofv3 --kernel-trace --stats`.
Usage: antialias_probe.py [workload, default c3] [frames, default 20] [value, default 307]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402  (before the library: conftest.py of the tests explains)

import bench  # noqa: E402
from gswt_renderer_amd import _lib as L  # noqa: E402
from gswt_renderer_amd import ortho, workloads  # noqa: E402
from gswt_renderer_amd.renderer import GSWTError, GSWTRenderer  # noqa: E402

name = sys.argv[1] if len(sys.argv) > 1 else "c3"
n = int(sys.argv[2]) if len(sys.argv) > 2 else 20
value = int(sys.argv[3]) if len(sys.argv) > 3 else 307
w, wang, cu, vp, sort = bench.build_workload(name)
W, H = w["width"], w["height"]
su = wang.scene_uniforms()
r = GSWTRenderer(0)
r.set_option(L.GSWT_OPT_TIMING, 2)
wang.upload_to(r)
r.configure(wang.height_map() if int(wang.user.surface_type) == 1 else None)
r.set_draws(sort.draws, sort.merged_gs_index, sort.merged_map_id, sort.merged_lod_id)
try:
    r.set_option(L.GSWT_OPT_ANTIALIAS, 0)
    values = (0, value)
except GSWTError:
    values = (0,)                                   # a build from before the option
pos = workloads.camera_for(name)["pos"]
tw = float(su.tile_width)
half = 0.5 * tw * (2 * max(w["half"]) + 1)          # the whole tile map
MW = MH = 512
views = {"perspective": (cu, W, H, L.GSWT_PROJECTION_PERSPECTIVE, L.GSWT_ORDER_REFERENCE),
         "top_down": (ortho.top_down((pos[0], pos[1]), half, 8.0, -8.0, MW, MH, lod_pos=pos).uniforms(), MW, MH, L.GSWT_PROJECTION_ORTHO,
                      L.GSWT_ORDER_DEPTH)}
lib = os.path.basename(os.environ.get("GSWT_HIP_LIB", "default"))
for view, (cam, vw, vh, proj, order) in views.items():
    out = torch.empty((vh, vw, 4), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    base = None
    for v in values:
        acc = {}
        for i in range(n + 3):
            kw = dict(antialias=v / 1024.0) if len(values) > 1 else {}
            r.render_wait(r.render_async(cam, su, vw, vh, out.data_ptr(), transmittance_eps=1e-5, order_mode=order, projection=proj, **kw))
            if i >= 3:
                for k, x in r.timings().items():
                    if k.startswith("ms_"):
                        acc[k] = acc.get(k, 0.0) + x / n
        t = r.timings()
        row = dict(project=acc["ms_project"] * 1e3, frame=acc["ms_total"] * 1e3, visible=t["n_visible"], pairs=t["n_pairs"])
        rel = "" if base is None else (f"  (x{row['project'] / base['project']:.3f} project stage, x{row['frame'] / base['frame']:.3f} frame, "
                                       f"x{row['pairs'] / max(base['pairs'], 1):.3f} pairs vs off)")
        base = base or row
        print(f"{lib} {name} {view} {vw}x{vh} antialias={v}: project stage (k_cull + k_project) {row['project']:.1f} us, frame {row['frame']:.1f} us, "
              f"n_visible {row['visible']}, n_pairs {row['pairs']}{rel}", flush=True)
