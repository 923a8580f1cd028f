#!/usr/bin/env python3
"""What gswt_set_atmosphere costs: stage times (hipEvents, timing level 2) of frames run one at a time in a workload's own
perspective view, with the block off, with the far fade alone and with fade + fog.  The ramp lies inside the tile map (and so inside
the culling distance): fade_start / fade_end = 0.4 / 0.7 of the map's half width.  An A/B against another build:
GSWT_HIP_LIB=<.so> (a library from before the call reports the `off` row only).  The project stage's event pair spans k_cull and
k_project; for the two kernels apart, run tools/serial_frames.py under `rocprofv3 --kernel-trace --stats`.
Usage: atmosphere_probe.py [workload, default c3] [frames, default 20]"""
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402  (before the library: conftest.py of the tests explains)

import bench  # noqa: E402
from gswt_renderer_amd import _lib as L  # noqa: E402
from gswt_renderer_amd import atmosphere as A  # noqa: E402
from gswt_renderer_amd.renderer import GSWTRenderer  # noqa: E402

name = sys.argv[1] if len(sys.argv) > 1 else "c3"
n = int(sys.argv[2]) if len(sys.argv) > 2 else 20
has = hasattr(C.CDLL(L.LIB_PATH), "gswt_set_atmosphere")
if not has:
    L.SYMBOLS.pop("gswt_set_atmosphere")            # a build from before the call
w, wang, cu, vp, sort = bench.build_workload(name)
W, H = w["width"], w["height"]
su = wang.scene_uniforms()
r = GSWTRenderer(0)
r.set_option(L.GSWT_OPT_TIMING, 2)
wang.upload_to(r)
r.configure(wang.height_map() if int(wang.user.surface_type) == 1 else None)
r.set_draws(sort.draws, sort.merged_gs_index, sort.merged_map_id, sort.merged_lod_id)
half = 0.5 * float(su.tile_width) * (2 * max(w["half"]) + 1)
fade = (0.4 * half, 0.7 * half)
fog = (1.0 / half, 0.1 * half, 0.9, (0.62, 0.71, 0.80))
blocks = [("off", A.OFF)]
if has:
    blocks += [("fade", A.Atmosphere(fade=fade)), ("fade+fog", A.Atmosphere(fade=fade, fog=fog))]
lib = os.path.basename(os.environ.get("GSWT_HIP_LIB", "default"))
out = torch.empty((H, W, 4), dtype=torch.float32, device="cuda")
torch.cuda.synchronize()
base = None
for label, blk in blocks:
    acc = {}
    for i in range(n + 3):
        kw = dict(atmosphere=blk) if has else {}
        r.render_wait(r.render_async(cu, su, W, H, out.data_ptr(), transmittance_eps=1e-5, **kw))
        if i >= 3:
            for k, x in r.timings().items():
                if k.startswith("ms_"):
                    acc[k] = acc.get(k, 0.0) + x / n
    t = r.timings()
    row = dict(project=acc["ms_project"] * 1e3, composite=acc["ms_composite_kernel"] * 1e3, frame=acc["ms_total"] * 1e3, visible=t["n_visible"], pairs=t["n_pairs"])
    rel = "" if base is None else (f"  (x{row['project'] / base['project']:.3f} project stage, x{row['composite'] / base['composite']:.3f} compositor, "
                                   f"x{row['frame'] / base['frame']:.3f} frame, x{row['pairs'] / max(base['pairs'], 1):.3f} pairs vs off)")
    base = base or row
    print(f"{lib} {name} {W}x{H} atmosphere={label} (ramp {fade[0]:.1f} .. {fade[1]:.1f}): project stage (k_cull + k_project) {row['project']:.1f} us, "
          f"compositor kernel {row['composite']:.1f} us, frame {row['frame']:.1f} us, n_visible {row['visible']}, n_pairs {row['pairs']}{rel}", flush=True)
