#!/usr/bin/env python3
"""What gswt_set_tile_styles costs: the project stage (k_cull + k_project + k_totals between the frame's stage events, as in
tools/project_ab.py) of frames run one at a time in a workload's own view, with styles off, on with one highlighted cell (the cell that
owns the most picked pixels: tinted) and on with a quarter of the map's cells hidden.  An A/B against another build:
GSWT_HIP_LIB=<.so>.
Usage: tile_style_probe.py [workload, default c3] [frames, default 40]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402  (before the library: conftest.py of the tests explains)

import bench  # noqa: E402
from gswt_renderer_amd import _lib as L  # noqa: E402
from gswt_renderer_amd import styles as ST  # noqa: E402
from gswt_renderer_amd.renderer import GSWTRenderer  # noqa: E402

name = sys.argv[1] if len(sys.argv) > 1 else "c3"
n = int(sys.argv[2]) if len(sys.argv) > 2 else 40
w, wang, cu, vp, sort = bench.build_workload(name)
W, H = w["width"], w["height"]
su = wang.scene_uniforms()
r = GSWTRenderer(0)
r.set_option(L.GSWT_OPT_TIMING, 2)
wang.upload_to(r)
r.configure(wang.height_map() if int(wang.user.surface_type) == 1 else None)
r.set_draws(sort.draws, sort.merged_gs_index, sort.merged_map_id, sort.merged_lod_id)
half, st = tuple(su.map_half_wh), int(su.surface_type)
n_cells = ST.map_width(half, st) * ST.map_height(half, st)
_, pick = r.render(cu, su, W, H, transmittance_eps=1e-5, pick=True)
ids, cnt = np.unique(pick["map_index"][pick["weight"] > 0], return_counts=True)
top = int(ids[np.argmax(cnt)])
one = bytearray(8 * n_cells)
one[8 * top:8 * top + 8] = ST.TileStyle(tint=(255, 220, 40), strength=160).pack()
quarter = bytearray(8 * n_cells)
for i in range(0, n_cells, 4):
    quarter[8 * i:8 * i + 8] = ST.HIDE.pack()
lib = os.path.basename(os.environ.get("GSWT_HIP_LIB", "default"))
out = torch.empty((H, W, 4), dtype=torch.float32, device="cuda")
torch.cuda.synchronize()
base = None
for label, table in (("off", b""), (f"one highlighted cell ({top} of {n_cells})", bytes(one)), ("a quarter of the cells hidden", bytes(quarter))):
    r.set_tile_styles(table)
    ts = []
    for i in range(n + 8):
        r.render_wait(r.render_async(cu, su, W, H, out.data_ptr(), transmittance_eps=1e-5))
        ts.append(r.timings())
    ts = ts[8:]
    row = dict(project=1e3 * float(np.median([t["ms_project"] for t in ts])), pmin=1e3 * min(t["ms_project"] for t in ts),
               frame=1e3 * float(np.median([t["ms_total"] for t in ts])), visible=ts[-1]["n_visible"], pairs=ts[-1]["n_pairs"])
    rel = "" if base is None else f"  (x{row['project'] / base['project']:.3f} project stage, x{row['frame'] / base['frame']:.3f} frame vs off)"
    base = base or row
    print(f"{lib} {name} {W}x{H} styles {label}: project stage {row['project']:.1f} us (min {row['pmin']:.1f}), frame {row['frame']:.1f} us, "
          f"n_visible {row['visible']}, n_pairs {row['pairs']}{rel}", flush=True)
r.close()
