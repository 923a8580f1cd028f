#!/usr/bin/env python3
"""Cost of the pick output (gswt_render_async_pick): c3 and c3d at 1920 x 1080, the workload's own camera, ONE frame at a time.
Every frame carries its stage events (GSWT_OPT_TIMING = 2); frames without and with a pick image alternate in blocks.  Reported per
workload, as medians over the frames: the frame's kernel time (ms_total, first kernel to last), the compositor kernel's own time
(ms_composite_kernel: k_composite's events), what follows the sort (ms_composite: k_items + k_composite + k_combine + k_pick_resolve) and
the resolve step (ms_pick_resolve: k_pick_resolve's own events).
The lines are appended to the output file.
usage: tools/pick_probe.py [output file, default profiles/pick_probe_c3.txt] [frames per block, default 40] [blocks per mode, default 4]"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import bench
from gswt_renderer_amd import _lib as L
from gswt_renderer_amd.renderer import GSWTRenderer

out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "pick_probe_c3.txt")
n_frames = int(sys.argv[2]) if len(sys.argv) > 2 else 40
n_blocks = int(sys.argv[3]) if len(sys.argv) > 3 else 4
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


r = GSWTRenderer(0)
for name in ("c3", "c3d"):
    w, wang, cu, vp, sort = bench.build_workload(name)
    W, H = w["width"], w["height"]
    wang.upload_to(r)
    r.configure(None)
    r.set_draws(sort.draws, sort.merged_gs_index, sort.merged_map_id, sort.merged_lod_id)
    su = wang.scene_uniforms()
    out = torch.empty((H, W, 4), dtype=torch.float32, device="cuda")
    pk = torch.empty((H, W, 4), dtype=torch.int32, device="cuda")
    r.set_option(L.GSWT_OPT_TIMING, 2)

    def frame(pick):
        r.render_wait(r.render_async(cu, su, W, H, out.data_ptr(), transmittance_eps=1e-5, out_pick_ptr=pk.data_ptr() if pick else 0))
        return r.timings()

    for pick in (False, True, False, True):                   # warm-up: buffers sized, both code paths loaded
        frame(pick)
    keys = ("ms_total", "ms_composite_kernel", "ms_composite", "ms_pick_resolve")
    got = {False: {k: [] for k in keys}, True: {k: [] for k in keys}}
    for b in range(2 * n_blocks):
        pick = b % 2 == 1
        for _ in range(n_frames):
            t = frame(pick)
            for k in keys:
                got[pick][k].append(t[k])
    med = {p: {k: float(np.median(got[p][k])) for k in keys} for p in got}
    t = r.timings()
    say(f"{name} {W}x{H}, static camera, one frame at a time, transmittance_eps 1e-5, {n_blocks} x {n_frames} frames per mode (alternating blocks); "
        f"pairs {t['n_pairs']}, screen tiles {t['n_tiles']}")
    for p in (False, True):
        m = med[p]
        say(f"  pick {'on ' if p else 'off'}: kernel time per frame {m['ms_total']:.4f} ms   k_composite {m['ms_composite_kernel']:.4f} ms   "
            f"composite stage {m['ms_composite']:.4f} ms (outside k_composite {m['ms_composite'] - m['ms_composite_kernel']:.4f})   "
            f"k_pick_resolve {m['ms_pick_resolve']:.4f} ms")
    a, b = med[False], med[True]
    say(f"  pick on - off: frame {b['ms_total'] - a['ms_total']:+.4f} ms ({b['ms_total'] / a['ms_total']:.3f} x)   k_composite "
        f"{b['ms_composite_kernel'] - a['ms_composite_kernel']:+.4f} ms ({b['ms_composite_kernel'] / a['ms_composite_kernel']:.3f} x)   "
        f"k_pick_resolve {b['ms_pick_resolve']:.4f} ms   rest of the composite stage (k_items, k_combine with its fold) "
        f"{(b['ms_composite'] - b['ms_composite_kernel'] - b['ms_pick_resolve']) - (a['ms_composite'] - a['ms_composite_kernel']):+.4f} ms")
r.close()
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "a") as f:            # appended: the file also holds the kernel resources of both builds
    f.write("\n".join(lines) + "\n")
