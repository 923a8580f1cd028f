#!/usr/bin/env python3
"""Per-work-item phase stamps of the compositor from a -DGSWT_TRACE build of the library (GSWT_HIP_LIB=build_var/libgswt_hip_trace.so):
one frame per segment length (pairs per work item), the raw stamps saved to trace_<workload>_<seg>.npy in the working directory and a summary printed.
Build: make -C gswt_renderer_amd/csrc variants (hipcc <Makefile flags> -DGSWT_TRACE -shared $(SRCS), the Makefile's source list, -o build_var/libgswt_hip_trace.so)"""
import ctypes as C, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import bench
from gswt_renderer_amd.renderer import GSWTRenderer
from gswt_renderer_amd import _lib as L

name = sys.argv[1] if len(sys.argv) > 1 else "c3"
segments = [int(a, 0) for a in sys.argv[2:]] or [L.GSWT_DEFAULT_SEGMENT]
w, wang, cu, vp, sort = bench.build_workload(name)
W, H = w["width"], w["height"]
su = wang.scene_uniforms()
r = GSWTRenderer(0)
r.set_option(L.GSWT_OPT_TIMING, 2)
wang.upload_to(r)
r.configure(wang.height_map() if int(wang.user.surface_type) == 1 else None)
r.set_draws(sort.draws, sort.merged_gs_index, sort.merged_map_id, sort.merged_lod_id)
out = torch.empty((H, W, 4), dtype=torch.float32, device="cuda")
lib = L.load()
lib.gswt_debug_trace.argtypes = [C.c_void_p, C.c_uint]
N = 1 << 17
for seg in segments:
    r.set_option(L.GSWT_OPT_SEGMENT, seg)
    for i in range(4):
        r.render_wait(r.render_async(cu, su, W, H, out.data_ptr(), transmittance_eps=1e-5))
    t = r.timings()
    buf = np.zeros((N, 8), dtype=np.uint64)
    assert lib.gswt_debug_trace(buf.ctypes.data, N) == 0
    n_items = int(np.count_nonzero(buf[:, 1]))          # items past the real count never stamp [1]; stale rows of earlier settings are cut by the caller
    np.save(f"trace_{name}_{seg}.npy", buf[:min(N, 40000)])
    print(f"{name} seg {seg}: k_composite {1e3 * t['ms_composite_kernel']:.1f} us, pairs {t['n_pairs']}, stamped items {n_items}", flush=True)
r.set_option(L.GSWT_OPT_SEGMENT, L.GSWT_DEFAULT_SEGMENT)
