"""k_proxy against tests/proxy_raster_ref.py, the float64 rasterisation of the reference's proxy mesh: the scenes and bounds of
tests/test_proxy_raster_cpu.py, with the kernel in the oracle's place.  Nothing here calls orc_proxy."""
import numpy as np
import pytest

from tests import proxy_raster_ref as R
from tests.test_proxy_raster_cpu import DEPTH_TOL, MAP_CASES, run_scene

pytestmark = pytest.mark.gpu


def _kernel(renderer):
    import torch

    def draw(us, W, H, grid_dim, hm, mips):
        renderer.configure(hm)
        renderer.proxy_configure(mips, grid_dim=grid_dim)
        rgba = torch.from_numpy(R.sky(W, H)).cuda()
        depth = torch.zeros((H, W), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        for k, u in enumerate(us):
            renderer.proxy_render(u, W, H, rgba.data_ptr(), depth.data_ptr(), clear_depth=(k == 0))
        renderer.synchronize()
        return depth.cpu().numpy(), rgba.cpu().numpy()
    return draw


@pytest.mark.parametrize("name,hm_n", MAP_CASES)
def test_kernel_matches_rasterised_mesh(renderer, name, hm_n):
    try:
        run_scene(name, _kernel(renderer), R.height_map(n=hm_n))
    finally:
        renderer.configure(None)


def test_kernel_matches_rasterised_mesh_reference_scale(renderer):
    (W, H), win, cam_kw, draws = R.BIG
    x0, y0, w, h = win
    cam = R.scene_camera(cam_kw, W, H)
    us = R.scene_uniforms(cam, draws)
    hm, mips = R.height_map(), R.mip_chain()
    try:
        got_d, got_c = _kernel(renderer)(us, W, H, 2048, hm, mips)
    finally:
        renderer.configure(None)
    ref_d, ref_c, amb, _, _ = R.reference(us, W, H, grid_dim=2048, hm=hm, mips=mips, window=win)
    assert (ref_d < 1.0).mean() > 0.5
    R.compare(got_d[y0:y0 + h, x0:x0 + w], got_c[y0:y0 + h, x0:x0 + w], ref_d, ref_c, amb, depth_tol=DEPTH_TOL, col_tol=5e-4)
