"""The chain a top-down map runs: gswt_proxy_render_ortho writes the ground's colour and depth, then an orthographic splat frame
(GSWT_OPT_PROJECTION = 1) takes them as bg_rgba / bg_depth.  The synthetic scene and the cameras of tests/test_ortho_gpu.py, 72 x 40; the
ground is the flat full grid (24 x 24 cells of 4 world units: wider than either view)."""
import numpy as np
import pytest

from gswt_renderer_amd import _lib as L
from gswt_renderer_amd import atmosphere as A
from gswt_renderer_amd import ortho
from oracle import gswt_oracle as orc
from tests import ortho_ref as OR
from tests import proxy_raster_ref as R
from tests import frame_modes as FM

pytestmark = pytest.mark.gpu
W, Hh = OR.W, OR.H
ORTHO, PERSP = L.GSWT_PROJECTION_ORTHO, L.GSWT_PROJECTION_PERSPECTIVE
GRID = 24


@pytest.fixture(autouse=True)
def _defaults(renderer):
    yield
    renderer.set_option(L.GSWT_OPT_PROJECTION, PERSP)
    renderer.set_option(L.GSWT_OPT_NO_LOD_PREFILTER, 0)
    renderer.set_atmosphere(A.OFF)
    renderer.configure(None)


def _ground(renderer, cam, height_offset, **kw):
    """The proxy's images on the device, and their host copies."""
    import torch
    renderer.proxy_configure(R.mip_chain(), grid_dim=GRID)
    u = cam.proxy_uniforms(map_proxy=0, surface_type=0, height_offset=height_offset, tile_width=4.0, width_scale=4.0, **kw)
    rgba = torch.from_numpy(R.sky(W, Hh)).cuda()
    depth = torch.zeros((Hh, W), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    renderer.proxy_render(u, W, Hh, rgba.data_ptr(), depth.data_ptr(), clear_depth=True, projection=ORTHO)
    renderer.synchronize()
    return rgba, depth, rgba.cpu().numpy(), depth.cpu().numpy()


@pytest.mark.parametrize("which", OR.CAMERAS)
def test_ground_above_every_splat_hides_them(renderer, which):
    g = OR.golden()
    FM.bind(renderer, g)
    su, cam = OR.scene_of(g), FM.ortho_cam(which, g)
    rgba_d, depth_d, rgba, depth = _ground(renderer, cam, 5.0)
    assert (depth < 1.0).all() and (depth > 0.0).all()
    img, z = renderer.render(cam.uniforms(), su, W, Hh, projection=ORTHO, order_mode=L.GSWT_ORDER_DEPTH, bg_rgba=rgba_d.data_ptr(),
                             bg_depth=depth_d.data_ptr(), bg_on_device=True, depth=True)
    assert renderer.timings()["n_visible"] > 300          # the splats are there, behind the ground
    assert FM.same(img, rgba) and FM.same(z, depth)


@pytest.mark.parametrize("order_mode", [L.GSWT_ORDER_REFERENCE, L.GSWT_ORDER_DEPTH], ids=["reference", "depth"])
def test_ground_below_the_splats(renderer, order_mode):
    g = OR.golden()
    FM.bind(renderer, g)
    su, cam = OR.scene_of(g), FM.ortho_cam("top", g)
    h = -0.45                                               # z_bottom is -0.5: depth ~0.998, behind nearly every splat
    rgba_d, depth_d, rgba, depth = _ground(renderer, cam, h)
    assert (depth < 1.0).all()
    kw = dict(projection=ORTHO, order_mode=order_mode, depth=True, pick=True)
    chained = renderer.render(cam.uniforms(), su, W, Hh, bg_rgba=rgba_d.data_ptr(), bg_depth=depth_d.data_ptr(), bg_on_device=True, **kw)
    plain = renderer.render(cam.uniforms(), su, W, Hh, bg_rgba=rgba, bg_depth=depth, **kw)
    for a, b in zip(chained, plain):
        assert FM.same(a, b)
    img, z, pick = chained
    free, covered = pick["weight"] == 0, pick["weight"] > 0
    assert free.sum() > 20 and covered.mean() > 0.3
    assert FM.same(z[free], depth[free]) and FM.same(img[free], rgba[free])
    # where no splat reaches, the height field holds the ground instead of z_bottom
    got = ortho.height_from_depth(cam, z[free])
    # (the bound: 16 roundings of 2^-24 at the magnitude of the range, 25.5 -- the ray's origin and hit, the view and the projection)
    assert np.abs(got - h).max() <= 25.5 * 16 * 2.0 ** -24 and (got > cam.z_bottom + 0.04).all()
    assert (ortho.height_from_depth(cam, z[covered]) >= h - 1e-4).all() and (ortho.height_from_depth(cam, z[covered]) > h + 0.01).mean() > 0.5
    # without the ground those pixels are at z_bottom
    _, z0, _ = renderer.render(cam.uniforms(), su, W, Hh, **kw)
    assert (ortho.height_from_depth(cam, z0[free]) == cam.z_bottom).all()


def test_option_left_at_ortho_does_not_reach_the_perspective_proxy(renderer):
    import torch
    g = OR.golden()
    FM.bind(renderer, g)
    renderer.proxy_configure(R.mip_chain(), grid_dim=GRID)
    pc = orc.Camera(W, Hh, g["pos"], g["tgt"], [0, 0, 1])
    u = orc.proxy_uniforms(pc, map_proxy=0, surface_type=0, height_offset=-0.45, tile_width=4.0, width_scale=4.0)
    out = []
    for opt in (PERSP, ORTHO, PERSP):
        renderer.render(FM.ortho_cam("top", g).uniforms(), OR.scene_of(g), W, Hh, projection=ORTHO)      # leaves the option at 1 ...
        renderer.set_option(L.GSWT_OPT_PROJECTION, opt)                                           # ... or puts it back
        rgba = torch.from_numpy(R.sky(W, Hh)).cuda()
        depth = torch.zeros((Hh, W), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        renderer.proxy_render(u, W, Hh, rgba.data_ptr(), depth.data_ptr(), clear_depth=True)
        renderer.synchronize()
        out.append((rgba.cpu().numpy(), depth.cpu().numpy()))
    assert (out[0][1] < 1.0).mean() > 0.2
    for o in out[1:]:
        assert FM.same(o[0], out[0][0]) and FM.same(o[1], out[0][1])
