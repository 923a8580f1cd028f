"""tests/proxy_ortho_ref.py, the float64 rasterisation the orthographic proxy pass is tested against (tests/test_proxy_ortho_gpu.py), on its
own: known answers, the conditions every scene of its table has to meet before a comparison against it means anything, the uniform block
of ortho.OrthoCamera.proxy_uniforms byte for byte, and the symbol in the header and the binding table."""
import os
import re
import struct

import numpy as np
import pytest

from gswt_renderer_amd import _lib as L
from gswt_renderer_amd import atmosphere as A
from gswt_renderer_amd import ortho
from tests import atmosphere_ref as AR
from tests import proxy_ortho_ref as O
from tests import proxy_raster_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_flat_plane_under_top_down_known_answers():
    """Every pixel's depth is (z_top - h) / (z_top - z_bottom), its uv the pixel's world xy / (4 tile_width), its triangle the one the
    cell diagonal (i+1, j)-(i, j+1) assigns.  64 x 48 at 0.25 world units per pixel, inside the 21 x 21 map of 4-unit cells."""
    W, H, z_top, z_bottom, h = 64, 48, 10.0, -10.0, -0.5
    cam = ortho.top_down((0.3, 0.2), 6.0, z_top, z_bottom, W, H)
    u = cam.proxy_uniforms(map_proxy=1, height_offset=h, tile_width=4.0, surface_type=0, map_half_wh=(10, 10))
    mips = R.mip_chain()
    r = O.render(u, W, H, mips=mips)
    assert r["written"].all()
    np.testing.assert_allclose(r["depth"], (z_top - h) / (z_top - z_bottom), rtol=0, atol=1e-8)
    np.testing.assert_allclose(ortho.height_from_depth(cam, r["depth"]), h, rtol=0, atol=2e-7)
    ys, xs = np.mgrid[0:H, 0:W]
    wx = 0.3 + ((xs + 0.5) / W * 2.0 - 1.0) * cam.half_width           # +x to the right, +y up the image
    wy = 0.2 + (1.0 - (ys + 0.5) / H * 2.0) * cam.half_height
    np.testing.assert_allclose(r["hit"][..., 0], wx, rtol=0, atol=1e-6)
    np.testing.assert_allclose(r["hit"][..., 1], wy, rtol=0, atol=1e-6)
    np.testing.assert_allclose(r["hit"][..., 2], h, rtol=0, atol=1e-12)
    ci, cj = np.floor(wx / 4.0 + 10).astype(int), np.floor(wy / 4.0 + 10).astype(int)
    fx, fy = wx / 4.0 + 10 - ci, wy / 4.0 + 10 - cj
    ok = (np.abs(fx + fy - 1.0) > 1e-6) & ~r["amb"]
    assert ok.mean() > 0.9
    assert np.array_equal(r["tri"][ok], (2 * (ci * 21 + cj) + (fx + fy > 1.0))[ok])
    # the colour is the texture at uv = world xy / 16, level 0 (16 / 64 texel per pixel: rho < 1), over the whole frame
    uv = np.stack([wx, wy], -1) / 4.0 / 4.0
    want = R._bilinear_repeat(np.asarray(mips[0], np.float64)[..., :3], uv[..., 0], uv[..., 1])
    np.testing.assert_allclose(r["rgba"][..., :3], want, rtol=0, atol=1e-6)
    assert (r["rgba"][..., 3] == 1.0).all()


def test_fog_known_answer():
    """The flat plane again: the fogged colour is the unfogged one blended by F(|hit - cam_pos|) of tests/atmosphere_ref.py."""
    W, H = 32, 24
    cam = ortho.top_down((0.0, 0.0), 6.0, 10.0, -10.0, W, H, lod_pos=(5.0, 3.0, 2.0))
    u = cam.proxy_uniforms(map_proxy=1, height_offset=-0.5, tile_width=4.0, surface_type=0, map_half_wh=(10, 10))
    assert tuple(u.cam_pos) == (5.0, 3.0, 2.0, 0.0)
    fog = A.Atmosphere(fog=(0.03, 5.0, 0.9, (0.6, 0.7, 0.8)))
    r0, r1 = O.render(u, W, H, mips=R.mip_chain()), O.render(u, W, H, mips=R.mip_chain(), fog=fog)
    assert np.array_equal(r0["depth"], r1["depth"]) and np.array_equal(r0["written"], r1["written"])
    dist = np.sqrt(((r0["hit"] - np.array([5.0, 3.0, 2.0])) ** 2).sum(-1))
    F = AR.fog_amount_f64(dist, AR.params(fog))[..., None]
    assert F.max() > 0.15 and F.min() == 0.0 and (F > 0).mean() > 0.5          # (the fog begins 5 units from cam_pos)
    want = r0["rgba"][..., :3] * (1.0 - F) + np.array([0.6, 0.7, 0.8], np.float32).astype(np.float64) * F
    np.testing.assert_allclose(r1["rgba"][..., :3], want, rtol=0, atol=1e-12)


@pytest.mark.parametrize("name", sorted(O.SCENES))
def test_scene_conditions(name):
    """Coverage of the reference above 5 %, rounding bands below the suite's max_amb (2 %, far scenes 10 %); the tabulated scenes reproduce
    the coverage of the float64 prototype they were chosen with."""
    us, grid_dim, hm, mips, opt, (depth, rgba, amb, res, col_tol) = O.scene_reference(name)
    cov = float((depth < 1.0).mean())
    tol, emu = O.depth_tol(us, O.W0, O.H0, res, amb)
    print(f"{name}: coverage {cov:.3f}, bands {amb.mean():.3%}, f32 emulation error {emu:.2e}, depth bound {tol:.2e}")
    assert cov > 0.05
    assert amb.mean() < opt.get("max_amb", 0.02)
    assert np.isfinite(depth).all() and np.isfinite(rgba).all() and depth.min() >= 0.0 and depth.max() <= 1.0
    assert np.isfinite(emu) and 1e-6 <= tol < 1e-3
    if name in O.COVERAGE:
        assert abs(cov - O.COVERAGE[name]) < 1e-3
    # every fragment lies inside its triangle
    hit = res[-1]["tri"] != O.NO_HIT
    assert (res[-1]["margin"][hit] >= 0.0).all()


def test_table_names_the_issues_scenes():
    assert set(O.TABULATED) == set(O.COVERAGE) and set(O.TABULATED) < set(O.SCENES) and len(O.SCENES) == len(O.TABULATED) + 4


def test_proxy_uniforms_is_the_block_laid_out_by_hand():
    cam = ortho.OrthoCamera(257, 161, (-40.0, -50.0, 40.0), (5.0, 3.0, 0.0), (0.0, 0.0, 1.0), 35.0, 1.0, 160.0, lod_pos=(5.0, 3.0, 2.0))
    u = cam.proxy_uniforms(height_offset=-0.45, tile_width=3.7, surface_type=1, width_scale=5.3, map_proxy=1, use_clip=1, clip_height=0.3,
                           brightness=0.5, black_background=1, map_half_wh=(10, 9), center_coord=(27000, -25000),
                           height_map_scale=(1.0, 2.0, 1.5))
    want = struct.pack("<ffIfIIffI3I", -0.45, 3.7, 1, 5.3, 1, 1, 0.3, 0.5, 1, 0, 0, 0)
    want += np.asarray(cam.view, "<f4").tobytes() + np.asarray(cam.projection, "<f4").tobytes()
    want += struct.pack("<2I2i4f4f", 10, 9, 27000, -25000, 1.0, 2.0, 1.5, 0.0, 5.0, 3.0, 2.0, 0.0)
    assert len(want) == 224 and bytes(u) == want
    # defaults, and cam_pos = the eye without a lod_pos
    cam = ortho.top_down((1.0, 2.0), 5.0, 3.0, -1.0, 64, 32)
    d = cam.proxy_uniforms()
    assert (d.tile_width, d.width_scale, d.brightness, d.map_proxy, d.surface_type) == (1.0, 1.0, 1.0, 0, 0)
    assert tuple(d.cam_pos) == (1.0, 2.0, 3.0, 0.0) and tuple(d.height_map_scale) == (1.0, 1.0, 1.0, 0.0)
    for bad in ("view", "projection", "cam_pos", "no_such_field"):
        with pytest.raises(TypeError):
            cam.proxy_uniforms(**{bad: 1})


def test_header_declares_and_lib_binds_the_symbol():
    hdr = open(os.path.join(ROOT, "include", "gswt_hip.h")).read()
    m = re.search(r"GSWT_API int gswt_proxy_render_ortho\(([^;]*)\);", hdr)
    assert m, "include/gswt_hip.h does not declare gswt_proxy_render_ortho"
    args = [a.strip() for a in m.group(1).replace("\n", " ").split(",")]
    assert len(args) == 7 and args[1].startswith("const gswt_proxy_uniforms")
    assert L.SYMBOLS["gswt_proxy_render_ortho"] == L.SYMBOLS["gswt_proxy_render"]
    assert "skybox_render remains" in " ".join(hdr.split()) and "gswt_proxy_render remain perspective-only" not in " ".join(hdr.split())
