"""orc_proxy (the oracle's ray cast of the proxy grid) against tests/proxy_raster_ref.py, an independent float64 rasterisation
of the reference's triangle mesh.  The kernel-against-oracle tests cannot see an error the two share (the cell diagonal, the
DDA's entry cell or walk, the near / far rule); this file pins the oracle to the mesh the reference draws, and
tests/test_proxy_raster_gpu.py pins k_proxy to the same reference.

Off the rounding bands (pixels within eps_edge of a triangle edge, 1e-6 of the near / far plane or incoming depth, 1e-5 of the
clip height), coverage must be equal, depth within DEPTH_TOL near the origin and colour within 1e-4.  Far from the origin the
depth bound is DEPTH_FACTOR times what a rasteriser working in f32 (per-vertex clip = GP V p in f32, z / w interpolated in
f64) makes of the same mesh, plus 1e-6, and colour may move by what the f32 rounding of uv (~1e4 there) allows."""
import numpy as np
import pytest

from oracle import gswt_oracle as orc
from tests import proxy_raster_ref as R

DEPTH_TOL = 1e-6
DEPTH_FACTOR = 2.0
# Every scene with the 16 x 16 height map and with a 12 x 12 one: the repeat sampler wraps a power-of-two map with an AND and any
# other size with a quotient and two fix-ups, and k_proxy shares that sampler with the splats.  (The 16 x 16 cases keep their ids.)
HM_SIZES = (16, 12)
MAP_CASES = [pytest.param(name, n, id=name if n == 16 else f"{name}-hm{n}") for n in HM_SIZES for name in sorted(R.SCENES)]


def _oracle(us, W, H, grid_dim, hm, mips):
    rgba, depth = R.sky(W, H), np.ones((H, W), np.float32)
    for u in us:
        orc.proxy_render(u, W, H, rgba, depth, mips, height_map=hm if int(u.surface_type) == 1 else None, grid_dim=grid_dim)
    return depth, rgba


def run_scene(name, draw_fn, hm=None):
    cam_kw, draws, grid_dim, opt = R.SCENES[name]
    W, H = R.W0, R.H0
    cam = R.scene_camera(cam_kw, W, H)
    us = R.scene_uniforms(cam, draws)
    hm, mips = R.height_map() if hm is None else hm, R.mip_chain()
    got_d, got_c = draw_fn(us, W, H, grid_dim, hm, mips)
    eps = opt.get("eps_edge", 1e-4)
    ref_d, ref_c, amb, res, ctol = R.reference(us, W, H, grid_dim=grid_dim, hm=hm, mips=mips, eps_edge=eps)
    cov = (ref_d < 1.0).mean()
    assert cov > 0.05, f"{name}: the draws cover {cov:.1%} only"
    if "depth_tol" in opt:
        emu = R.emulated_error(us, W, H, res, amb)
        tol = DEPTH_FACTOR * emu + 1e-6
    else:
        emu, tol = None, DEPTH_TOL
    derr = R.compare(got_d, got_c, ref_d, ref_c, amb, depth_tol=tol, colour=opt.get("colour", True),
                     max_amb=opt.get("max_amb", 0.02), ulp_tol=ctol)
    return derr, emu


@pytest.mark.parametrize("name,hm_n", MAP_CASES)
def test_oracle_matches_rasterised_mesh(name, hm_n):
    run_scene(name, _oracle, R.height_map(n=hm_n))


def test_oracle_matches_rasterised_mesh_reference_scale():
    """The 129 x 129 tile map at 3840 x 2160: the oracle draws the whole frame, the reference one window of it."""
    (W, H), win, cam_kw, draws = R.BIG
    x0, y0, w, h = win
    cam = R.scene_camera(cam_kw, W, H)
    us = R.scene_uniforms(cam, draws)
    hm, mips = R.height_map(), R.mip_chain()
    got_d, got_c = _oracle(us, W, H, 2048, hm, mips)
    ref_d, ref_c, amb, _, _ = R.reference(us, W, H, grid_dim=2048, hm=hm, mips=mips, window=win)
    assert (ref_d < 1.0).mean() > 0.5
    # uv reaches ~32 here: the f32 uv of the ray cast moves the checker's bilinear ramps by up to ~2e-4
    R.compare(got_d[y0:y0 + h, x0:x0 + w], got_c[y0:y0 + h, x0:x0 + w], ref_d, ref_c, amb, depth_tol=DEPTH_TOL, col_tol=5e-4)


def test_reference_known_answers():
    """The reference itself on a flat grid seen straight down the z axis: every pixel's depth is the plane's z / w, the
    uv is the pixel's world xy / (4 tile_width), and the triangle is the one the cell diagonal (i+1, j)-(i, j+1) assigns."""
    W, H = 64, 48
    cam = orc.Camera(W, H, (0.3, 0.2, 10.0), (0.3, 0.2000001, 0.0), [0, 1, 0])
    u = orc.proxy_uniforms(cam, map_proxy=1, height_offset=-0.5, surface_type=0, map_half_wh=(10, 10))
    r = R.render(u, W, H, mips=[np.zeros((1, 1, 4), np.float32)])
    assert r["written"].all()
    _, t, GP = R.camera(u)
    w = 10.5
    np.testing.assert_allclose(r["depth"], (GP[2, 2] * -w + GP[2, 3]) / w, rtol=0, atol=1e-9)
    hit = r["cam_hit"]
    np.testing.assert_allclose(-hit[..., 2], w, rtol=1e-7)      # R is orthonormal to f32 only
    # the triangle: lattice cell from the world xy (camera axes: x -> world x, y -> world y)
    Rm, tt, _ = R.camera(u)
    world = np.einsum("rc,hwr->hwc", Rm, hit - tt)             # R^T (c - t), R orthonormal to f32 rounding
    ci = np.floor(world[..., 0] / 4.0 + 10).astype(int)
    cj = np.floor(world[..., 1] / 4.0 + 10).astype(int)
    fx, fy = world[..., 0] / 4.0 + 10 - ci, world[..., 1] / 4.0 + 10 - cj
    ok = np.abs(fx + fy - 1.0) > 1e-6
    want = 2 * (ci * 21 + cj) + (fx + fy > 1.0)
    assert np.array_equal(r["tri"][ok], want[ok])
