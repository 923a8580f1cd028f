"""k_skybox_bake (gswt_skybox_configure_equirect) against the float64 restatement of the reference's bake
(tests/skybox_bake_ref.py), the baked cube through k_skybox, and the skybox state transitions."""
import ctypes as C

import numpy as np
import pytest

from gswt_renderer_amd import _lib as L
from oracle import gswt_oracle as orc
from tests import skybox_bake_ref as R

pytestmark = pytest.mark.gpu

# Bounds against the float64 restatement.
#  smooth / constant panoramas: what f32 evaluation of the same formula leaves (~1e-7 relative).
#  per-texel noise in [0.05, 8]: x = u * w - 0.5 is an f32 value, so ulp-level differences in u (atan2f, the product, the
#  rounding of x itself: ulp(4094) = 4.9e-4) move the tap by up to ~4e-4 texel at w = 4096.  Next to a jump of up to 7.95
#  between neighbouring texels that is a linear-colour error of ~3e-3, and the tone map's slope reaches ~2.3 near 0.05:
#  worst case ~7e-3.  Small panoramas (w <= 257, tap error ~3e-5 texel) stay within 1e-3; at 4096 x 2048 an f32 emulation of the
#  kernel on the CPU already reached 1.9e-3 over 1.2 M texels, so the reference-size noise case is held to the worst-case 1e-2.
#  The mean stays at 1e-5 everywhere: only texels whose taps straddle such a jump move.
TOL_SMOOTH, TOL_CONST = 1e-5, 2e-7
TOL_NOISE_MAX, TOL_NOISE_MAX_4096, TOL_NOISE_MEAN = 1e-3, 1e-2, 1e-5


def smooth_panorama(w, h):
    """Band-limited, periodic in both directions (Repeat wraps it without a step), HDR values in [0.3, 2.1]."""
    c = (np.arange(w) + 0.5) / w * 2 * np.pi
    r = (np.arange(h) + 0.5) / h * 2 * np.pi
    r, c = np.meshgrid(r, c, indexing="ij")
    out = np.full((h, w, 4), 0.5)
    for k in range(3):
        out[..., k] = 1.2 + 0.6 * np.sin((k + 1) * c + k) * np.cos(r) + 0.3 * np.cos(2 * c + r + 0.5 * k)
    return out.astype(np.float32)


def noise_panorama(w, h, seed=0):
    return np.random.default_rng(seed).uniform(0.05, 8.0, (h, w, 4)).astype(np.float32)


def bake(renderer, equi, n):
    renderer.skybox_configure_equirect(equi, n)
    got = renderer.skybox_download()
    assert got.shape == (6, n, n, 4) and np.all(got[..., 3] == 1.0)
    return got


def err(got, ref):
    d = np.abs(got[..., :3].astype(np.float64) - ref[..., :3])
    return float(d.max()), float(d.mean())


@pytest.mark.parametrize("wh", [(1, 1), (64, 32), (257, 129)])
@pytest.mark.parametrize("n", [1, 7, 64, 256])
def test_bake_matches_restatement(renderer, wh, n):
    w, h = wh
    equi = smooth_panorama(w, h)
    mx, _ = err(bake(renderer, equi, n), R.bake(equi, n))
    assert mx <= TOL_SMOOTH, mx
    equi = noise_panorama(w, h, seed=w + n)
    mx, mean = err(bake(renderer, equi, n), R.bake(equi, n))
    assert mx <= TOL_NOISE_MAX and mean <= TOL_NOISE_MEAN, (mx, mean)


@pytest.mark.parametrize("n", [1, 64, 256])
def test_bake_of_a_constant_panorama(renderer, n):
    c = np.array([0.2, 1.0, 3.7], np.float32)
    equi = np.empty((31, 45, 4), np.float32)
    equi[..., :3], equi[..., 3] = c, 5.0
    got = bake(renderer, equi, n)
    want = (c.astype(np.float64) / (c + 1.0)) ** R.GAMMA
    assert float(np.abs(got[..., :3] - want).max()) <= TOL_CONST


def test_bake_seam(renderer):
    """First and last panorama columns differ from each other and from the rest.  At w = 4096 the seam of the baked cube
    (phi = +-pi: the -X face's centre columns at n = 2048) shows column w-1 on one side and column 0 on the other, as the
    restatement does, and no texel mixes the wrap pair (w-1, 0)."""
    w, h, n = 4096, 16, 2048
    equi = np.full((h, w, 4), 0.5, np.float32)
    equi[:, 0, :3], equi[:, w - 1, :3] = (6.0, 0.5, 0.5), (0.5, 6.0, 0.5)
    got = bake(renderer, equi, n)
    yy, xx = np.meshgrid(np.arange(n), np.arange(n // 2 - 8, n // 2 + 8), indexing="ij")
    band = got[1][yy, xx]
    mx, _ = err(band, R.bake_texels(equi, 1, yy, xx, n))
    assert mx <= TOL_NOISE_MAX, mx
    lo = R.tone_map(np.float64(0.5))
    red, green = band[..., 0] > lo + 1e-3, band[..., 1] > lo + 1e-3
    assert green[:, 7].all() and red[:, 8].all()           # phi = +pi - 0.0005 | phi = -pi + 0.0005
    assert not np.any(red & green)


def _edge_sample(n, count, seed):
    rng = np.random.default_rng(seed)
    face = rng.integers(0, 6, count)
    y, x = rng.integers(0, n, count), rng.integers(0, n, count)
    e = np.arange(n)
    ef, ey, ex = [], [], []
    for f in range(6):                                   # every texel of every face's four edges (corners included)
        for yy, xx in ((np.zeros_like(e), e), (np.full_like(e, n - 1), e), (e, np.zeros_like(e)), (e, np.full_like(e, n - 1))):
            ef.append(np.full_like(e, f)); ey.append(yy); ex.append(xx)
    return np.concatenate([face] + ef), np.concatenate([y] + ey), np.concatenate([x] + ex)


@pytest.mark.parametrize("kind", ["smooth", "noise"])
def test_bake_at_reference_size(renderer, kind):
    """CUBEMAP_RESO = 2048 from a 4096 x 2048 panorama: a seeded sample of 1 M texels plus every face's edges."""
    w, h, n = 4096, 2048, 2048
    equi = smooth_panorama(w, h) if kind == "smooth" else noise_panorama(w, h, seed=7)
    got = bake(renderer, equi, n)
    f, y, x = _edge_sample(n, 1_000_000, seed=3)
    mx, mean = err(got[f, y, x], R.bake_texels(equi, f, y, x, n))
    if kind == "smooth":
        assert mx <= TOL_SMOOTH, mx
    else:
        assert mx <= TOL_NOISE_MAX_4096 and mean <= TOL_NOISE_MEAN, (mx, mean)


def _render(renderer, cam, W, Hh):
    import torch
    out = torch.zeros((Hh, W, 4), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    renderer.skybox_render(cam.uniforms(), W, Hh, out.data_ptr())
    renderer.synchronize()
    return out.cpu().numpy()


CAMERAS = (((0.0, 0.0, 1.0), (5.0, 2.0, 1.0)),           # level
           ((0.0, 0.0, 1.0), (-5.0, 0.05, 1.0)),         # across the seam (phi = +-pi of the panorama)
           ((0.0, 0.0, 0.0), (0.05, 0.02, 1.0)),         # ~3 deg from straight up
           ((0.0, 0.0, 0.0), (-0.03, 0.04, -1.0)))       # ~3 deg from straight down


def test_bake_then_render_end_to_end(renderer):
    W, Hh, n = 333, 201, 256
    equi = smooth_panorama(512, 256)
    got = bake(renderer, equi, n)
    ref_faces = R.bake(equi, n).astype(np.float32)
    for pos, tgt in CAMERAS:
        cam = orc.Camera(W, Hh, pos, tgt, [0, 0, 1])
        img = _render(renderer, cam, W, Hh)
        assert float(np.abs(img - orc.skybox_render(cam, ref_faces, W, Hh, 1)).max()) <= 1e-5
        assert float(np.abs(img - orc.skybox_render(cam, got, W, Hh, 1)).max()) <= 1e-5
        assert img[..., :3].std() > 0.01 and np.all(img[..., 3] == 1.0)


def _cube(n):
    rng = np.random.default_rng(n)
    faces = rng.uniform(0.0, 1.0, (6, n, n, 4)).astype(np.float32)
    faces[..., 3] = 1.0
    return faces


def test_bake_and_cube_configure_replace_each_other(renderer):
    """A bake after a cube configure, and a cube configure after a bake, render exactly what a render right after that
    configure renders: the faces, the face size and the equirectangular flag switch together."""
    W, Hh = 160, 96
    cam = orc.Camera(W, Hh, (0.0, 0.0, 1.0), (3.0, 1.0, 1.5), [0, 0, 1])
    equi, cube = smooth_panorama(128, 64), _cube(48)
    renderer.skybox_configure_equirect(equi, 40)
    baked = _render(renderer, cam, W, Hh)
    renderer.skybox_configure(cube, False)
    cubed = _render(renderer, cam, W, Hh)
    # (the first bake left is_equi on and a 40-texel cube: the cube configure takes its own flag and size)
    assert float(np.abs(cubed - orc.skybox_render(cam, cube, W, Hh, 0)).max()) <= 1e-5
    renderer.skybox_configure_equirect(equi, 40)                       # bake after a cube configure
    np.testing.assert_array_equal(_render(renderer, cam, W, Hh), baked)
    renderer.skybox_configure(cube, False)                             # cube configure after a bake
    np.testing.assert_array_equal(_render(renderer, cam, W, Hh), cubed)
    assert not np.array_equal(baked, cubed)


def test_rebake_at_another_face_size(renderer):
    equi = noise_panorama(96, 48, seed=5)
    for n in (64, 300, 7):                                # grows the cube, then fits smaller ones into it
        mx, mean = err(bake(renderer, equi, n), R.bake(equi, n))
        assert mx <= TOL_NOISE_MAX and mean <= TOL_NOISE_MEAN, (n, mx, mean)


def test_bad_arguments_keep_the_previous_skybox(renderer):
    W, Hh = 96, 64
    cam = orc.Camera(W, Hh, (0.0, 0.0, 1.0), (-2.0, 1.0, 1.3), [0, 0, 1])
    equi = smooth_panorama(64, 32)
    renderer.skybox_configure_equirect(equi, 32)
    before, faces = _render(renderer, cam, W, Hh), renderer.skybox_download()
    lib, h = renderer._lib, renderer._h
    p = equi.ctypes.data_as(C.c_void_p)
    for args in ((None, 64, 32, 32), (p, 0, 32, 32), (p, -1, 32, 32), (p, 32769, 32, 32), (p, 64, 0, 32), (p, 64, 32769, 32),
                 (p, 64, 32, 0), (p, 64, 32, -5), (p, 64, 32, 16385)):
        assert lib.gswt_skybox_configure_equirect(h, *args) == L.GSWT_ERR_BAD_ARG, args
        assert b"gswt_skybox_configure_equirect" in lib.gswt_last_error(h)
    assert lib.gswt_skybox_download(h, None) == L.GSWT_ERR_BAD_ARG
    np.testing.assert_array_equal(_render(renderer, cam, W, Hh), before)
    np.testing.assert_array_equal(renderer.skybox_download(), faces)


def test_download_before_any_configure():
    from gswt_renderer_amd.renderer import GSWTRenderer, GSWTError
    r = GSWTRenderer(0)
    try:
        with pytest.raises(GSWTError) as e:
            r.skybox_download()
        assert e.value.code == L.GSWT_ERR_STATE
    finally:
        r.close()
