"""The sun shadows without a GPU: tests/shadow_ref.py's two forms of the definition against each other and against hand-computed answers,
shadows.from_ortho_camera against the orthographic frame's own pixel and depth conventions, the packed block, the Python refusals."""
import ctypes as C
import struct

import numpy as np
import pytest

from gswt_renderer_amd import _lib as L
from gswt_renderer_amd import shadows
from tests import atmosphere_ref as AR
from tests import frame_modes as FM
from tests import ortho_ref as OR
from tests import shadow_ref as SR

F32 = np.float32


_unit_light = SR.unit_light


def test_definition_known_answers():
    Z = np.ones((4, 4), F32)
    Z[:, :2] = 0.25                                   # the two left columns shadow what lies below z = 1
    p = SR.params(_unit_light(Z, strength=0.5))
    pts = np.array([[2.5, 1.5, 0.0],                  # centre of a lit texel
                    [0.5, 1.5, 0.0],                  # centre of a shadowing texel, below its depth: fully shadowed
                    [0.5, 1.5, 1.5],                  # above its depth: lit
                    [2.0, 1.5, 0.0],                  # midway between a shadowing and a lit texel
                    [9.0, 1.5, 0.0],                  # outside the image
                    [0.5, 1.5, -3.0],                 # ld > 1
                    [0.5, 1.5, 3.0],                  # ld < 0
                    [-0.25, 1.5, 0.0],                # the image's edge: the texel past it counts as lit (wx = 0.25 of texel 0)
                    [np.nan, 1.5, 0.0]], F32)
    for look in (SR.lookup_f32, SR.lookup_f64):
        sh, lit, outside, _ = look([pts[:, 0], pts[:, 1], pts[:, 2]], p)
        assert list(lit) == [1.0, 0.0, 1.0, 0.5, 1.0, 1.0, 1.0, 0.75, 1.0]
        assert list(outside) == [False, False, False, False, True, True, True, False, True]
        assert list(sh) == [0.0, 0.5, 0.0, 0.25, 0.0, 0.0, 0.0, 0.125, 0.0]
    # a NaN texel is lit; the bias moves the compare
    Zn = Z.copy()
    Zn[:, 0] = np.nan
    assert SR.lookup_f32([pts[1:2, 0], pts[1:2, 1], pts[1:2, 2]], SR.params(_unit_light(Zn)))[1][0] == 1.0
    below = np.array([[0.5, 1.5, 1.0 - 0.125]], F32)                                 # ld = 0.28125: 0.03125 behind the texel
    for bias, lit in ((0.0, 0.0), (0.03125, 1.0), (0.0625, 1.0), (0.015625, 0.0)):   # r > Z is strict
        assert SR.lookup_f32([below[:, 0], below[:, 1], below[:, 2]], SR.params(_unit_light(Z, bias=bias)))[1][0] == lit
    # the shade: sh == 0 keeps the colour, otherwise one quantisation
    rgb = (np.array([[200, 100, 51]], F32) / F32(255.0)).repeat(3, 0)
    got = SR.shaded_rgb_f32(rgb, np.array([0.0, 0.5, 1.0], F32), SR.params(_unit_light(Z, shade_color=(0.0, 0.0, 1.0))))
    assert np.array_equal(AR.bytes_of(got), [[200, 100, 51], [100, 50, 153], [0, 0, 255]])
    assert FM.bits_equal(got[0].copy(), rgb[0].copy())


def test_f32_and_f64_forms_agree_on_the_plane_case():
    cam = SR.plane_light()
    m = shadows.from_ortho_camera(cam, SR.plane_map(cam), bias=0.002, strength=0.75, shade_color=(0.1, 0.05, 0.2))
    p = SR.params(m)
    g, _, su, _, _ = FM.view("case_plane", "top")
    c = SR.centres_f32(su, g["pp"].tex, g["draws"])
    s32, _, o32, (u32, v32, d32) = SR.lookup_f32(c, p)
    s64, _, o64, (u64, v64, d64) = SR.lookup_f64(c, p)
    assert c[0].shape[0] == 510 and np.array_equal(o32, o64)
    assert np.abs(u32 - u64).max() < 1e-4 and np.abs(v32 - v64).max() < 1e-4 and np.abs(d32 - d64).max() < 1e-6
    # away from a texel's depth and a texel boundary the two agree to the weights' rounding
    agree = np.abs(s32.astype(np.float64) - s64) < 1e-4
    assert agree.mean() > 0.98
    lit, dark, between = SR.shares(s32, p)
    assert min(lit, dark, between) >= 0.2


@pytest.mark.parametrize("which", ["top", "oblique"])
def test_from_ortho_camera_matches_the_frames_pixels_and_depth(which):
    g = OR.golden()
    cam = FM.ortho_cam(which, g)
    blk = cam.uniforms()
    M = shadows.world_to_light(cam)
    assert M.dtype == F32 and tuple(M[[3, 7, 11, 15]]) == (0.0, 0.0, 0.0, 1.0)
    Mr = M.astype(np.float64).reshape(4, 4).T
    rng = np.random.default_rng(5)
    xs, ys = rng.integers(0, cam.width, 200), rng.integers(0, cam.height, 200)
    depth = rng.uniform(0.0, 1.0, 200)
    ndc = np.stack([(xs + 0.5) / cam.width * 2.0 - 1.0, 1.0 - (ys + 0.5) / cam.height * 2.0], 1)
    pos, _ = AR.unproject_f64(blk, ndc, depth)                      # the world points the frame puts at those pixel centres
    l = Mr @ np.vstack([pos.T, np.ones(200)])
    u = (l[0] * 0.5 + 0.5) * cam.width - 0.5
    v = (0.5 - l[1] * 0.5) * cam.height - 0.5
    assert np.abs(u - xs).max() <= 1e-4 and np.abs(v - ys).max() <= 1e-4
    assert np.abs(l[2] - depth).max() <= 1e-6
    m = shadows.from_ortho_camera(cam, np.ones((cam.height, cam.width), F32))
    assert (m.width, m.height) == (cam.width, cam.height) and not m.on_device
    with pytest.raises(ValueError):
        shadows.from_ortho_camera(cam, np.ones((cam.width, cam.height), F32))


def test_block_packing():
    Z = np.ones((3, 5), F32)
    m = _unit_light(Z, bias=0.25, strength=0.5, shade_color=(0.125, 0.25, 0.75))
    raw = bytes(m)
    assert len(raw) == shadows.BLOCK_BYTES == 96 == C.sizeof(L.ShadowParams)
    s = L.ShadowParams.from_buffer_copy(raw)
    assert [L.ShadowParams.world_to_light.offset, L.ShadowParams.bias.offset, L.ShadowParams.strength.offset, L.ShadowParams.shade_color.offset,
            L.ShadowParams._pad.offset] == [0, 64, 68, 72, 84]
    assert list(s.world_to_light) == [float(x) for x in m.world_to_light] and s.world_to_light[0] == 0.4000000059604645
    assert (s.bias, s.strength, list(s.shade_color), list(s._pad)) == (0.25, 0.5, [0.125, 0.25, 0.75], [0, 0, 0])
    assert struct.unpack("<3I", raw[84:]) == (0, 0, 0)
    assert (m.width, m.height) == (5, 3) and m.depth_ptr() == m.depth.ctypes.data
    assert shadows.OFF.is_off and len(bytes(shadows.OFF)) == 96 and not m.is_off
    assert "gswt_set_shadow_map" in L.SYMBOLS


def test_python_refusals():
    Z = np.ones((4, 4), F32)
    ok = _unit_light(Z).world_to_light
    nan, inf = float("nan"), float("inf")
    bad_m = ok.copy(); bad_m[3] = 0.5
    nan_m = ok.copy(); nan_m[5] = nan
    for kw in (dict(bias=-0.1), dict(bias=nan), dict(bias=inf), dict(strength=0.0), dict(strength=1.5), dict(strength=nan),
               dict(shade_color=(0.0, 1.5, 0.0)), dict(shade_color=(0.0, nan, 0.0)), dict(shade_color=(0.0, 0.0)),
               dict(shade_color=(-0.1, 0.0, 0.0))):
        with pytest.raises(ValueError):
            shadows.ShadowMap(ok, Z, **kw)
    for m, z in ((bad_m, Z), (nan_m, Z), (ok[:12], Z), (ok, Z.astype(np.float64)), (ok, np.ones(16, F32)), (ok, np.ones((0, 4), F32)),
                 (ok, np.ones((1, 4097), F32)), (ok, np.ones((4097, 1), F32))):
        with pytest.raises(ValueError):
            shadows.ShadowMap(m, z)
    with pytest.raises(ValueError):
        shadows.ShadowMap(ok, None)
    # the edges of the ranges are accepted
    shadows.ShadowMap(ok, np.ones((1, 4096), F32), bias=0.0, strength=1.0, shade_color=(0.0, 1.0, 1.0))
