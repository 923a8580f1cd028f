"""The atmosphere's CPU side: tests/atmosphere_ref.py's known values, the Atmosphere dataclass's 32-byte block, and the conditions the GPU
tests (tests/test_atmosphere_gpu.py) rely on, checked for the reference alone with the parameters those tests use."""
import struct

import numpy as np
import pytest

from gswt_renderer_amd import atmosphere as A
from gswt_renderer_amd import host
from oracle import gswt_oracle as orc
from tests import atmosphere_ref as AR
from tests import ortho_ref as OR

F32 = np.float32
FADE = (4.0, 8.0)
FOG = (0.15, 2.0, 0.9, (0.62, 0.71, 0.80))


def _persp(g):
    return host.camera_uniforms(g["pos"], g["tgt"], (0, 0, 1), 45.0, 0.1, 2400.0, OR.W, OR.H)[0]


def _unfaded(name):
    g = OR.golden(name)
    cu, su = _persp(g), OR.scene_of(g)
    cam = orc.Camera176.from_buffer_copy(bytes(cu))
    return g, cam, su, orc.project_draws(cam, su, g["pp"].tex, g["draws"], height_map=g["hm"])


# ---- the dataclass ----------------------------------------------------------------------------------------------------------------
def test_block_is_32_bytes_in_field_order():
    a = A.Atmosphere(fade=(1.5, 2.5), fog=(0.25, 3.0, 0.75, (0.125, 0.5, 1.0)))
    b = a.pack()
    assert len(b) == A.BLOCK_BYTES == 32 and bytes(a) == b
    assert struct.unpack("<8f", b) == (1.5, 2.5, 0.25, 3.0, 0.75, 0.125, 0.5, 1.0)
    assert struct.unpack("<8f", A.Atmosphere(fade=(1.5, 2.5)).pack()) == (1.5, 2.5, 0, 0, 0, 0, 0, 0)
    assert struct.unpack("<8f", A.Atmosphere(fog=(0.25, 3.0, 0.75, (0.125, 0.5, 1.0))).pack()) == (0, 0, 0.25, 3.0, 0.75, 0.125, 0.5, 1.0)
    with pytest.raises(ValueError):
        A.Atmosphere(fog=(0.25, 3.0, 0.75, (0.125, 0.5))).pack()


def test_off_is_all_zero():
    assert A.OFF.pack() == bytes(32) and A.OFF == A.Atmosphere()
    p = AR.params(A.OFF)
    assert not p["fade_on"] and not p["fog_on"]


def test_symbol_is_declared():
    from gswt_renderer_amd import _lib
    assert "gswt_set_atmosphere" in _lib.SYMBOLS


# ---- known values of the reference --------------------------------------------------------------------------------------------------
def test_fade_known_values():
    p = AR.params(A.Atmosphere(fade=(5.0, 10.0)))
    assert p["fade_inv"] == F32(0.2)
    t, fs = AR.fade_f32(np.array([5.0, 7.5, 10.0, 15.0, 2.5, np.nan, np.inf], F32), p)
    assert t.dtype == F32 and fs.dtype == F32
    assert list(t[:5]) == [1.0, 0.5, 0.0, 0.0, 1.0] and list(fs[:5]) == [1.0, 0.5, 0.0, 0.0, 1.0]       # t = 0.5 -> fs = 0.5 exactly
    assert t[5] == 0.0 and t[6] == 0.0                                                                   # a NaN dist clamps to 0
    t64, fs64 = AR.fade_f64(np.array([6.25]), p)
    assert t64[0] == pytest.approx(0.75) and fs64[0] == pytest.approx(0.75 * 0.75 * 1.5)
    # the smoothstep's slope never exceeds 1.5
    tt = np.linspace(0.0, 1.0, 10001)
    assert np.max(np.diff(tt * tt * (3 - 2 * tt)) / np.diff(tt)) <= 1.5


def test_fog_known_values():
    p = AR.params(A.Atmosphere(fog=FOG))
    d = np.array([0.0, 1.0, 2.0, 2.0 + 1.0 / 0.15, 1e9])
    F = AR.fog_amount_f64(d, p)
    assert F[0] == 0.0 and F[1] == 0.0 and F[2] == 0.0                                                  # fog_start >= dist -> F = 0
    assert F[3] == pytest.approx(0.9 * (1.0 - np.exp(-1.0)), rel=1e-6) and F[4] == pytest.approx(0.9, rel=1e-6)
    rgb = np.array([[0.2, 0.4, 0.6]] * 5)
    codes = AR.fog_codes_f64(rgb, d, p)
    assert np.allclose(codes[0], 255.0 * rgb[0], atol=1e-9)
    assert np.allclose(codes[4], 255.0 * (0.1 * rgb[0] + 0.9 * p["fog_color"].astype(np.float64)), atol=1e-4)
    want, near_half = AR.fog_bytes(np.array([[10.5004, 10.4, 200.4985]]))
    assert list(want[0]) == [11.0, 10.0, 200.0] and list(near_half[0]) == [True, False, False]
    # fog_density 1e6, fog_max 1: every colour is the fog colour
    q = AR.params(A.Atmosphere(fog=(1e6, 0.0, 1.0, FOG[3])))
    assert np.array_equal(np.rint(AR.fog_codes_f64(rgb[:1], np.array([2.5]), q)), np.rint(255.0 * q["fog_color"].astype(np.float64))[None])


def test_unprojection_inverts_the_projection():
    g, cam, su, sp = _unfaded("case_plane")
    vis = sp["visible"] == 1
    exact = AR.dist_f32(cam.cam_pos, su, g["pp"].tex, g["draws"]).astype(np.float64)[vis]
    got, z = AR.dist_f64(cam, sp["ndc"][vis], sp["depth"][vis])
    near = AR.near_of(cam)
    assert near == pytest.approx(0.1, rel=1e-5)
    # the unprojected distance is within the docstring's depth-quantisation bound of the exact one
    bound = AR.DEPTH_ROUNDINGS * z * z / near * AR.U + 4 * AR.U * exact
    print(f"max |unprojected - exact| / bound {np.max(np.abs(got - exact) / bound):.3f}, max |.| {np.max(np.abs(got - exact)):.3e}")
    assert (np.abs(got - exact) <= bound).all()


# ---- the conditions the GPU tests rely on ---------------------------------------------------------------------------------------------
def test_plane_case_ramp_counts():
    """case_plane, eye at the case's pos, fade = (4, 8): of the 510 instances 110 land at t = 0, 92 at t = 1 and 308 inside the ramp."""
    g, cam, su, sp = _unfaded("case_plane")
    dist = AR.dist_f32(cam.cam_pos, su, g["pp"].tex, g["draws"])
    assert dist.shape[0] == sp.shape[0] == 510
    t, fs = AR.fade_f32(dist, AR.params(A.Atmosphere(fade=FADE)))
    assert (int((t == 0).sum()), int((t == 1).sum()), int(((t > 0) & (t < 1)).sum())) == (110, 92, 308)
    vis = sp["visible"] == 1
    assert ((t > 0) & (t < 1) & vis).sum() > 100 and ((t == 0) & vis).sum() > 20
    # the orthographic cameras fade around the same point (cam_pos = the LOD transition's reference point)
    for which in OR.CAMERAS:
        cu = OR.block_of(OR.camera_args(which, lod_pos=g["pos"]))
        assert np.array_equal(AR.dist_f32(cu.cam_pos, su, g["pp"].tex, g["draws"]), dist)


@pytest.mark.parametrize("name", ["case_hmap", "case_sphere"])
def test_surface_ramps_and_masked_share(name):
    """The percentile ramp of the surface cases: at least 25 % of the visible splats strictly inside, at least 10 % on each side, and
    fewer than 2 % within the derived tolerance of t = 0."""
    g, cam, su, sp = _unfaded(name)
    vis = sp["visible"] == 1
    assert vis.sum() > 100
    dist, z = AR.dist_f64(cam, sp["ndc"][vis], sp["depth"][vis])
    p = AR.params(A.Atmosphere(fade=AR.ramp_from_percentiles(dist)))
    tol = AR.surface_t_tol(z, AR.near_of(cam), p)
    inside, at_one, at_zero, masked = AR.ramp_shares(dist, p, tol)
    print(f"{name}: ramp {float(p['fade_start']):.4f} .. {float(p['fade_end']):.4f}, inside {inside:.3f}, t = 1 {at_one:.3f}, t = 0 {at_zero:.3f}, "
          f"masked {masked:.4f}, largest tolerance on t {tol.max():.3e}")
    assert inside >= 0.25 and at_one >= 0.10 and at_zero >= 0.10
    assert masked <= AR.MAX_MASKED
    assert tol.max() < 1e-2                                   # the tolerance still tells a wrong ramp from a right one


@pytest.mark.parametrize("name", ["case_plane", "case_hmap", "case_sphere"])
def test_fog_margin_share_and_effect(name):
    """fog = (0.15, 2.0, 0.9, (0.62, 0.71, 0.80)): at most 2 % of the reference's channels lie within FOG_MARGIN of a half-integer, and
    most bytes change, so an unfogged frame cannot pass."""
    g, cam, su, sp = _unfaded(name)
    vis = sp["visible"] == 1
    if name == "case_plane":
        dist = AR.dist_f32(cam.cam_pos, su, g["pp"].tex, g["draws"]).astype(np.float64)[vis]
    else:
        dist, _ = AR.dist_f64(cam, sp["ndc"][vis], sp["depth"][vis])
    codes = AR.fog_codes_f64(sp["rgba"][vis][:, :3], dist, AR.params(A.Atmosphere(fog=FOG)))
    want, near_half = AR.fog_bytes(codes)
    changed = float((want != AR.bytes_of(sp["rgba"][vis])).mean())
    print(f"{name}: {int(vis.sum())} visible, {near_half.mean():.4%} of the channels inside the margin, {changed:.2%} of the bytes change")
    assert near_half.mean() <= AR.MAX_MASKED
    assert changed > 0.9
