"""The skybox bake restatement (tests/skybox_bake_ref.py) against independent constructions and known answers, and the
bake's entry points in the C ABI and the Python wrapper (no GPU needed)."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import skybox_bake_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("n", [1, 7, 64])
def test_texel_directions_equal_the_unprojected_pixel_rays(n):
    """The bake ray of every texel == the segment between the texel's NDC point unprojected through inverse(P * V_i) on
    the near plane and on the far plane (OpenGL clip space of cgmath's perspective: z_ndc = -1 / +1)."""
    yy, xx = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    nx, ny = R.texel_ndc(yy, xx, n)
    for face in range(6):
        inv = np.linalg.inv(R.bake_projection() @ R.bake_view(face))
        pts = []
        for z in (-1.0, 1.0):
            q = np.stack([nx, ny, np.full_like(nx, z), np.ones_like(nx)], -1) @ inv.T
            pts.append(q[..., :3] / q[..., 3:])
        ray = pts[1] - pts[0]
        ray /= np.linalg.norm(ray, axis=-1, keepdims=True)
        np.testing.assert_allclose(R.texel_dirs(face, yy, xx, n), ray, rtol=0, atol=1e-6)


def test_look_at_matches_the_face_table():
    """cgmath look_at_rh of skybox.rs:584-617: each face looks along its target (the +Z face down -Z, as written)."""
    fwd = [-R.bake_view(f)[2, :3] for f in range(6)]
    np.testing.assert_array_equal(np.array(fwd), np.array([t for t, _ in R.BAKE_VIEWS]))
    for f in range(6):
        m = R.bake_view(f)[:3, :3]
        np.testing.assert_allclose(m @ m.T, np.eye(3), atol=1e-15)
        assert np.linalg.det(m) == pytest.approx(1.0)


@pytest.mark.parametrize("n", [1, 7, 65])
def test_centre_of_the_plus_x_face_samples_the_panorama_centre(n):
    c = n // 2
    u, v = R.sample_spherical_map(R.texel_dirs(0, c, c, n))
    assert u == pytest.approx(0.5, abs=1e-15) and v == pytest.approx(0.5, abs=1e-15)


def test_constant_panorama_bakes_to_the_tone_mapped_constant():
    c = np.array([0.25, 1.0, 6.5], np.float32)
    equi = np.empty((9, 17, 4), np.float32)
    equi[..., :3] = c
    equi[..., 3] = -3.0                                       # the panorama's alpha is ignored (skybox.wgsl:84)
    out = R.bake(equi, 7)
    want = (c.astype(np.float64) / (c + 1.0)) ** np.float64(np.float32(1.0 / 2.2))
    np.testing.assert_allclose(out[..., :3], np.broadcast_to(want, out[..., :3].shape), rtol=0, atol=1e-15)
    assert np.all(out[..., 3] == 1.0)


def test_seam_samples_the_last_two_and_the_first_two_columns():
    """u = phi * 0.1591 + 0.5 spans [0.00017, 0.99983]: at w = 4096, phi = +pi lands at x = u * w - 0.5 = 4094.79 (between
    columns w-2 and w-1), phi = -pi at x = 0.21 (columns 0 and 1).  1 / (2 pi) would put both on the wrap pair (w-1, 0)."""
    w = 4096
    for z, want in ((0.0, 4094.793), (-0.0, 0.207)):             # atan2(+0, -1) = +pi, atan2(-0, -1) = -pi
        u, _ = R.sample_spherical_map(np.array([-1.0, 0.0, z]))
        assert u * w - 0.5 == pytest.approx(want, abs=1e-3)
        a, b, t = R.bilinear_taps(u, w)
        assert (int(a), int(b)) == ((w - 2, w - 1) if want > 1 else (0, 1))
        assert t == pytest.approx(want % 1.0, abs=1e-3)
    # through the whole bake: the centre column of the -X face at odd n is d = (-1, y, +0), phi = +pi on every row; of the
    # panorama's marked wrap pair only column w-1 (green) is mixed in, never column 0 (red)
    h, n = 8, 65
    equi = np.full((h, w, 4), 0.5, np.float32)
    equi[:, 0, :3], equi[:, w - 1, :3] = (8.0, 0.5, 0.5), (0.5, 8.0, 0.5)
    seam = R.bake_texels(equi, 1, np.arange(n), n // 2, n)[:, :3]
    lo, mix = R.tone_map(np.float64(0.5)), R.tone_map(np.float64(0.5 * (1 - 0.793) + 8.0 * 0.793))
    np.testing.assert_allclose(seam[:, 0], lo, rtol=0, atol=1e-12)
    np.testing.assert_allclose(seam[:, 1], mix, rtol=0, atol=2e-3)


def test_poles_sample_between_the_last_and_the_first_row():
    """v = theta * 0.3183 + 0.5: at h = 2048 the north pole lands at y = 2047.468 and the south pole at y = -0.468, both
    between rows h-1 and 0 (Repeat) with weight 0.468 / 0.532 on the second row; 1 / pi would give 2047.5 / -0.5."""
    h = 2048
    for dy, want in ((1.0, 2047.468), (-1.0, -0.468)):
        _, v = R.sample_spherical_map(np.array([0.0, dy, 0.0]))
        assert v * h - 0.5 == pytest.approx(want, abs=1e-3)
        a, b, t = R.bilinear_taps(v, h)
        assert (int(a), int(b)) == (h - 1, 0)
        assert t == pytest.approx(want % 1.0, abs=1e-3)


def test_library_exports_the_bake_and_the_download():
    lib = C.CDLL(os.path.join(ROOT, "gswt_renderer_amd", "lib", "libgswt_hip.so"))
    assert hasattr(lib, "gswt_skybox_configure_equirect") and hasattr(lib, "gswt_skybox_download")


def test_renderer_has_the_bake_and_the_download():
    from gswt_renderer_amd.renderer import GSWTRenderer
    assert callable(getattr(GSWTRenderer, "skybox_configure_equirect", None))
    assert callable(getattr(GSWTRenderer, "skybox_download", None))
