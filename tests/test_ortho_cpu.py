"""Orthographic cameras (gswt_renderer_amd/ortho.py) and the CPU references of the orthographic vertex stage (tests/ortho_ref.py),
without a GPU.

The camera blocks of ortho.py equal the independently built ones bit for bit; top_down maps z_top to depth 0 and z_bottom to depth 1
and height_from_depth inverts it; the float32 restatement of the vertex stage (a) agrees with the oracle on every output that does
not depend on the Jacobian and with the analytic float64 covariance (b) on the axes; and the image reference of the GPU tests --
depth_ref.composite over (a)'s records -- agrees with a float64 evaluation of the same blend on all but a quarter of the pixel cap
the GPU tests allow, so the reference alone does not eat that cap."""
import os
import re

import numpy as np
import pytest

from gswt_renderer_amd import _lib as L
from gswt_renderer_amd import ortho
from oracle import gswt_oracle as orc
from tests import depth_ref as DR
from tests import ortho_ref as OR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-4                  # tests/test_depth_out_gpu.py: colour parity tolerance ...
PIXEL_CAP = 2e-3            # ... except on at most this share of the pixels
U = OR.U


@pytest.mark.parametrize("which", OR.CAMERAS)
def test_uniforms_equal_the_independent_block(which):
    g = OR.golden()
    for lod_pos in (None, g["pos"]):
        args = OR.camera_args(which, lod_pos=lod_pos)
        cam = OR.ortho_camera_of(args)
        got, want = bytes(cam.uniforms()), bytes(OR.block_of(args))
        assert len(got) == 176 and got == want
        cu = cam.uniforms()
        assert list(cu.htan_fov) == [0.0] * 4 and [cu.projection[k] for k in (3, 7, 11, 15)] == [0.0, 0.0, 0.0, 1.0]
        # pixels per world unit: the frame spans 2 half_width x 2 half_height world units
        assert abs(cu.focal[0] - OR.W / (2 * cam.half_width)) <= 4 * U * cu.focal[0]
        assert abs(cu.focal[1] - OR.H / (2 * cam.half_height)) <= 4 * U * cu.focal[1]
        assert cam.half_width == cam.half_height * OR.W / OR.H
        want_pos = np.asarray(cam.eye if lod_pos is None else lod_pos, np.float64).astype(np.float32)
        assert np.array_equal(np.array(list(cu.cam_pos)[:3], np.float32), want_pos)
        assert np.array_equal(cam.view_proj(), orc.mat4_mul(cam.projection, cam.view))


def _depth_f64(cu, p):
    """NDC depth of world point p through the block's binary32 matrices, evaluated in float64."""
    V = np.array(list(cu.view), np.float64).reshape(4, 4).T
    P = np.array(list(cu.projection), np.float64).reshape(4, 4).T
    q = P @ (V @ np.array([p[0], p[1], p[2], 1.0]))
    return (0.5 * q[2] + 0.5 * q[3]) / q[3], q


@pytest.mark.parametrize("z_top,z_bottom", [(25.0, -0.5), (3.0, -1.0), (1.7, 0.3), (-2.0, -9.5)])
def test_top_down_maps_heights_to_depth(z_top, z_bottom):
    cam = ortho.top_down((4.0, 6.0), 6.0, z_top, z_bottom, OR.W, OR.H)
    cu = cam.uniforms()
    rng = z_top - z_bottom
    # the binary32 matrix elements carry one rounding each: V[14] = fl(z_top) moves the view depth by u |z_top|, P[10] = fl(-2 / range)
    # scales the depth by (1 + u); the evaluation below is binary64
    bound = 2 * U * (1.0 + abs(z_top) / rng)
    d0, q0 = _depth_f64(cu, (4.0, 6.0, z_top))
    d1, _ = _depth_f64(cu, (4.0, 6.0, z_bottom))
    assert abs(d0) <= bound and abs(d1 - 1.0) <= bound, (d0, d1, bound)
    assert abs(q0[0]) <= 4 * U and abs(q0[1]) <= 4 * U and q0[3] == 1.0          # the map centre is the image centre
    # world +y is up the image, +x to the right
    _, qy = _depth_f64(cu, (4.0, 6.0 + cam.half_height, z_top))
    _, qx = _depth_f64(cu, (4.0 + cam.half_width, 6.0, z_top))
    assert abs(qy[1] - 1.0) <= 4 * U and abs(qx[0] - 1.0) <= 4 * U and abs(qy[0]) <= 4 * U and abs(qx[1]) <= 4 * U
    # height_from_depth inverts the mapping (binary64: one product, one difference)
    assert ortho.height_from_depth(cam, 0.0) == z_top
    assert abs(ortho.height_from_depth(cam, 1.0) - z_bottom) <= 2.0 ** -52 * (abs(z_top) + rng)
    for zz in (z_bottom + 0.25 * rng, z_bottom + 0.6 * rng):
        d, _ = _depth_f64(cu, (1.0, 2.0, zz))
        assert abs(ortho.height_from_depth(cam, d) - zz) <= bound * rng
    with pytest.raises(ValueError):
        ortho.height_from_depth(OR.ortho_camera_of(OR.camera_args("oblique")), 0.5)


@pytest.mark.parametrize("which", OR.CAMERAS)
def test_float32_stage_agrees_with_the_oracle_where_the_jacobian_plays_no_part(which):
    """ndc, depth and rgba do not depend on the Jacobian, so the oracle's perspective code yields them for an orthographic matrix too:
    (a) must reproduce them bit for bit.  (The oracle's `visible` does not include the fragment setup's axis test.)"""
    g = OR.golden()
    cu, su, sp = OR.plane_records(which)
    want = orc.project_draws(cu, su, g["pp"].tex, g["draws"])
    both = (sp["visible"] == 1) & (want["visible"] == 1)
    assert both.sum() > 300 and not ((sp["visible"] == 1) & (want["visible"] == 0)).any()
    for fld in ("ndc", "depth", "rgba"):
        assert np.array_equal(sp[fld][both].view(np.uint32), want[fld][both].view(np.uint32)), fld
    # all three draw classes take part (plain, blending, merged group), and the LOD blend fades some splats
    classes = {(d.tile.single_draw, d.tile.changing) for d in g["draws"]}
    assert {(0, 0), (0, 1), (1, 1)} <= classes


@pytest.mark.parametrize("which", OR.CAMERAS)
def test_axes_agree_with_the_analytic_covariance(which):
    """(a)'s major / minor axes against those of (b), cov2d = J Sigma J^T in binary64, through the shader's own eigen formulas.

    The bound, per splat, by first-order propagation of the binary32 chain's roundings (u = 2^-24):
      cov2d:  an entry is sum_k sum_l T[k] K[k][l] T[l].  T = transpose(view3) * J_T carries 1 rounding (its other products are with the
              zeros of J_T), A = transpose(T) * K adds 3 (a product and two sums per term), cov2d = A * T another 3 and T's rounding
              again: 8 roundings on any path, so |d c_ij| <= 9 u (|T|^T |K| |T|)_ij  =: dc_ij  (gamma_8 < 9 u; S = 1 here).
      mid, hxx = 0.5 (c00 +- c11): d <= 0.5 (dc00 + dc11) + u |.|.      radius = sqrt(hxx^2 + c01^2): the gradient has norm <= 1 in
              (hxx, c01), two squares, a sum and a root add <= 3 u radius:  d_rad <= d_hxx + dc01 + 3 u radius.
      l1, l2 = mid +- radius:  d_l <= d_mid + d_rad + u |l|.
      s = min(sqrt(2 l), 1024):  d_s <= sqrt(2 (l + d_l)) - sqrt(2 max(l - d_l, 0)) + 2 u s   (monotone; min is 1-Lipschitz).
      v = (c01, l1 - c00):  d_v <= dc01 + d_l1 + dc00 + u |vy|;   e = v / |v|:  |d e| <= 2 d_v / |v| + 4 u  (normalisation of a
              perturbed vector; two squares, sum, root, quotient), capped at 2 (unit vectors).
      axis = s e:  |d axis| <= d_s + s d_e + u s.
    The bound grows where the shader's formulas are ill-conditioned (l2 = mid - radius cancels on thin ellipses, v cancels on
    axis-aligned ones): that is their conditioning, not slack -- and most splats must be well inside it (last assertion)."""
    g = OR.golden()
    cu, su, sp = OR.plane_records(which)
    cov, cabs = OR.cov2d_f64(cu, su, g["pp"].tex, g["draws"])
    major, minor, p = OR.axes_f64(cov)
    vis = sp["visible"] == 1
    dc = 9 * U * cabs
    d_mid = 0.5 * (dc[:, 0] + dc[:, 2]) + U * np.abs(0.5 * (cov[:, 0] + cov[:, 2]))
    d_hxx = 0.5 * (dc[:, 0] + dc[:, 2]) + U * np.abs(0.5 * (cov[:, 0] - cov[:, 2]))
    d_rad = d_hxx + dc[:, 1] + 3 * U * p["radius"]
    d_l1 = d_mid + d_rad + U * np.abs(p["l1"])
    d_l2 = d_mid + d_rad + U * np.abs(p["l2"])

    def d_root(l, dl, s):
        return np.sqrt(2 * (np.maximum(l, 0) + dl)) - np.sqrt(2 * np.maximum(l - dl, 0)) + 2 * U * s
    d_smaj, d_smin = d_root(p["l1"], d_l1, p["smaj"]), d_root(p["l2"], d_l2, p["smin"])
    d_v = dc[:, 1] + d_l1 + dc[:, 0] + U * np.abs(p["vy"])
    with np.errstate(all="ignore"):
        d_e = np.minimum(2 * d_v / p["vlen"] + 4 * U, 2.0)
    b_maj = d_smaj + p["smaj"] * d_e + U * p["smaj"]
    b_min = d_smin + p["smin"] * d_e + U * p["smin"]
    e_maj = np.abs(sp["major"].astype(np.float64) - major).max(axis=1)
    e_min = np.abs(sp["minor"].astype(np.float64) - minor).max(axis=1)
    print(f"{which}: {int(vis.sum())} visible, max axis error {e_maj[vis].max():.3e} / {e_min[vis].max():.3e}, median bound "
          f"{np.median(b_maj[vis]):.3e} / {np.median(b_min[vis]):.3e}, median |major| {np.median(p['smaj'][vis]):.3e}")
    assert vis.sum() > 300
    assert (e_maj[vis] <= b_maj[vis]).all() and (e_min[vis] <= b_min[vis]).all()
    # not vacuous: for nine splats in ten the bound is a small fraction of the axis itself -- 2^-12, the square root of u: what is left of
    # binary32 when half the digits cancel
    tight = (b_maj[vis] <= 2.0 ** -12 * p["smaj"][vis]) & (b_min[vis] <= 2.0 ** -12 * p["smaj"][vis])
    assert tight.mean() >= 0.9, float(tight.mean())
    # the analytic form itself: an isotropic covariance sigma^2 I projects to sigma^2 diag(fx^2, fy^2) whatever the view direction
    iso, _ = OR.cov2d_f64(cu, su, _iso_tex(0.25), [orc.Draw(orc.tile_uniforms(), np.zeros(1, np.uint32))])
    fx, fy = cu.focal[0], cu.focal[1]
    assert np.allclose(iso[0], [0.25 * fx * fx, 0.0, 0.25 * fy * fy], rtol=1e-6, atol=1e-6 * fx * fx)


def _iso_tex(var):
    h = orc.float_to_half(var)
    rec = np.zeros((1, 8), np.uint32)
    rec[0, 4], rec[0, 5], rec[0, 6] = h, h << 16, h << 16          # K = diag(var): halves a | b << 16, c | d << 16, e | f << 16
    return rec


IMAGE_CASES = [(w, o, b, s) for w in OR.CAMERAS for o in (0, 1) for b in (False, True) for s in (OR.SPLAT_SCALE,)] + \
              [(w, 1, True, OR.SPLAT_SCALE_DENSE) for w in OR.CAMERAS]


@pytest.mark.parametrize("which,order_mode,bg,splat_scale", IMAGE_CASES)
def test_image_reference_against_float64_blend(which, order_mode, bg, splat_scale):
    """depth_ref.composite over (a)'s records (binary32, the fragment sequence F1..F4) against the same blend in binary64: beyond TOL
    on at most a quarter of the GPU tests' pixel cap.  And the frame is a real test image: most of it covered, pixels under several
    splats, some splats behind the proxy depth."""
    cu, su, sp = OR.plane_records(which, splat_scale)
    bgc, bgd = DR.bg_images(OR.W, OR.H) if bg else (None, None)
    img, z, n_cover = DR.composite(sp, OR.W, OR.H, splat_scale=splat_scale, order_mode=order_mode, bg_rgba=bgc, bg_depth=bgd, with_cover=True)
    img64, z64 = OR.composite_f64(sp, OR.W, OR.H, splat_scale=splat_scale, order_mode=order_mode, bg_rgba=bgc, bg_depth=bgd)
    bad = (np.abs(img.astype(np.float64) - img64) > TOL).any(axis=-1)
    dz = np.abs(z.astype(np.float64) - z64)
    print(f"{which} order={order_mode} bg={bg} scale={splat_scale}: covered {float((n_cover > 0).mean()):.3f}, deepest pixel {int(n_cover.max())}, "
          f"beyond TOL {int(bad.sum())} px, max colour diff {np.abs(img - img64).max():.3e}, max depth diff {dz[~bad].max():.3e}")
    assert bad.sum() <= 0.25 * PIXEL_CAP * OR.W * OR.H
    assert dz[~bad].max() <= 1e-5
    assert (n_cover > 0).mean() > 0.5 and n_cover.max() >= 8
    vis = sp["visible"] == 1
    assert vis.sum() > 300 and (sp["depth"][vis] > 0.9).all()
    if bg:
        assert (sp["depth"][vis] < bgd.min()).any() and (sp["depth"][vis] > bgd.min()).any()


def test_option_constant_matches_the_header():
    hdr = open(os.path.join(ROOT, "include", "gswt_hip.h")).read()
    assert int(re.search(r"GSWT_OPT_PROJECTION\s*=\s*(\d+)", hdr).group(1)) == L.GSWT_OPT_PROJECTION == 17
    assert (L.GSWT_PROJECTION_PERSPECTIVE, L.GSWT_PROJECTION_ORTHO) == (0, 1)
