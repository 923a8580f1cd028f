"""CPU references of the orthographic vertex stage (GSWT_OPT_PROJECTION = 1, include/gswt_hip.h), in numpy.

(a) project_ortho_f32: vs_main (gswt.wgsl:27-422) on the plain surface with the affine Jacobian in place of gswt.wgsl:213-232,
    restated operator by operator in np.float32 -- one rounding per written `*` `+` `-` `/` and sqrt, products and sums in the written
    order, no fused multiply-add (numpy's element-wise float32 operations are single IEEE operations).  The GPU's per-splat outputs
    are compared with it bit for bit, and so is the C oracle's orthographic mode (oracle.frame_mode(ortho=1), which came later and
    also covers the mapped surfaces: tests/test_pair_list_modes_cpu.py).
(b) cov2d_f64: the same 2 x 2 covariance from the analytic J Sigma J^T in float64, with a per-entry bound of the float32 chain's
    rounding error.  It anchors (a): a slip in (a)'s index juggling shows there, not only as "GPU differs".
(c) composite_f64: the blend of tests/depth_ref.py evaluated in float64 from the same records.

The cameras are built here from eye, target and extents (float64, rounded to float32 once per element), independently of
gswt_renderer_amd/ortho.py; tests/test_ortho_cpu.py compares the two bit for bit."""
from __future__ import annotations

import math

import numpy as np

from oracle import gswt_oracle as orc

F32 = np.float32
W, H = 72, 40             # 5 x 3 screen tiles, partial on the right and bottom edges
U = 2.0 ** -24            # unit roundoff of binary32


# ---- cameras ------------------------------------------------------------------------------------------------------------------------
def _unit(v):
    n = math.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])
    return (v[0] / n, v[1] / n, v[2] / n)


def _cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def _dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def camera_block(width, height, eye, target, up, half_height, near, far, lod_pos=None) -> orc.Camera176:
    """The 176-byte block of an orthographic camera: look-at view (the camera looks down its -z), OpenGL `ortho` projection,
    focal = pixels per world unit (|0.5 P[0][0] W|, |0.5 P[1][1] H| in binary32), htan_fov = 0, cam_pos = lod_pos or eye."""
    eye = tuple(float(x) for x in eye)
    fwd = _unit(tuple(float(t) - e for t, e in zip(target, eye)))
    side = _unit(_cross(fwd, tuple(float(x) for x in up)))
    upv = _cross(side, fwd)
    view = np.zeros((4, 4), np.float64)          # [column, row]
    for c in range(3):
        view[c] = (side[c], upv[c], -fwd[c], 0.0)
    view[3] = (-_dot(side, eye), -_dot(upv, eye), _dot(fwd, eye), 1.0)
    half_width = float(half_height) * int(width) / int(height)
    proj = np.zeros((4, 4), np.float64)
    proj[0, 0] = 1.0 / half_width
    proj[1, 1] = 1.0 / float(half_height)
    proj[2, 2] = -2.0 / (float(far) - float(near))
    proj[3, 2] = -(float(far) + float(near)) / (float(far) - float(near))
    proj[3, 3] = 1.0
    v32, p32 = view.astype(F32).reshape(16), proj.astype(F32).reshape(16)
    cu = orc.Camera176()
    cu.projection[:] = [float(x) for x in p32]
    cu.view[:] = [float(x) for x in v32]
    cu.focal[:] = [abs(float((F32(0.5) * p32[0]) * F32(width))), abs(float((F32(0.5) * p32[5]) * F32(height)))]
    cu.viewport[:] = [float(width), float(height)]
    cu.htan_fov[:] = [0.0] * 4
    lp = np.asarray(eye if lod_pos is None else lod_pos, np.float64).astype(F32)
    cu.cam_pos[:] = [float(lp[0]), float(lp[1]), float(lp[2]), 0.0]
    return cu


def top_down_block(center_xy, half_extent, z_top, z_bottom, width, height, lod_pos=None) -> orc.Camera176:
    cx, cy = float(center_xy[0]), float(center_xy[1])
    return camera_block(width, height, (cx, cy, float(z_top)), (cx, cy, float(z_top) - 1.0), (0.0, 1.0, 0.0), half_extent, 0.0,
                        float(z_top) - float(z_bottom), lod_pos=lod_pos)


# The two cameras of the orthographic tests, over the part of the golden plane map that its own perspective sort event draws (the
# event looks towards +y from (1.3, 0.4): splat centres in x -4 .. 12, y 0 .. 12, heights -0.47 .. 0.43).  "top": straight down,
# 21.6 x 12 world units.  "oblique": from the south at 35 degrees elevation.  Depth ranges are chosen so that the splats' depths fall
# in 0.94 .. 1.0, the range of depth_ref.bg_images' proxy depth: some splats in front of it, some behind.  (The oblique camera's near
# plane lies behind its eye -- legitimate for an orthographic view: depth = (d - near) / (far - near) along the view direction.)
CENTRE = (4.0, 6.0)
SPLAT_SCALE = 24.0        # golden-case splats are ~0.25 px at 3.3 px per world unit: scaled up, they cover ~90 % of the frame
SPLAT_SCALE_DENSE = 64.0  # ... and at this scale several screen tiles hold more than 256 pairs (GSWT_OPT_SEGMENT = 256 cuts them)


def camera_args(which: str, centre=CENTRE, lod_pos=None):
    cx, cy = centre
    if which == "top":
        return dict(kind="top_down", center_xy=(cx, cy), half_extent=6.0, z_top=25.0, z_bottom=-0.5, lod_pos=lod_pos)
    el = math.radians(35.0)
    dist = 30.0
    eye = (cx, cy - dist * math.cos(el), 0.5 + dist * math.sin(el))
    return dict(kind="look_at", eye=eye, target=(cx, cy, 0.5), up=(0.0, 0.0, 1.0), half_height=5.0, near=-200.0, far=40.0, lod_pos=lod_pos)


CAMERAS = ("top", "oblique")


def surface_camera_args(name: str, which: str, lod_pos=None):
    """The two cameras over the HeightMap / Sphere golden cases (vertex-stage comparisons only); a hostile case's are its benign one's."""
    if name in ("case_hmap", "case_hmap_hostile"):
        if which == "top":
            return dict(kind="top_down", center_xy=(2.0, 2.0), half_extent=6.0, z_top=4.0, z_bottom=-2.0, lod_pos=lod_pos)
        el = math.radians(35.0)
        return dict(kind="look_at", eye=(2.0, 2.0 - 30.0 * math.cos(el), 0.5 + 30.0 * math.sin(el)), target=(2.0, 2.0, 0.5), up=(0.0, 0.0, 1.0),
                    half_height=5.0, near=10.0, far=50.0, lod_pos=lod_pos)
    assert name == "case_sphere"
    if which == "top":
        return dict(kind="top_down", center_xy=(0.0, 0.0), half_extent=8.0, z_top=8.0, z_bottom=-8.0, lod_pos=lod_pos)
    return dict(kind="look_at", eye=(3.0, -19.0, 6.0), target=(0.0, 0.0, 0.0), up=(0.0, 0.0, 1.0), half_height=8.0, near=5.0, far=35.0, lod_pos=lod_pos)
_CACHE = {}


def golden(name="case_plane"):
    """tests/depth_ref.py's golden case: the scene, and the draws of the case's own perspective sort event.  case_plane_hostile and
    case_hmap_hostile: the same case over a hostile tile set (tests/hostile_cases.py)."""
    from tests import depth_ref as DR
    from tests import hostile_cases as HC
    if name not in _CACHE:
        _CACHE[name] = HC.build(name) if HC.is_hostile(name) else DR.golden_case(name)
    return _CACHE[name]


def scene_of(g, splat_scale=SPLAT_SCALE) -> orc.Scene160:
    su = orc.Scene160.from_buffer_copy(bytes(g["su"]))
    su.splat_scale = splat_scale
    return su


def plane_records(which: str, splat_scale=SPLAT_SCALE):
    """(camera block, scene block, (a)'s records) of the plane case under camera `which`; computed once."""
    k = ("rec", which, splat_scale)
    if k not in _CACHE:
        g = golden()
        cu, su = block_of(camera_args(which, lod_pos=g["pos"])), scene_of(g, splat_scale)
        _CACHE[k] = (cu, su, project_ortho_f32(cu, su, g["pp"].tex, g["draws"]))
    return _CACHE[k]


def block_of(args, width=W, height=H) -> orc.Camera176:
    a = dict(args)
    if a.pop("kind") == "top_down":
        return top_down_block(a["center_xy"], a["half_extent"], a["z_top"], a["z_bottom"], width, height, lod_pos=a["lod_pos"])
    return camera_block(width, height, a["eye"], a["target"], a["up"], a["half_height"], a["near"], a["far"], lod_pos=a["lod_pos"])


def ortho_camera_of(args, width=W, height=H):
    """The same camera through the product's gswt_renderer_amd/ortho.py."""
    from gswt_renderer_amd import ortho
    a = dict(args)
    if a.pop("kind") == "top_down":
        return ortho.top_down(a["center_xy"], a["half_extent"], a["z_top"], a["z_bottom"], width, height, lod_pos=a["lod_pos"])
    return ortho.OrthoCamera(width, height, a["eye"], a["target"], a["up"], a["half_height"], a["near"], a["far"], lod_pos=a["lod_pos"])


# ---- (a) the vertex stage in float32 ------------------------------------------------------------------------------------------------
_HALF = None


def _half_table():
    global _HALF
    if _HALF is None:
        _HALF = np.array([orc.half_to_float(h) for h in range(65536)], dtype=F32)      # halfToFloat, gswt.wgsl:478-494
    return _HALF


def _f32a(x):
    return np.array(list(x), dtype=F32)


def _clamp(e, lo, hi):
    return np.fmin(np.fmax(e, lo), hi)           # WGSL clamp = min(max(e, lo), hi); fmin / fmax drop a NaN operand as fminf / fmaxf do


def _draw_inputs(scene, tex, d):
    """Per instance of one draw: the record words, list LOD ids, map ids and the instance offset (A1..A3 inputs)."""
    gs = np.asarray(d.gs_index, dtype=np.int64)
    n = gs.shape[0]
    rec = np.ascontiguousarray(tex, dtype=np.uint32).reshape(-1, 8)[gs]
    lod = np.asarray(d.lod_id, dtype=np.uint32) if d.lod_id is not None else np.zeros(n, np.uint32)
    t = d.tile
    if t.single_draw == 1:
        mid = np.asarray(d.map_id, dtype=np.uint32)
        wh_y = np.uint32(2 * scene.map_half_wh[1] + (1 if scene.surface_type != 2 else 0))
        qx = (mid // wh_y).astype(np.int64) - int(scene.map_half_wh[0]) + int(scene.center_coord[0])
        qy = (mid % wh_y).astype(np.int64) - int(scene.map_half_wh[1]) + int(scene.center_coord[1])
        off = [qx.astype(F32) * F32(scene.tile_width), qy.astype(F32) * F32(scene.tile_width), np.zeros(n, F32)]
    else:
        off = [np.full(n, F32(t.offset[k]), F32) for k in range(3)]
    return rec, lod, off


def _centres(scene, rec, off):
    pos = [rec[:, k].copy().view(F32) for k in range(3)]
    return [(pos[k] + off[k]) * F32(scene.scene_scale[k]) for k in range(3)]


def _covariance3(scene, rec):
    """A7 on the plain surface: Vrk = scene_scale_mat * K * transpose(scene_scale_mat), the full products, K[3 c + r]."""
    hf = _half_table()
    a, b = hf[rec[:, 4] & 0xFFFF], hf[rec[:, 4] >> 16]
    c2, dd = hf[rec[:, 5] & 0xFFFF], hf[rec[:, 5] >> 16]
    e, ff = hf[rec[:, 6] & 0xFFFF], hf[rec[:, 6] >> 16]
    K = [a, b, c2, b, dd, e, c2, e, ff]
    z = np.zeros_like(a)
    S = [np.full_like(a, F32(scene.scene_scale[0])), z, z, z, np.full_like(a, F32(scene.scene_scale[1])), z, z, z,
         np.full_like(a, F32(scene.scene_scale[2]))]
    SK = [None] * 9
    for cc in range(3):
        for r in range(3):
            SK[3 * cc + r] = (S[r] * K[3 * cc] + S[3 + r] * K[3 * cc + 1]) + S[6 + r] * K[3 * cc + 2]
    R = [None] * 9
    for cc in range(3):
        for r in range(3):
            R[3 * cc + r] = (SK[r] * S[cc] + SK[3 + r] * S[3 + cc]) + SK[6 + r] * S[6 + cc]
    return R


def project_ortho_f32(cam, scene, tex, draws, aa_s=None) -> np.ndarray:
    """The orthographic vertex stage of every instance of `draws` (orc.Draw, draw order) -> orc.SPLAT_DTYPE records.  Plain surface,
    draw_mode 0, no point-cloud radius.  `visible` carries the product's meaning: a vertex-stage survivor whose fragment setup F1 / F2
    (|major|^2, |minor|^2 in (0, inf), as tests/depth_ref.py evaluates them) also passes.
    aa_s (a binary32 number > 0, tests/antialias_ref.py: aa_s): GSWT_OPT_ANTIALIAS' pixel filter on this stage's own eigenvalues --
    antialias_ref.filter_f32 behind the rejection l2 < 0 and the direction, comp on alpha behind the LOD-transition product."""
    from tests import antialias_ref as AA
    assert scene.surface_type == 0 and scene.draw_mode == 0 and not scene.point_cloud_radius > 0.0
    V, P = _f32a(cam.view), _f32a(cam.projection)
    GP = np.zeros(16, F32)                           # opengl_to_wgpu * projection, gswt.wgsl:152-160
    for cc in range(4):
        GP[4 * cc + 0] = P[4 * cc + 0]
        GP[4 * cc + 1] = P[4 * cc + 1]
        GP[4 * cc + 2] = F32(0.5) * P[4 * cc + 2] + F32(0.5) * P[4 * cc + 3]
        GP[4 * cc + 3] = P[4 * cc + 3]
    fx, fy = F32(cam.focal[0]), F32(cam.focal[1])
    cpos = _f32a(cam.cam_pos)
    tdist = _f32a(scene.transition_dist)
    out = []
    with np.errstate(all="ignore"):
        for d in draws:
            t = d.tile
            rec, lod, off = _draw_inputs(scene, tex, d)
            n = rec.shape[0]
            sp = np.zeros(n, dtype=orc.SPLAT_DTYPE)
            keep = np.ones(n, bool)
            if t.valid_lod_id >= 0:                                                  # A1 :38-42
                keep &= lod == np.uint32(t.valid_lod_id)
            c = _centres(scene, rec, off)                                            # A2, A3 :45-65
            if scene.use_clip == 1:                                                  # (mapped height of the plain surface: 0)
                keep &= not (F32(0.0) < F32(scene.clip_height))
            t_ratio = np.full(n, F32(-1.0), F32)                                     # A5 :91-150
            higher = np.zeros(n, np.uint32)
            if t.changing == 1:
                dx, dy, dz = c[0] - cpos[0], c[1] - cpos[1], c[2] - cpos[2]
                cam_dist = np.sqrt((dx * dx + dy * dy) + dz * dz)
                if t.single_draw == 1:
                    d1 = tdist[(lod - np.uint32(1)) & np.uint32(15)]
                    d2 = tdist[lod & np.uint32(15)]
                    mid_lod = np.where(cam_dist - d1 < d2 - cam_dist, lod - np.uint32(1), lod)
                    higher = np.where(lod == 0, np.uint32(0), np.where(lod == np.uint32(scene.num_lod - 1), lod - np.uint32(1), mid_lod)).astype(np.uint32)
                else:
                    higher = np.full(n, np.uint32(t.tile_id[0] if t.changing_to_lower == 1 else t.tile_id[0] - 1), np.uint32)
                td = tdist[higher & np.uint32(15)]
                thw = F32(scene.transition_width_ratio) * td
                t_ratio = _clamp((cam_dist - td) / thw + F32(0.5), F32(0.0), F32(1.0))
                keep &= ~(((lod == higher + np.uint32(1)) & (t_ratio == 0)) | ((lod == higher) & (t_ratio == 1)))
            # A6 :152-167
            one = np.ones(n, F32)
            cv = [((V[r] * c[0] + V[4 + r] * c[1]) + V[8 + r] * c[2]) + V[12 + r] * one for r in range(4)]
            q = [((GP[r] * cv[0] + GP[4 + r] * cv[1]) + GP[8 + r] * cv[2]) + GP[12 + r] * cv[3] for r in range(4)]
            clip = F32(1.2) * q[3]
            keep &= ~((q[2] < -clip) | (q[0] < -clip) | (q[0] > clip) | (q[1] < -clip) | (q[1] > clip))
            K = _covariance3(scene, rec)                                             # A7 :169-205
            # A8: J_T columns (fx, 0, 0), (0, fy, 0), (0, 0, 0) in place of gswt.wgsl:213-232; T and cov2d the written full products
            z = np.zeros(n, F32)
            JT = [np.full(n, fx, F32), z, z, z, np.full(n, fy, F32), z, z, z, z]
            Tm = [None] * 9
            for cc in range(3):
                for r in range(3):
                    Tm[3 * cc + r] = (V[4 * r + 0] * JT[3 * cc] + V[4 * r + 1] * JT[3 * cc + 1]) + V[4 * r + 2] * JT[3 * cc + 2]
            Am, C2 = [None] * 9, [None] * 9
            for cc in range(3):
                for r in range(3):
                    Am[3 * cc + r] = (Tm[3 * r + 0] * K[3 * cc] + Tm[3 * r + 1] * K[3 * cc + 1]) + Tm[3 * r + 2] * K[3 * cc + 2]
            for cc in range(3):
                for r in range(3):
                    C2[3 * cc + r] = (Am[r] * Tm[3 * cc] + Am[3 + r] * Tm[3 * cc + 1]) + Am[6 + r] * Tm[3 * cc + 2]
            c00, c01, c11 = C2[0], C2[1], C2[4]
            mid = F32(0.5) * (c00 + c11)
            hxx = F32(0.5) * (c00 - c11)
            radius = np.sqrt(hxx * hxx + c01 * c01)
            l1, l2 = mid + radius, mid - radius
            keep &= ~(l2 < 0)
            vx, vy = c01, l1 - c00
            vlen = np.sqrt(vx * vx + vy * vy)
            ex, ey = vx / vlen, vy / vlen
            comp = None
            if aa_s is not None and float(aa_s) > 0.0:
                smaj, smin, comp = AA.filter_f32(l1, l2, F32(aa_s))
            else:
                smaj = np.fmin(np.sqrt(F32(2.0) * l1), F32(1024.0))
                smin = np.fmin(np.sqrt(F32(2.0) * l2), F32(1024.0))
            sp["major"][:, 0], sp["major"][:, 1] = smaj * ex, smaj * ey
            sp["minor"][:, 0], sp["minor"][:, 1] = smin * ey, smin * -ex
            # A9 :260-265, 402-410
            cw = rec[:, 7]
            col = [((cw >> np.uint32(8 * k)) & np.uint32(0xFF)).astype(F32) / F32(255.0) for k in range(4)]
            if t.changing == 1:
                col[3] = np.where(lod != higher, col[3] * t_ratio, col[3] * (F32(1.0) - t_ratio))
            if comp is not None:
                col[3] = col[3] * comp
            # A10 :415-419
            fade = _clamp(q[2] / q[3] + F32(1.0), F32(0.0), F32(1.0))
            for k in range(4):
                sp["rgba"][:, k] = col[k] * fade
            sp["ndc"][:, 0], sp["ndc"][:, 1] = q[0] / q[3], q[1] / q[3]
            sp["depth"] = q[2] / q[3]
            keep &= (sp["depth"] >= 0) & (sp["depth"] <= 1)
            # fragment setup F1 / F2, as tests/depth_ref.py: fma(uy, uy, ux * ux)
            hs = F32(0.5) * F32(scene.splat_scale)
            ux, uy = hs * sp["major"][:, 0], -(hs * sp["major"][:, 1])
            wx, wy = hs * sp["minor"][:, 0], -(hs * sp["minor"][:, 1])
            uu = (uy.astype(np.float64) * uy + (ux * ux).astype(np.float64)).astype(F32)
            ww = (wy.astype(np.float64) * wy + (wx * wx).astype(np.float64)).astype(F32)
            keep &= (uu > 0) & (ww > 0) & (uu < np.inf) & (ww < np.inf)
            sp["visible"] = keep.astype(np.int32)
            for fld in ("ndc", "depth", "major", "minor", "rgba"):                  # (a discarded instance's outputs are zero, as the oracle's)
                sp[fld][~keep] = 0
            out.append(sp)
    return np.concatenate(out) if out else np.zeros(0, orc.SPLAT_DTYPE)


# ---- (b) the covariance in float64 ---------------------------------------------------------------------------------------------------
def cov2d_f64(cam, scene, tex, draws):
    """(cov [n, 3] = (c00, c01, c11), err [n, 3]) of every instance: the analytic cov2d = J Sigma J^T with Sigma = S K S (S the
    scene scale, K the decoded covariance) and J = diag(fx, fy) * (rows 0, 1 of the view rotation), in float64 from the binary32
    inputs; err bounds the rounding error of the binary32 chain of (a) per entry (see tests/test_ortho_cpu.py)."""
    hf = _half_table().astype(np.float64)
    Wm = np.array([[float(cam.view[4 * c + r]) for c in range(3)] for r in range(3)])        # world -> view rotation
    J = np.diag([float(cam.focal[0]), float(cam.focal[1])]) @ Wm[:2]
    S = np.diag([float(scene.scene_scale[k]) for k in range(3)])
    covs, errs = [], []
    for d in draws:
        rec = np.ascontiguousarray(tex, dtype=np.uint32).reshape(-1, 8)[np.asarray(d.gs_index, dtype=np.int64)]
        a, b = hf[rec[:, 4] & 0xFFFF], hf[rec[:, 4] >> 16]
        c2, dd = hf[rec[:, 5] & 0xFFFF], hf[rec[:, 5] >> 16]
        e, ff = hf[rec[:, 6] & 0xFFFF], hf[rec[:, 6] >> 16]
        K = np.stack([np.stack([a, b, c2], -1), np.stack([b, dd, e], -1), np.stack([c2, e, ff], -1)], -2)      # [n, 3, 3]
        JS = J @ S
        C = JS @ K @ JS.T
        Cabs = np.abs(JS) @ np.abs(K) @ np.abs(JS).T
        covs.append(np.stack([C[:, 0, 0], C[:, 0, 1], C[:, 1, 1]], -1))
        errs.append(np.stack([Cabs[:, 0, 0], Cabs[:, 0, 1], Cabs[:, 1, 1]], -1))
    return np.concatenate(covs), np.concatenate(errs)


def axes_f64(cov, splat_clamp=1024.0):
    """(major [n, 2], minor [n, 2], parts) from (c00, c01, c11) by the shader's formulas (gswt.wgsl:234-258) in float64."""
    c00, c01, c11 = cov[:, 0], cov[:, 1], cov[:, 2]
    mid, hxx = 0.5 * (c00 + c11), 0.5 * (c00 - c11)
    radius = np.sqrt(hxx * hxx + c01 * c01)
    l1, l2 = mid + radius, mid - radius
    vx, vy = c01, l1 - c00
    vlen = np.sqrt(vx * vx + vy * vy)
    with np.errstate(all="ignore"):
        ex, ey = vx / vlen, vy / vlen
        smaj = np.minimum(np.sqrt(2.0 * np.maximum(l1, 0.0)), splat_clamp)
        smin = np.minimum(np.sqrt(2.0 * np.maximum(l2, 0.0)), splat_clamp)
    return (np.stack([smaj * ex, smaj * ey], -1), np.stack([smin * ey, smin * -ex], -1),
            dict(l1=l1, l2=l2, vy=vy, vlen=vlen, smaj=smaj, smin=smin, radius=radius))


# ---- (c) the blend in float64 --------------------------------------------------------------------------------------------------------
def composite_f64(sp, width: int, height: int, *, splat_scale: float = 1.0, order_mode: int = 0, bg_rgba=None, bg_depth=None):
    """The image and depth of tests/depth_ref.py's composite from the same records, every operation in float64 and without the
    fragment sequence's block origins: pixel-centre offset through the inverse axis map, r^2 <= 4, B = exp(-r^2) alpha, `over`."""
    f = np.float64
    vis = sp["visible"] == 1
    idx = np.nonzero(vis)[0]
    if order_mode == 1:
        idx = idx[np.argsort(-sp["depth"][idx].astype(f), kind="stable")]
    img = np.zeros((height, width, 4), f) if bg_rgba is None else np.array(bg_rgba, f).reshape(height, width, 4)
    zbg = np.ones((height, width), f) if bg_depth is None else np.array(bg_depth, f).reshape(height, width)
    z = zbg.copy()
    ys, xs = np.mgrid[0:height, 0:width]
    pxc, pyc = xs + 0.5, ys + 0.5
    hs = 0.5 * float(splat_scale)
    for k in idx:
        cx = (0.5 * f(sp["ndc"][k, 0]) + 0.5) * width
        cy = (-0.5 * f(sp["ndc"][k, 1]) + 0.5) * height
        ux, uy = hs * f(sp["major"][k, 0]), -hs * f(sp["major"][k, 1])
        vx, vy = hs * f(sp["minor"][k, 0]), -hs * f(sp["minor"][k, 1])
        uu, vv = ux * ux + uy * uy, vx * vx + vy * vy
        if not (uu > 0 and vv > 0 and np.isfinite(uu) and np.isfinite(vv)):
            continue
        dx, dy = pxc - cx, pyc - cy
        pu, pv = (dx * ux + dy * uy) / uu, (dx * vx + dy * vy) / vv
        r2 = pu * pu + pv * pv
        dk = f(sp["depth"][k])
        cover = (r2 <= 4.0) & (dk < zbg)
        if not cover.any():
            continue
        B = np.where(cover, np.exp(-r2) * f(sp["rgba"][k, 3]), 0.0)
        om = 1.0 - B
        for ch in range(3):
            img[..., ch] = B * f(sp["rgba"][k, ch]) + img[..., ch] * om
        img[..., 3] = B + img[..., 3] * om
        z = B * dk + z * om
    return img, z
