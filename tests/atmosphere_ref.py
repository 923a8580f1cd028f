"""CPU reference of the atmosphere (gswt_set_atmosphere, include/gswt_hip.h): the per-splat far fade and distance fog, in numpy.

Plain surface.  The splat centres are tests/ortho_ref.py's (`_draw_inputs` / `_centres`: every instance of every draw, in draw order, the
order of the varyings), and dist, t and fs are restated operator by operator in np.float32: one rounding per written `*` `+` `-` and
sqrt, sums in the written order.  Every operation of the fade is correctly rounded on the device too, so this reference is exact: the
faded alpha is compared bit for bit.

HeightMap and Sphere surfaces.  The mapped centre is not restated here; dist comes in float64 from the splat's own record, its `ndc` and
`depth` unprojected through the inverse of GP * V (GP = opengl_to_wgpu * projection).  What that distance can be off by, and the
tolerance on t that follows (`surface_t_tol`):
  * depth = q.z / q.w is a binary32 number below 1, so it carries a rounding of up to 2^-25, and q.z, q.w themselves are two chained
    four-term sums of binary32 products (A6: view, then projection; 7 roundings each) whose terms are of the size of the splat's world
    coordinates relative to the camera, i.e. of the order of the view depth z.  That is up to about 15 roundings of 2^-24 relative to z
    on q.z against q.w: delta_depth <= C * 2^-24 with C = 16.
  * With depth = far / (far - near) * (1 - near / z), d depth / dz = near / z^2 (far >> near), so the unprojected view depth -- and with
    it the distance along the ray -- moves by delta_z = z^2 / near * delta_depth = C * z^2 / near * 2^-24.  The lateral part (ndc, one
    rounding each, times z) is below 2^-23 z and is covered by the same term (z / near > 1).
  * t = (fade_end - dist) * fade_inv: delta_t = delta_z * fade_inv, plus 4 * 2^-24 for the device's own three roundings and dist's.
  * fs = t^2 (3 - 2 t) has slope 6 t (1 - t) <= 1.5: delta_fs <= 1.5 * delta_t (+ 4 * 2^-24 for its four roundings); the faded alpha is
    the unfaded one times fs, one more rounding.
A splat whose reference t is within delta_t of 0 may be discarded or not; the comparisons leave it out (`masked`).

Fog.  F and the unrounded 255 c' in float64, from the binary32 block as packed (`params`) and the colours of the unfogged record.  The
device's binary32 chain puts at most about 5e-7 on c' (dist 2 ulp, the exponent's argument 3 ulp, e 2 ulp), 1.3e-4 codes; a byte
must equal the float64 rint wherever 255 c' is farther than FOG_MARGIN = 1e-3 codes from a half-integer, and be within one code of it
everywhere."""
from __future__ import annotations

import struct

import numpy as np

from tests import ortho_ref as OR

F32 = np.float32
U = 2.0 ** -24
DEPTH_ROUNDINGS = 16.0        # C above
FOG_MARGIN = 1e-3             # codes
MAX_MASKED = 0.02             # share of the visible splats (fade) / of the channels (fog) that may be left out


def params(a) -> dict:
    """The block's fields as the library reads them (binary32), and the derived fade_inv = 1.0f / (fade_end - fade_start)."""
    fs, fe, dens, start, mx, r, g, b = (F32(x) for x in struct.unpack("<8f", bytes(a)))
    p = dict(fade_start=fs, fade_end=fe, fog_density=dens, fog_start=start, fog_max=mx, fog_color=np.array([r, g, b], F32))
    p["fade_on"], p["fog_on"] = bool(fe > 0), bool(dens > 0)
    p["fade_inv"] = F32(1.0) / (fe - fs) if p["fade_on"] else F32(0.0)
    return p


# ---- the fade --------------------------------------------------------------------------------------------------------------------
def dist_f32(cam_pos, scene, tex, draws) -> np.ndarray:
    """Plain surface: sqrtf((dx*dx + dy*dy) + dz*dz) of every instance in draw order, d = centre - cam_pos, in binary32."""
    assert scene.surface_type == 0
    cp = np.array([cam_pos[0], cam_pos[1], cam_pos[2]], F32)
    out = []
    for d in draws:
        rec, _, off = OR._draw_inputs(scene, tex, d)
        c = OR._centres(scene, rec, off)
        dx, dy, dz = c[0] - cp[0], c[1] - cp[1], c[2] - cp[2]
        out.append(np.sqrt((dx * dx + dy * dy) + dz * dz))
    return np.concatenate(out) if out else np.zeros(0, F32)


def fade_f32(dist, p):
    """(t, fs) in binary32: t = clampf((fade_end - dist) * fade_inv, 0, 1) (a NaN clamps to 0), fs = (t * t) * (3.0f - 2.0f * t)."""
    dist = np.asarray(dist, F32)
    with np.errstate(all="ignore"):
        t = np.fmin(np.fmax((p["fade_end"] - dist) * p["fade_inv"], F32(0.0)), F32(1.0)).astype(F32)
        fs = ((t * t) * (F32(3.0) - F32(2.0) * t)).astype(F32)
    return t, fs


def fade_f64(dist, p):
    t = np.clip((float(p["fade_end"]) - np.asarray(dist, np.float64)) * float(p["fade_inv"]), 0.0, 1.0)
    return t, t * t * (3.0 - 2.0 * t)


def _gp_v(cam):
    P = np.array(cam.projection, np.float64).reshape(4, 4).T          # column-major blocks -> [row, column]
    V = np.array(cam.view, np.float64).reshape(4, 4).T
    gl_to_wgpu = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 0.5, 0.5], [0, 0, 0, 1.0]])
    return gl_to_wgpu @ P, V


def unproject_f64(cam, ndc, depth):
    """(world position [n, 3], view depth z = clip w [n]) of the points (ndc.x, ndc.y, depth) through the inverse of GP * V, float64."""
    GP, V = _gp_v(cam)
    M = GP @ V
    n = np.asarray(depth).shape[0]
    h = np.stack([np.asarray(ndc, np.float64)[:, 0], np.asarray(ndc, np.float64)[:, 1], np.asarray(depth, np.float64), np.ones(n)], 0)
    with np.errstate(all="ignore"):
        w = np.linalg.solve(M, h)
        pos = (w[:3] / w[3]).T
        clip = M @ np.vstack([pos.T, np.ones(n)])
    return pos, clip[3]


def dist_f64(cam, ndc, depth):
    """(distance from cam.cam_pos, view depth z) of the records' unprojected centres."""
    pos, z = unproject_f64(cam, ndc, depth)
    cp = np.array([float(cam.cam_pos[k]) for k in range(3)])
    return np.sqrt(((pos - cp) ** 2).sum(1)), z


def near_of(cam) -> float:
    """The near plane of the perspective block: depth 0 on the view axis."""
    _, z = unproject_f64(cam, np.zeros((1, 2)), np.zeros(1))
    return float(z[0])


def surface_t_tol(z, near, p):
    """delta_t of the docstring per splat, from its view depth z."""
    return DEPTH_ROUNDINGS * np.asarray(z, np.float64) ** 2 / near * U * float(p["fade_inv"]) + 4.0 * U


def ramp_from_percentiles(dist, lo=30.0, hi=75.0):
    """(fade_start, fade_end) as binary32 numbers at the lo-th / hi-th percentile of the distances."""
    return float(F32(np.percentile(dist, lo))), float(F32(np.percentile(dist, hi)))


def ramp_shares(dist, p, tol_t=0.0):
    """Shares of `dist` (strictly inside the ramp, at t = 1, at t = 0, within tol_t of t = 0 but not beyond the ramp's end + tol)."""
    t, _ = fade_f64(dist, p)
    n = max(1, t.shape[0])
    raw = (float(p["fade_end"]) - np.asarray(dist, np.float64)) * float(p["fade_inv"])
    return (float(((t > 0) & (t < 1)).sum()) / n, float((t >= 1).sum()) / n, float((t <= 0).sum()) / n,
            float((np.abs(raw) <= tol_t).sum()) / n)


# ---- the fog ---------------------------------------------------------------------------------------------------------------------
def fog_amount_f64(dist, p):
    x = float(p["fog_density"]) * np.maximum(np.asarray(dist, np.float64) - float(p["fog_start"]), 0.0)
    return float(p["fog_max"]) * (1.0 - np.exp(-x))


def fog_codes_f64(rgb, dist, p):
    """The unrounded 255 c' [n, 3] of colours rgb [n, 3] (in 0 .. 1) at distances dist."""
    F = fog_amount_f64(dist, p)[:, None]
    c = np.asarray(rgb, np.float64) * (1.0 - F) + p["fog_color"].astype(np.float64)[None, :] * F
    return 255.0 * np.clip(c, 0.0, 1.0)


def fog_bytes(codes):
    """(float64 rint of the codes, mask of the channels within FOG_MARGIN of a half-integer)."""
    return np.rint(codes), np.abs(codes - np.floor(codes) - 0.5) <= FOG_MARGIN


def bytes_of(rgba):
    """The 8-bit codes of a record's float colours (code / 255 in binary32)."""
    return np.rint(np.asarray(rgba, np.float64)[:, :3] * 255.0)
