"""CPU reference of the sun shadows (gswt_set_shadow_map, include/gswt_hip.h), in numpy.

Plain surface.  The splat centres are tests/ortho_ref.py's (`_draw_inputs` / `_centres`: every instance of every draw, in draw order,
the order of the varyings), and the lookup and the shade are restated operator by operator in np.float32: one rounding per written
`*` `+` `-`, sums in the written order.  Every operation is correctly rounded on the device too, so this reference is exact: the
shaded colour bytes are compared bit for bit.  `lookup_f64` is the same function in float64.

HeightMap and Sphere surfaces.  The mapped centre is not restated; it comes in float64 from the splat's own unshadowed record, its
`ndc` and `depth` unprojected through the inverse of GP * V (tests/atmosphere_ref.py: unproject_f64).  What follows from that:
  * the unprojected position is off by up to delta = AR.DEPTH_ROUNDINGS * z^2 / near * 2^-24 world units (atmosphere_ref's
    derivation: the record's depth carries about 16 roundings of 2^-24 relative to the view depth z, and d depth / dz = near / z^2);
  * u = (lx * 0.5 + 0.5) * W - 0.5 with lx = row 0 of M . c moves by at most delta * |row 0 of M| * W / 2 texels, v likewise with row 1
    and H; to that comes the device's own binary32 evaluation of M . c, at most 8 * 2^-24 * (sum |M_k c_k| + |M_12|) * W / 2;
  * the test's texels are exactly 0.0 or 1.0 and ld is kept away from 0 and 1 (below), so each compare r > Z is the same on both
    sides and lit is the bilinear mix of fixed 0 / 1 values: piecewise linear in (u, v) with |d lit / du| <= 1 and |d lit / dv| <= 1
    per texel.  So delta_lit <= delta_u + delta_v;
  * c' = c (1 - sh) + shade * sh with sh = strength * (1 - lit): |dc' / d lit| = strength * |c - shade| <= strength, in codes
    255 * strength * delta_lit.
`surface_tols` is that bound; a byte must lie within 0.5 + tol + MARGIN of the float64 code.  A splat whose ld is within
delta * |row 2 of M| of 0 or 1, or of `bias` (where r changes sign against a 0.0 texel), may fall on either side of the `outside` test
or the compare: the comparisons leave it out (`masked`), at most AR.MAX_MASKED of the visible splats.

With tint and fog.  The order tint, shadow, fog in float64 (`chain_codes_f64`); a byte equals the float64 rint wherever the code is
farther than AR.FOG_MARGIN from a half-integer, and is within one code of it everywhere (the binary32 chain of at most a dozen
operations on values in 0 .. 1 stays below 1e-6, 3e-4 codes)."""
from __future__ import annotations

import struct

import numpy as np

from tests import atmosphere_ref as AR
from tests import ortho_ref as OR

F32 = np.float32
U = 2.0 ** -24
MARGIN = 1e-3                 # codes: the device's binary32 chain against the float64 one


def params(m) -> dict:
    """The block's fields as the library reads them (binary32), the image and its size."""
    v = struct.unpack("<16f2f3f3I", bytes(m))
    M = np.array(v[:16], F32)
    return dict(M=M, bias=F32(v[16]), strength=F32(v[17]), shade=np.array(v[18:21], F32), W=int(m.width), H=int(m.height),
                Z=np.ascontiguousarray(np.asarray(m.depth, F32)).reshape(int(m.height), int(m.width)))


def centres_f32(scene, tex, draws):
    """Plain surface: the scene-scaled centre (c0, c1, c2) of every instance in draw order, binary32."""
    assert scene.surface_type == 0
    out = [[], [], []]
    for d in draws:
        rec, _, off = OR._draw_inputs(scene, tex, d)
        c = OR._centres(scene, rec, off)
        for k in range(3):
            out[k].append(c[k])
    return [np.concatenate(o) if o else np.zeros(0, F32) for o in out]


def _texel(Z, W, H, i, j):
    """(value, in range) of texel (i, j) per element; out of range reads as lit."""
    ok = (i >= 0) & (i < W) & (j >= 0) & (j < H)
    ii, jj = np.clip(i, 0, W - 1), np.clip(j, 0, H - 1)
    return Z[jj, ii], ok


def _lookup(c, p, ft):
    """The definition of include/gswt_hip.h in the float type `ft`: (sh, lit, outside, (u, v, ld))."""
    M = p["M"].astype(ft)
    c0, c1, c2 = (np.asarray(x, ft) for x in c)
    W, H = p["W"], p["H"]
    half, one = ft(0.5), ft(1.0)
    with np.errstate(all="ignore"):
        lx = ((M[0] * c0 + M[4] * c1) + M[8] * c2) + M[12]
        ly = ((M[1] * c0 + M[5] * c1) + M[9] * c2) + M[13]
        ld = ((M[2] * c0 + M[6] * c1) + M[10] * c2) + M[14]
        u = (lx * half + half) * ft(W) - half
        v = (half - ly * half) * ft(H) - half
        outside = ~((ld >= 0) & (ld <= 1)) | ~((u > -1) & (u < W)) | ~((v > -1) & (v < H))
        us, vs = np.where(outside, ft(0.0), u), np.where(outside, ft(0.0), v)
        x0, y0 = np.floor(us), np.floor(vs)
        wx, wy = us - x0, vs - y0
        r = ld - p["bias"].astype(ft)
        i0, j0 = x0.astype(np.int64), y0.astype(np.int64)
        Z = p["Z"].astype(ft)
        t = {}
        for name, (di, dj) in dict(t00=(0, 0), t10=(1, 0), t01=(0, 1), t11=(1, 1)).items():
            z, ok = _texel(Z, W, H, i0 + di, j0 + dj)
            t[name] = np.where(ok & (r > z), ft(0.0), one).astype(ft)
        lit = (t["t00"] * (one - wx) + t["t10"] * wx) * (one - wy) + (t["t01"] * (one - wx) + t["t11"] * wx) * wy
        lit = np.where(outside, one, lit).astype(ft)
        sh = (p["strength"].astype(ft) * (one - lit)).astype(ft)
    return sh, lit, outside, (u, v, ld)


def lookup_f32(c, p):
    return _lookup(c, p, F32)


def lookup_f64(c, p):
    return _lookup(c, p, np.float64)


def quantise_f32(c):
    """(uint32_t)rintf(fminf(fmaxf(c, 0), 1) * 255.0f) per channel, as float codes."""
    c = np.asarray(c, F32)
    return np.rint(np.fmin(np.fmax(c, F32(0.0)), F32(1.0)) * F32(255.0)).astype(F32)


def shaded_rgb_f32(rgb, sh, p):
    """What gswt_debug_read_projected reports for colours rgb [n, 3] (code / 255 in binary32) under shadow amounts sh, in binary32:
    sh == 0 leaves the colour as it is; otherwise c' = c * (1 - sh) + shade * sh, quantised once, reported as (float)byte' / 255.0f."""
    rgb, sh = np.asarray(rgb, F32), np.asarray(sh, F32)
    out = rgb.copy()
    one = F32(1.0)
    for k in range(3):
        mixed = rgb[:, k] * (one - sh) + p["shade"][k] * sh
        out[:, k] = np.where(sh == 0, rgb[:, k], quantise_f32(mixed) / F32(255.0))
    return out


def shade_codes_f64(rgb, sh, p):
    """The unrounded 255 c' [n, 3] in float64."""
    rgb, sh = np.asarray(rgb, np.float64), np.asarray(sh, np.float64)[:, None]
    return 255.0 * np.clip(rgb * (1.0 - sh) + p["shade"].astype(np.float64)[None, :] * sh, 0.0, 1.0)


def shares(sh, p):
    """Shares of (fully lit, fully shadowed, strictly between) among the amounts sh."""
    sh = np.asarray(sh, np.float64)
    n = max(1, sh.shape[0])
    s = float(p["strength"])
    return float((sh == 0).sum()) / n, float((sh == s).sum()) / n, float(((sh > 0) & (sh < s)).sum()) / n


# ---- the surfaces ----------------------------------------------------------------------------------------------------------------
def persp_delta(z, near):
    """What a position unprojected from a perspective record's (or proxy pixel's) binary32 depth can be off by, world units."""
    return AR.DEPTH_ROUNDINGS * np.asarray(z, np.float64) ** 2 / near * U


def surface_tols(pos, delta, p):
    """(tolerance on lit * strength, i.e. on sh; tolerance on ld) per point of the docstring, from the float64 position pos [n, 3] and
    its error bound delta; 255 x the first is the tolerance in codes."""
    M = p["M"].astype(np.float64)
    rows = [np.array([M[r], M[4 + r], M[8 + r]]) for r in range(3)]
    own = [8.0 * U * (np.abs(pos * rows[r][None, :]).sum(1) + abs(M[12 + r])) for r in range(3)]
    du = (delta * np.abs(rows[0]).sum() + own[0]) * p["W"] / 2.0
    dv = (delta * np.abs(rows[1]).sum() + own[1]) * p["H"] / 2.0
    return float(p["strength"]) * (du + dv), delta * np.abs(rows[2]).sum() + own[2]


def unit_light(Z, **kw):
    """A light whose texel (i, j) of a W x H map covers world x in i .. i + 1 and y in H - 1 - j .. H - j, depth 0 at z = 2 and 1 at
    z = -2: every coefficient exact in binary32 for W, H powers of two, u = x - 0.5, v = H - 0.5 - y, ld = 0.5 - z / 4."""
    from gswt_renderer_amd import shadows
    H, W = Z.shape
    M = np.zeros(16)
    M[0], M[12] = 2.0 / W, -1.0
    M[5], M[13] = 2.0 / H, -1.0
    M[10], M[14], M[15] = -0.25, 0.5, 1.0
    return shadows.ShadowMap(M, Z, **kw)


def two_region_map(W, H):
    """Texels exactly 0.0 (everything behind them is shadowed) in the left half and 1.0 (lit) in the right half."""
    Z = np.ones((H, W), F32)
    Z[:, :W // 2] = 0.0
    return Z


# ---- tint, shadow, fog -------------------------------------------------------------------------------------------------------------
def chain_codes_f64(rgb, tint, sh, p, dist=None, atm=None):
    """The unrounded 255 c' of colours rgb [n, 3] through the tint (r, g, b, strength bytes, or None), the shadow and the fog (atm:
    AR.params of a block with the fog on, or None), float64."""
    c = np.asarray(rgb, np.float64)
    if tint is not None:
        k = tint[3] / 255.0
        c = c * (1.0 - k) + (np.array(tint[:3], np.float64) / 255.0)[None, :] * k
    s = np.asarray(sh, np.float64)[:, None]
    c = c * (1.0 - s) + p["shade"].astype(np.float64)[None, :] * s
    if atm is not None:
        F = AR.fog_amount_f64(dist, atm)[:, None]
        c = c * (1.0 - F) + atm["fog_color"].astype(np.float64)[None, :] * F
    return 255.0 * np.clip(c, 0.0, 1.0)


# ---- the light of the plane case ---------------------------------------------------------------------------------------------------
LIGHT_W, LIGHT_H = 32, 24     # not square: a swap of W and H shows


def plane_light():
    """An oblique sun over the part of the golden plane map its sort event draws (tests/ortho_ref.py: x -4 .. 12, y 0 .. 12, heights
    -0.47 .. 0.43): from the south-west at about 50 degrees elevation, 32 x 24 texels of about 0.55 world units."""
    from gswt_renderer_amd import ortho
    return ortho.OrthoCamera(LIGHT_W, LIGHT_H, (-8.0, -6.0, 20.0), (4.0, 6.0, 0.0), (0.0, 0.0, 1.0), 6.5, 5.0, 45.0)


def plane_map(cam):
    """The plane case's map: blocks of 4 x 4 texels in a pattern of three values -- 0.0 (shadows everything), 1.0 (lights everything)
    and the depth of the plane z = 0 at the texel (splats above it are lit, splats below it shadowed) -- so that a good share of the
    2 x 2 footprints mixes two kinds."""
    from gswt_renderer_amd import shadows
    M = shadows.world_to_light(cam).astype(np.float64)
    H, W = cam.height, cam.width
    js, is_ = np.mgrid[0:H, 0:W]
    kind = ((is_ // 4) + (js // 4)) % 3
    # the depth of the world plane z = 0 under texel (i, j): invert (u, v) -> (x, y) on z = 0, then ld
    lx = (is_ + 0.5) / W * 2.0 - 1.0
    ly = 1.0 - (js + 0.5) / H * 2.0
    A = np.array([[M[0], M[4]], [M[1], M[5]]])
    xy = np.linalg.solve(A, np.stack([(lx - M[12]).reshape(-1), (ly - M[13]).reshape(-1)]))
    ground = (M[2] * xy[0] + M[6] * xy[1] + M[14]).reshape(H, W)
    Z = np.where(kind == 0, 0.0, np.where(kind == 1, 1.0, ground)).astype(F32)
    return Z
