"""Float64 reference of one gswt_proxy_render_sphere draw (include/gswt_hip.h, "sphere proxy pass"): the pixel's ray cut with the sphere of
radius sphere_radius + height_offset about the world origin, the inverse of the sphere unfolding for the texture coordinate, trilinear Repeat
texturing, shade and fog.  numpy only; nothing here is shared with the kernel or with host/gswt_surface.h.

`evaluate(..., ft)` writes the header's definition down once in the float type `ft`: float64 is the reference, float32 the "binary32
restatement of the same operator sequence" whose distance from float64 scales the depth bound (tests/test_proxy_raster_cpu.py's rule).

A pixel is AMBIGUOUS when a binary32 rounding could flip one of its decisions: relative disc within 1e-5 of 0, a candidate that decides the
pixel within 1e-6 of depth 0 / 1 or of the incoming depth, its clipped height within 1e-5 of clip_height, v within 1e-6 of 1/3 or 2/3, f
within 1e-6 of 0, 1 or (mid bands) 1 - w, and, with a shadow map, a tap whose depth compare lies within 1e-5 of equality."""
import math

import numpy as np

from tests import atmosphere_ref as AR
from tests import proxy_raster_ref as R
from tests import shadow_ref as SR

F32 = np.float32
DEPTH_FACTOR = 2.0
EPS_DISC, EPS_DEPTH, EPS_CLIP, EPS_BAND, EPS_F, EPS_SHADOW = 1e-5, 1e-6, 1e-5, 1e-6, 1e-6, 1e-5


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


# ---- the unfolding ---------------------------------------------------------------------------------------------------------------
def block_width(u, ft=np.float64):
    """bw = (2 half_w tile_width) / 5."""
    return (ft(2.0) * ft(int(u.map_half_wh[0])) * ft(F32(u.tile_width))) / ft(5.0)


def _mod5(x, ft):
    t = x - ft(5.0) * np.floor(x / ft(5.0))
    return np.where((t >= ft(5.0)) | (t < ft(0.0)), ft(0.0), t).astype(ft)


def inverse_unfold(n, bw, ft=np.float64):
    """Unit directions n [..., 3] -> (px, py, info): the plane position relative to the unfolding's origin, px = bidx bw + bx and
    py = bidy bw + by, and info = dict(v, f, w, band, bidx, bidy) -- band 0 south caps, 1 mid bands, 2 north caps; w is nan off the mid bands."""
    n = np.asarray(n, ft)
    bw = ft(bw)
    pi = ft(math.pi)
    one, three, five, half = ft(1.0), ft(3.0), ft(5.0), ft(0.5)
    v = (np.arcsin(np.clip(n[..., 2], -one, one)) / pi + half).astype(ft)
    u = (np.arctan2(n[..., 1], n[..., 0]) / (ft(2.0) * pi)).astype(ft)
    u = (u - np.floor(u)).astype(ft)
    u = np.where(u >= one, ft(0.0), u).astype(ft)
    south, north = v < one / three, v >= ft(2.0) / three
    band = np.where(south, 0, np.where(north, 2, 1))
    # south caps
    s_s = three * v
    t_s = _mod5(five * u, ft)
    # mid bands
    w_m = three * v - one
    t_m = _mod5(five * u - half * w_m, ft)
    # north caps
    s_n = three * v - ft(2.0)
    t_n = _mod5(five * u - half, ft)
    t = np.where(south, t_s, np.where(north, t_n, t_m)).astype(ft)
    bidx = np.minimum(np.floor(t), ft(4.0)).astype(ft)
    f = (t - bidx).astype(ft)
    by_s = f * bw * s_s
    bx_s = by_s + bw * (one - s_s)
    bx_m = f * bw
    low = f <= one - w_m
    by_m = np.where(low, bx_m + w_m * bw, bx_m - bw * (one - w_m))
    bx_n = f * bw * (one - s_n)
    by_n = bx_n + s_n * bw
    bx = np.where(south, bx_s, np.where(north, bx_n, bx_m)).astype(ft)
    by = np.where(south, by_s, np.where(north, by_n, by_m)).astype(ft)
    bidy = np.where(south, ft(0.0), np.where(north, one, np.where(low, ft(0.0), one))).astype(ft)
    px = (bidx * bw + bx).astype(ft)
    py = (bidy * bw + by).astype(ft)
    return px, py, dict(v=v, f=f, w=np.where(band == 1, w_m, np.nan), band=band, bidx=bidx, bidy=bidy, bx=bx, by=by)


def forward_unfold(bw, bidx, bidy, bx, by):
    """sphere_get_uv + sphere_uv_to_pos in float64 with exact sin / cos: block (bidx, bidy), position (bx, by) in it -> unit direction."""
    bw, bx, by = float(bw), np.asarray(bx, np.float64), np.asarray(by, np.float64)
    bidx, bidy = np.asarray(bidx, np.float64), np.asarray(bidy, np.float64)
    lower = by < bx
    with np.errstate(divide="ignore", invalid="ignore"):
        k = np.where(lower, bw - (bx - by), by - bx)              # bidy 0: cap below / band above the diagonal; bidy 1: band / cap
        u00 = np.where(bx - by == bw, 0.0, (by / (bw - (bx - by)) + bidx) / 5.0)
        v00 = k / bw / 3.0
        u01 = (bx / bw + bidx) / 5.0 + (by - bx) / bw * 0.1
        v01 = (by - bx) / bw / 3.0 + 1.0 / 3.0
        u10 = (bx / bw + bidx) / 5.0 + (bw - (bx - by)) / bw * 0.1
        v10 = (bw - (bx - by)) / bw / 3.0 + 1.0 / 3.0
        u11 = np.where(by - bx == bw, 0.0, (bx / (bw - (by - bx)) + bidx) / 5.0 + 0.1)
        v11 = (by - bx) / bw / 3.0 + 2.0 / 3.0
    first = bidy == 0
    u = np.where(first, np.where(lower, u00, u01), np.where(lower, u10, u11))
    v = np.where(first, np.where(lower, v00, v01), np.where(lower, v10, v11))
    u = (u + 0.5 * np.floor(v)) * (2.0 * math.pi)
    v = (v - 0.5) * math.pi
    return np.stack([np.cos(v) * np.cos(u), np.cos(v) * np.sin(u), np.sin(v)], -1)


def plane_origin(u, ft=np.float64):
    """(center_coord - half) tile_width: the origin map_sphere_surface subtracts."""
    tw = ft(F32(u.tile_width))
    return (ft(int(u.center_coord[0]) - int(u.map_half_wh[0])) * tw, ft(int(u.center_coord[1]) - int(u.map_half_wh[1])) * tw)


# ---- rays ------------------------------------------------------------------------------------------------------------------------
def _gp(u, ft):
    """opengl_to_wgpu * projection as the library forms it in binary32 (row 2 = 0.5 row 2 + 0.5 row 3), [r, c]."""
    P = np.asarray(u.projection[:], F32).reshape(4, 4).T
    GP = P.copy()
    GP[2] = F32(0.5) * P[2] + F32(0.5) * P[3]
    return GP.astype(ft)


def ortho_setup(u):
    """The host part of the orthographic pass with g = 0, binary64: (e [3], d [3], sz)."""
    GP = _gp(u, np.float64)
    V = np.asarray(u.view[:], np.float64).reshape(4, 4).T
    g10, g14 = GP[2, 2], GP[2, 3]
    zn, zf = (0.0 - g14) / g10, (1.0 - g14) / g10
    sz = -1.0 if g10 < 0.0 else 1.0
    z0 = zn - sz * 0.125 * abs(zf - zn)
    e = np.linalg.solve(V[:3, :3], np.array([0.0, 0.0, z0]) - V[:3, 3])
    return e, sz * V[2, :3], sz


def rays(u, W, H, projection, ft, xs, ys):
    """(o [n, 3], d [n, 3]) of pixels (xs, ys) in the float type ft, by the header's operator sequence."""
    V = np.asarray(u.view[:], F32).reshape(4, 4).T.astype(ft)
    P = np.asarray(u.projection[:], F32).astype(ft)
    nx = (np.asarray(xs, ft) + ft(0.5)) / ft(W) * ft(2.0) - ft(1.0)
    ny = ft(1.0) - (np.asarray(ys, ft) + ft(0.5)) / ft(H) * ft(2.0)
    if projection == 0:
        vx, vy, vz = nx / P[0], ny / P[5], ft(-1.0)
        d = np.stack([(V[0, k] * vx + V[1, k] * vy) + V[2, k] * vz for k in range(3)], -1).astype(ft)
        o = np.broadcast_to(np.asarray(u.cam_pos[:3], F32).astype(ft), d.shape)
        return o, d
    e, dv, _ = ortho_setup(u)
    e, dv = e.astype(ft), dv.astype(ft)                    # (binary32: each rounded once, as the host does)
    cx, cy = (nx - P[12]) / P[0], (ny - P[13]) / P[5]
    o = np.stack([(V[0, k] * cx + V[1, k] * cy) + e[k] for k in range(3)], -1).astype(ft)
    return o, np.broadcast_to(dv, o.shape)


def cut(o, d, r, ft, clamp=False):
    """(tc, h, dd, disc): tc = -(o.d) / dd, c = o + tc d, disc = r r - c.c, h = sqrt(disc / dd) (nan where disc < 0 unless clamped)."""
    dd = _dot(d, d)
    tc = -_dot(o, d) / dd
    c = o + tc[..., None] * d
    disc = r * r - _dot(c, c)
    dc = np.maximum(disc, ft(0.0)) if clamp else disc
    with np.errstate(invalid="ignore"):
        h = np.sqrt(dc / dd)
    return tc.astype(ft), h.astype(ft), dd.astype(ft), disc.astype(ft)


def _depth(u, hit, ft):
    V = np.asarray(u.view[:], F32).reshape(4, 4).T.astype(ft)
    GP = _gp(u, ft)
    cv = [((V[r, 0] * hit[..., 0] + V[r, 1] * hit[..., 1]) + V[r, 2] * hit[..., 2]) + V[r, 3] for r in range(4)]
    q = [((GP[r, 0] * cv[0] + GP[r, 1] * cv[1]) + GP[r, 2] * cv[2]) + GP[r, 3] * cv[3] for r in range(4)]
    with np.errstate(divide="ignore", invalid="ignore"):
        return (q[2] / q[3]).astype(ft), q[3]


def evaluate(u, sphere_radius, W, H, projection=0, ft=np.float64, depth_in=None):
    """The geometry of one draw in float type ft, per pixel [H, W]: hit (bool), root (0 / 1), t, dep, pos [.., 3], and the ambiguity mask of
    the geometric decisions (float64 thresholds, whatever ft)."""
    ys, xs = np.mgrid[0:H, 0:W]
    o, d = rays(u, W, H, projection, ft, xs.ravel(), ys.ravel())
    sr, r = ft(F32(sphere_radius)), ft(F32(sphere_radius)) + ft(F32(u.height_offset))
    tc, h, dd, disc = cut(o, d, r, ft)
    din = np.ones(W * H) if depth_in is None else np.asarray(depth_in, np.float64).ravel()
    use_clip, clip_h = int(u.use_clip) == 1, ft(F32(u.clip_height))
    kept, amb_c, ts, deps, poss = [], [], [], [], []
    for sgn in (-1.0, 1.0):
        t = tc + ft(sgn) * h
        pos = o + t[..., None] * d
        dep, qw = _depth(u, pos, ft)
        mh = (pos[..., 2] / r) * sr
        with np.errstate(invalid="ignore"):
            alive = (disc >= 0) & (t > 0) & (qw > 0)
            ok = alive & (dep >= 0) & (dep <= 1) & ~(use_clip & (mh < clip_h))
            a = alive & ((np.abs(dep) < EPS_DEPTH) | (np.abs(dep - 1.0) < EPS_DEPTH) | (np.abs(dep - din) < EPS_DEPTH) |
                         (use_clip & (np.abs(mh - clip_h) < EPS_CLIP)))
        kept.append(ok); amb_c.append(a); ts.append(t); deps.append(dep); poss.append(pos)
    hit = kept[0] | kept[1]
    root = np.where(kept[0], 0, 1)
    pick = lambda pair: np.where(kept[0].reshape(kept[0].shape + (1,) * (pair[0].ndim - 1)), pair[0], pair[1])
    with np.errstate(invalid="ignore"):
        amb = (np.abs(disc) / (r * r) < EPS_DISC) | amb_c[0] | (~kept[0] & amb_c[1])
    sh = (H, W)
    return dict(hit=hit.reshape(sh), root=root.reshape(sh), t=pick(ts).reshape(sh), dep=pick(deps).astype(np.float64).reshape(sh),
                pos=pick(poss).reshape(sh + (3,)), amb=amb.reshape(sh), o=o.reshape(sh + (3,)), d=d.reshape(sh + (3,)), dd=dd.reshape(sh),
                r=r, sr=sr)


def _neighbour_hit(u, W, H, projection, xs, ys, root, r):
    o, d = rays(u, W, H, projection, np.float64, xs, ys)
    tc, h, _, _ = cut(o, d, r, np.float64, clamp=True)
    t = np.where(root == 0, tc - h, tc + h)
    return o + t[..., None] * d


def texture(u, W, H, projection, g, mips, shift=(0.0, 0.0)):
    """rgb [n, 3] (brightness applied) of the hit pixels of geometry g (float64), their plane position displaced by `shift`; and the
    unfolding's info."""
    m = g["hit"]
    ys, xs = np.nonzero(m)
    r = float(g["r"])
    pos = g["pos"][m].astype(np.float64)
    bw = block_width(u)
    px, py, info = inverse_unfold(pos / r, bw)
    ox, oy = plane_origin(u)
    tw = float(F32(u.tile_width))
    uv = np.stack([(ox + px + shift[0]) / tw / 4.0, (oy + py + shift[1]) / tw / 4.0], -1)
    root = g["root"][m]
    hx = _neighbour_hit(u, W, H, projection, xs + 1, ys, root, r)
    hy = _neighbour_hit(u, W, H, projection, xs, ys + 1, root, r)
    n = len(mips)
    size = np.asarray(mips[0]).shape[0]
    k = int(u.map_half_wh[0]) * size / (4.0 * math.pi * r)
    rho = np.maximum(np.linalg.norm(hx - pos, axis=1), np.linalg.norm(hy - pos, axis=1)) * k
    with np.errstate(divide="ignore", invalid="ignore"):
        lod = np.log2(rho)
    lod = np.clip(np.nan_to_num(lod, nan=0.0, neginf=0.0), 0.0, n - 1)
    l0 = np.floor(lod).astype(np.int64)
    l1 = np.minimum(l0 + 1, n - 1)
    fl = (lod - l0)[:, None]
    c0, c1 = np.empty((ys.size, 3)), np.empty((ys.size, 3))
    for lvl in range(n):
        img = np.asarray(mips[lvl], np.float64)[..., :3]
        m0, m1 = l0 == lvl, l1 == lvl
        if m0.any():
            c0[m0] = R._bilinear_repeat(img, uv[m0, 0], uv[m0, 1])
        if m1.any():
            c1[m1] = R._bilinear_repeat(img, uv[m1, 0], uv[m1, 1])
    return (c0 * (1.0 - fl) + c1 * fl) * float(F32(u.brightness)), info


def shade(u, projection, g, rgb, fog=None, shadow=None):
    """Shadow then fog on rgb [n, 3] of g's hit pixels, float64; and the shadow's ambiguity per hit pixel."""
    m = g["hit"]
    pos = g["pos"][m].astype(np.float64)
    amb = np.zeros(pos.shape[0], bool)
    if shadow is not None and not shadow.is_off:
        p = SR.params(shadow)
        sh, _, outside, (_, _, ld) = SR.lookup_f64((pos[:, 0], pos[:, 1], pos[:, 2]), p)
        rgb = rgb * (1.0 - sh[:, None]) + p["shade"].astype(np.float64)[None, :] * sh[:, None]
        rr = ld - float(p["bias"])
        zs = np.unique(p["Z"].astype(np.float64))
        amb = ~outside & (np.abs(rr[:, None] - zs[None, :]) < EPS_SHADOW).any(1) if zs.size <= 64 else ~outside
    if fog is not None:
        a = AR.params(fog)
        if a["fog_on"]:
            if projection == 0:
                dist = g["t"][m].astype(np.float64) * np.sqrt(g["dd"][m].astype(np.float64))
            else:
                dist = np.linalg.norm(pos - np.asarray(u.cam_pos[:3], np.float64), axis=1)
            F = AR.fog_amount_f64(dist, a)[:, None]
            rgb = rgb * (1.0 - F) + a["fog_color"].astype(np.float64)[None, :] * F
    return rgb, amb


def plane_delta(u):
    """4 * 2^-23 * (2 half_w tile_width): 2 ulp each for atan2f and asinf at the size of the unfolded map."""
    return 4.0 * 2.0 ** -23 * (2.0 * int(u.map_half_wh[0]) * float(F32(u.tile_width)))


def render(u, sphere_radius, W, H, *, projection=0, mips=None, depth_in=None, rgba_in=None, fog=None, shadow=None):
    """One draw: dict of depth / rgba after the draw, written, amb, col_tol (what the colour moves when the plane position moves by
    plane_delta in either axis), the float64 geometry `geo` and the binary32 restatement's depth error `emu` off the mask."""
    g = evaluate(u, sphere_radius, W, H, projection, np.float64, depth_in)
    g32 = evaluate(u, sphere_radius, W, H, projection, F32, depth_in)
    din = np.ones((H, W)) if depth_in is None else np.asarray(depth_in, np.float64).reshape(H, W)
    hit = g["hit"]
    with np.errstate(invalid="ignore"):
        written = hit & (g["dep"] < din)
    amb = g["amb"].copy()
    depth = np.where(written, g["dep"], din)
    rgba = np.zeros((H, W, 4)) if rgba_in is None else np.asarray(rgba_in, np.float64).reshape(H, W, 4).copy()
    col_tol = np.zeros((H, W))
    info = None
    if int(u.black_background) == 1:
        rgba[written] = (0.0, 0.0, 0.0, 1.0)
    elif hit.any():
        rgb, info = texture(u, W, H, projection, g, mips)
        d = plane_delta(u)
        moved = np.zeros(rgb.shape[0])
        for sx, sy in ((d, 0.0), (-d, 0.0), (0.0, d), (0.0, -d)):
            moved = np.maximum(moved, np.abs(texture(u, W, H, projection, g, mips, shift=(sx, sy))[0] - rgb).max(1))
        rgb, amb_s = shade(u, projection, g, rgb, fog, shadow)
        full = np.ones((rgb.shape[0], 4))
        full[:, :3] = rgb
        img = rgba.copy()
        img[hit] = full
        rgba = np.where(written[..., None], img, rgba)
        col_tol[hit] = moved
        third = 1.0 / 3.0
        v, f, w = info["v"], info["f"], info["w"]
        with np.errstate(invalid="ignore"):
            seam = (np.abs(v - third) < EPS_BAND) | (np.abs(v - 2.0 * third) < EPS_BAND) | (f < EPS_F) | (f > 1.0 - EPS_F) | \
                   ((info["band"] == 1) & (np.abs(f - (1.0 - w)) < EPS_F))
        a = np.zeros((H, W), bool)
        a[hit] = seam | amb_s
        amb |= a
    both = hit & g32["hit"] & ~amb
    emu = float(np.abs(g32["dep"] - g["dep"])[both].max()) if both.any() else 0.0
    return dict(depth=depth, rgba=rgba, written=written, amb=amb, col_tol=col_tol, geo=g, geo32=g32, emu=emu, info=info)


# ---- scenes shared by tests/test_proxy_sphere_cpu.py and tests/test_proxy_sphere_gpu.py ------------------------------------------
W0, H0 = 96, 72
RADIUS = 6.5
BLOCK = dict(map_half_wh=(5, 2), tile_width=4.0, height_offset=-0.25, brightness=0.9)          # r = 6.25; the unfolded map is 40 x 16
UPZ, UPY = (0.0, 0.0, 1.0), (0.0, 1.0, 0.0)


def _persp(pos, tgt, up=UPZ, z_near=0.1, z_far=2400.0):
    return dict(kind="persp", pos=pos, tgt=tgt, up=up, z_near=z_near, z_far=z_far)


def _ortho(eye, tgt, hh, near, far, up=UPZ, lod_pos=None):
    return dict(kind="ortho", eye=eye, tgt=tgt, up=up, hh=hh, near=near, far=far, lod_pos=lod_pos)


def fog_block():
    from gswt_renderer_amd import atmosphere as A
    return A.Atmosphere(fog=(0.08, 6.0, 0.9, (0.6, 0.7, 0.8)))


def shadow_block():
    """A sun along -x over the whole planet, 32 x 32: the left half of its image (world y < 0) holds depth 0 (shadows everything behind
    it), the right half depth 1 (lights everything), so no compare is close; the column between them mixes the two bilinearly."""
    from gswt_renderer_amd import ortho, shadows
    cam = ortho.OrthoCamera(32, 32, (20.0, 0.0, 0.0), (0.0, 0.0, 0.0), UPZ, 8.0, 1.0, 40.0)
    return shadows.from_ortho_camera(cam, SR.two_region_map(32, 32), bias=0.0, strength=0.75, shade_color=(0.05, 0.1, 0.2))


# name: (camera, block fields, options).  Options: size (W, H), fog, shadow, second (a second draw over an incoming depth nearer on half
# the frame: the first draw's fields), depth_in.
SCENES = {
    "equatorial": (_persp((19.0, 1.5, 0.8), (0.0, 0.0, 0.0)), {}, {}),
    "north_pole": (_persp((0.7, 0.45, 21.0), (0.0, 0.0, 0.0), up=UPY), {}, {}),
    "south_pole": (_persp((-0.55, 0.8, -20.0), (0.0, 0.0, 0.0), up=UPY), {}, {}),
    "oblique": (_persp((-11.0, 9.0, 12.0), (1.0, -0.5, 0.5)), {}, {}),
    "grazing_horizon": (_persp((4.0, -3.5, 3.6), (-6.0, 4.0, 5.5)), {}, {}),          # |eye| = 6.39, 0.14 above r = 6.25
    "inside": (_persp((1.0, -2.0, 0.5), (6.0, 3.0, 1.0)), {}, {}),
    "clip_cap": (_persp((14.0, -10.0, -6.0), (0.0, 0.0, 0.5)), dict(use_clip=1, clip_height=2.0), {}),
    "incoming_depth": (_persp((19.0, 1.5, 0.8), (0.0, 0.0, 0.0)), {}, dict(depth_in="half")),
    "black_background": (_persp((-11.0, 9.0, 12.0), (1.0, -0.5, 0.5)), dict(black_background=1), {}),
    "fog": (_persp((-11.0, 9.0, 12.0), (1.0, -0.5, 0.5)), {}, dict(fog=True)),
    "shadow": (_persp((16.0, 1.0, 6.0), (0.0, 0.0, 0.0)), {}, dict(shadow=True)),
    "ortho_planet": (_ortho((14.0, -12.0, 9.0), (0.0, 0.0, 0.0), 7.5, 1.0, 40.0), {}, {}),
    "ortho_near_negative": (_ortho((2.0, 1.5, 1.0), (0.0, 0.0, 0.0), 7.0, -2.0, 20.0, lod_pos=(9.0, 8.0, 4.0)), {}, dict(fog=True)),
    "partial_blocks": (_persp((-11.0, 9.0, 12.0), (1.0, -0.5, 0.5)), {}, dict(size=(101, 67))),
}


def scene_block(name):
    """(uniform block, projection, W, H, options)."""
    from gswt_renderer_amd import ortho
    from oracle import gswt_oracle as orc
    cam, fields, opt = SCENES[name]
    W, H = opt.get("size", (W0, H0))
    kw = dict(BLOCK)
    kw.update(fields)
    if cam["kind"] == "persp":
        c = orc.Camera(W, H, cam["pos"], cam["tgt"], list(cam["up"]), z_near=cam["z_near"], z_far=cam["z_far"])
        u = orc.proxy_uniforms(c, surface_type=2, map_proxy=1, **kw)
        return u, 0, W, H, opt
    c = ortho.OrthoCamera(W, H, cam["eye"], cam["tgt"], cam["up"], cam["hh"], cam["near"], cam["far"], lod_pos=cam["lod_pos"])
    return c.proxy_uniforms(surface_type=2, map_proxy=1, **kw), 1, W, H, opt


def incoming_depth(W, H, ref_depth):
    """An incoming depth image nearer than the sphere on the left half of the frame (and 1.0 on the right)."""
    d = np.ones((H, W), F32)
    near = float(np.nanmin(np.where(ref_depth < 1.0, ref_depth, np.nan)))
    d[:, :W // 2] = F32(near * 0.5)
    return d


_CACHE = {}


def scene_reference(name):
    """(block, projection, W, H, mips, fog, shadow, depth_in, result of render) -- computed once per process; nobody writes into it."""
    if name not in _CACHE:
        u, projection, W, H, opt = scene_block(name)
        mips = R.mip_chain()
        fog = fog_block() if opt.get("fog") else None
        shadow = shadow_block() if opt.get("shadow") else None
        depth_in = None
        if opt.get("depth_in") == "half":
            first = render(u, RADIUS, W, H, projection=projection, mips=mips, rgba_in=R.sky(W, H))
            depth_in = incoming_depth(W, H, first["depth"])
        res = render(u, RADIUS, W, H, projection=projection, mips=mips, depth_in=depth_in, rgba_in=R.sky(W, H), fog=fog, shadow=shadow)
        _CACHE[name] = (u, projection, W, H, mips, fog, shadow, depth_in, res)
    return _CACHE[name]


MAX_AMB, MIN_COVER = 0.02, 0.05


def conditions(res):
    """(share of the covered pixels on the mask, share of the frame covered)."""
    hit = res["geo"]["hit"]
    return float((res["amb"] & hit).sum() / max(int(hit.sum()), 1)), float(hit.mean())


def compare(got_depth, got_rgba, res, depth_in=None):
    """The assertions of the GPU test; returns (depth error, bound, colour error beyond the 1e-4 + col_tol allowance)."""
    got_depth = np.asarray(got_depth, np.float64)
    din = np.ones_like(got_depth) if depth_in is None else np.asarray(depth_in, np.float64)
    amb, written = res["amb"], res["written"]
    cov_g = got_depth != din
    bad = (cov_g != written) & ~amb
    assert not bad.any(), f"coverage differs off the mask at {int(bad.sum())} pixels, e.g. (y, x) = {np.argwhere(bad)[:4].tolist()}"
    share, cover = conditions(res)
    assert share <= MAX_AMB, f"the mask covers {share:.3%} of the covered pixels"
    assert cover >= MIN_COVER, f"the sphere covers {cover:.3%} of the frame"
    both = cov_g & written & ~amb
    derr = float(np.abs(got_depth - res["depth"])[both].max()) if both.any() else 0.0
    tol = DEPTH_FACTOR * res["emu"] + 1e-6
    assert derr <= tol, f"depth error {derr:.3e} > {tol:.3e}"
    err = np.abs(np.asarray(got_rgba, np.float64) - res["rgba"]).max(-1)
    over = (err - (1e-4 + res["col_tol"]))[~amb]
    cerr = float(over.max()) if over.size else 0.0
    assert cerr <= 0.0, f"colour beyond 1e-4 + the plane-delta allowance by {cerr:.3e} at {int((over > 0).sum())} pixels"
    return derr, tol, cerr
