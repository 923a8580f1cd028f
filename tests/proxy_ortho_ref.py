"""Float64 rasterisation of one gswt_proxy_render_ortho draw (include/gswt_hip.h, "orthographic proxy pass"): the proxy mesh of
tests/proxy_raster_ref.py under an affine projection.  It does not share the kernel's ray cast: nothing here is a ray.

The f32 lattice vertices (proxy_raster_ref.lattice / triangles: the same mesh, the same two triangles per cell, the same diagonal)
are projected with GP * V in float64 (GP = opengl_to_wgpu * projection, clip w = 1) to pixel coordinates
    px = (ndc.x + 1) / 2 * W - 0.5,   py = (1 - ndc.y) / 2 * H - 0.5        (pixel (x, y)'s centre has ndc ((x + .5) / W * 2 - 1, ...))
and every triangle's edge functions are evaluated over its bounding box.  Under an affine projection the screen-space barycentrics
ARE the world-space ones, so depth, mapped height, uv and the world position of the fragment are their plain linear blends.  The
nearest fragment with depth in [0, 1] that the clip height does not discard is what depth-test-Less rasterisation keeps.

Ambiguity bands as in the perspective reference: a candidate not behind the visible fragment with a barycentric within eps_edge of
an edge, depth within eps_depth of 0, of 1 or of the incoming depth, or mapped height within eps_clip of clip_height.

Colour: the pixel's uv on the hit triangle's plane (the blend of the f32 vertex xy / tile_width / 4), the stated LOD rule -- rho =
max |delta uv| * tex_size towards the right and the lower pixel ON THE SAME PLANE, lod = clamp(log2 rho, 0, n_mips - 1) -- and trilinear
Repeat taps times `brightness`.  With fog: the float64 F of tests/atmosphere_ref.py at |hit - cam_pos|, rgb (1 - F) + fog_color F.

`f32_clip_depth` is proxy_raster_ref's: per-vertex clip = (GP * V) p in f32, interpolated in f64 (w = 1 here).
"""
import numpy as np

from gswt_renderer_amd import ortho
from tests import atmosphere_ref as AR
from tests import proxy_raster_ref as R

F32 = np.float32
NO_HIT = R.NO_HIT
f32_clip_depth = R.f32_clip_depth
emulated_error = R.emulated_error


def camera(u):
    """(V [4, 4], GP [4, 4]) float64 from the block's f32 view / projection; the projection must be of ortho() form."""
    V = np.asarray(u.view[:], np.float64).reshape(4, 4).T
    P = np.asarray(u.projection[:], np.float64).reshape(4, 4).T
    G = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 0.5, 0.5], [0, 0, 0, 1]], np.float64)
    assert tuple(P[3]) == (0.0, 0.0, 0.0, 1.0) and P[0, 1] == P[0, 2] == P[1, 0] == P[1, 2] == P[2, 0] == P[2, 1] == 0.0, "ortho() form"
    return V, G @ P


def _project(u, W, H, pts):
    """Pixel-centre coordinates and depth [..., 3] of world points [..., 3]."""
    V, GP = camera(u)
    M = GP @ V
    q = np.einsum("rc,...c->...r", M[:, :3], pts) + M[:, 3]
    return np.stack([(q[..., 0] + 1.0) * 0.5 * W - 0.5, (1.0 - q[..., 1]) * 0.5 * H - 0.5, q[..., 2]], -1)


def _bary(S, x, y):
    """Barycentrics (l0, l1, l2) of points (x, y) against screen triangles S [n, 3, 3] (edge functions / doubled area)."""
    x0, y0, x1, y1, x2, y2 = S[:, 0, 0], S[:, 0, 1], S[:, 1, 0], S[:, 1, 1], S[:, 2, 0], S[:, 2, 1]
    den = (y1 - y2) * (x0 - x2) + (x2 - x1) * (y0 - y2)
    with np.errstate(divide="ignore", invalid="ignore"):
        l0 = ((y1 - y2) * (x - x2) + (x2 - x1) * (y - y2)) / den
        l1 = ((y2 - y0) * (x - x2) + (x0 - x2) * (y - y2)) / den
    return l0, l1, 1.0 - l0 - l1


def render(u, W, H, *, grid_dim=2048, height_map=None, mips=None, depth_in=None, rgba_in=None, fog=None,
           eps_edge=1e-4, eps_depth=1e-6, eps_clip=1e-5, uv_ulps=8.0, max_pairs=4_000_000):
    """One draw over the whole W x H target.  The dict of proxy_raster_ref.render (depth, rgba, frag, tri, margin, written, amb,
    col_tol, tris, mapped) plus 'bary' ([H, W, 3], nan without a fragment) and 'hit' ([H, W, 3] world position of the fragment).
    fog: a 32-byte gswt_atmosphere block (or None); only its fog part is read."""
    tris, mapped = R.triangles(u, grid_dim, height_map)
    S = _project(u, W, H, tris)                                           # [T, 3, (px, py, depth)]
    lo, hi = S.min(1), S.max(1)
    keep = ~((hi[:, 2] < -eps_depth) | (lo[:, 2] > 1.0 + eps_depth))
    bx0 = np.clip(np.floor(lo[:, 0]) - 1, 0, W).astype(np.int64)
    bx1 = np.clip(np.ceil(hi[:, 0]) + 1, -1, W - 1).astype(np.int64)
    by0 = np.clip(np.floor(lo[:, 1]) - 1, 0, H).astype(np.int64)
    by1 = np.clip(np.ceil(hi[:, 1]) + 1, -1, H - 1).astype(np.int64)
    keep &= (bx1 >= bx0) & (by1 >= by0)
    idx = np.nonzero(keep)[0]
    area = (bx1[idx] - bx0[idx] + 1) * (by1[idx] - by0[idx] + 1)
    use_clip = int(u.use_clip) == 1
    clip_h = float(F32(u.clip_height))

    npx = W * H
    best = np.full(npx, np.inf)
    best_tri = np.full(npx, NO_HIT, np.int64)
    best_l = np.full((npx, 3), np.nan)
    amb = np.zeros(npx, bool)
    band_pix, band_dep = [], []
    start, csum = 0, np.cumsum(area)
    while start < idx.size:
        base = csum[start - 1] if start else 0
        stop = max(int(np.searchsorted(csum, base + max_pairs, side="right")), start + 1)
        ti, a = idx[start:stop], area[start:stop]
        rep = np.repeat(np.arange(ti.size), a)
        loc = np.arange(rep.size) - np.repeat(np.cumsum(a) - a, a)
        bw = (bx1[ti] - bx0[ti] + 1)[rep]
        lx, ly = bx0[ti][rep] + loc % bw, by0[ti][rep] + loc // bw
        tri = ti[rep]
        l0, l1, l2 = _bary(S[tri], lx.astype(np.float64), ly.astype(np.float64))
        margin = np.minimum(np.minimum(l0, l1), l2)
        dep = l0 * S[tri, 0, 2] + l1 * S[tri, 1, 2] + l2 * S[tri, 2, 2]
        mh = l0 * mapped[tri, 0] + l1 * mapped[tri, 1] + l2 * mapped[tri, 2]
        fin = np.isfinite(margin)
        kept = ~(mh < clip_h) if use_clip else np.ones(mh.shape, bool)
        ok = fin & (margin >= 0.0) & (dep >= 0.0) & (dep <= 1.0) & kept
        pix = ly * W + lx
        near = fin & (margin > -eps_edge)
        a_edge = near & (margin < eps_edge) & (dep > -eps_depth) & (dep < 1.0 + eps_depth) & ((not use_clip) | (mh > clip_h - eps_clip))
        a_plane = near & ((np.abs(dep) < eps_depth) | (np.abs(dep - 1.0) < eps_depth))
        a_clip = near & use_clip & (np.abs(mh - clip_h) < eps_clip) & (dep > -eps_depth) & (dep < 1.0 + eps_depth)
        a_any = a_edge | a_plane | a_clip
        band_pix.append(pix[a_any])
        band_dep.append(dep[a_any])
        if np.any(ok):
            p, dd, tt, ll = pix[ok], dep[ok], tri[ok], np.stack([l0[ok], l1[ok], l2[ok]], -1)
            order = np.lexsort((dd, p))
            p, dd, tt, ll = p[order], dd[order], tt[order], ll[order]
            first = np.r_[True, p[1:] != p[:-1]]
            p, dd, tt, ll = p[first], dd[first], tt[first], ll[first]
            better = dd < best[p]
            p, dd, tt, ll = p[better], dd[better], tt[better], ll[better]
            best[p], best_tri[p], best_l[p] = dd, tt, ll
        start = stop

    if band_pix:
        bp, bd = np.concatenate(band_pix), np.concatenate(band_dep)
        amb[bp[bd <= best[bp] + eps_depth]] = True                       # not hidden behind the visible fragment
    shape = (H, W)
    dep_in = np.ones(npx) if depth_in is None else np.asarray(depth_in, np.float64).reshape(npx)
    out_d = dep_in.copy()
    hit = best_tri != NO_HIT
    written = hit & (best < dep_in)                                       # CompareFunction::Less
    amb |= hit & (np.abs(best - dep_in) < eps_depth)
    out_d[written] = best[written]
    rgba = (np.zeros((npx, 4)) if rgba_in is None else np.asarray(rgba_in, np.float64).reshape(npx, 4).copy())
    ys, xs = np.divmod(np.arange(npx), W)
    world = np.full((npx, 3), np.nan)
    world[hit] = np.einsum("nv,nvc->nc", best_l[hit], tris[best_tri[hit]])
    col_tol = np.zeros(npx)
    if np.any(written):
        if int(u.black_background) == 1:
            rgba[written] = (0.0, 0.0, 0.0, 1.0)
        else:
            rgba[written], col_tol[written] = _shade(u, tris, S, best_tri[written], xs[written], ys[written], mips, uv_ulps)
            if fog is not None and AR.params(fog)["fog_on"]:
                p = AR.params(fog)
                cp = np.array([float(F32(u.cam_pos[k])) for k in range(3)])
                F = AR.fog_amount_f64(np.sqrt(((world[written] - cp) ** 2).sum(1)), p)[:, None]
                rgba[written, :3] = rgba[written, :3] * (1.0 - F) + p["fog_color"].astype(np.float64)[None] * F
    return dict(depth=out_d.reshape(shape), rgba=rgba.reshape(shape + (4,)), frag=np.where(hit, best, np.nan).reshape(shape),
                tri=best_tri.reshape(shape), margin=best_l.min(1).reshape(shape),
                written=written.reshape(shape), amb=amb.reshape(shape), col_tol=col_tol.reshape(shape), tris=tris, mapped=mapped,
                bary=best_l.reshape(shape + (3,)), hit=world.reshape(shape + (3,)))


def _uv_on_plane(u, tris, S, tri, xs, ys):
    l0, l1, l2 = _bary(S[tri], np.asarray(xs, np.float64), np.asarray(ys, np.float64))
    P = tris[tri]
    xy = l0[:, None] * P[:, 0, :2] + l1[:, None] * P[:, 1, :2] + l2[:, None] * P[:, 2, :2]
    return xy / float(F32(u.tile_width)) / 4.0


def _shade(u, tris, S, tri, xs, ys, mips, uv_ulps):
    """(rgba [n, 4], colour tolerance [n]); the tolerance is proxy_raster_ref._shade's: what a uv off by uv_ulps ulp_f32(|uv|) can
    move the trilinear sample by."""
    uv = _uv_on_plane(u, tris, S, tri, xs, ys)
    uvx = _uv_on_plane(u, tris, S, tri, xs + 1, ys)
    uvy = _uv_on_plane(u, tris, S, tri, xs, ys + 1)
    n = len(mips)
    size = np.asarray(mips[0]).shape[0]
    rho = np.maximum(np.linalg.norm((uvx - uv) * size, axis=1), np.linalg.norm((uvy - uv) * size, axis=1))
    with np.errstate(divide="ignore", invalid="ignore"):
        lod = np.log2(rho)
    lod = np.clip(np.nan_to_num(lod, nan=0.0, neginf=0.0), 0.0, n - 1)
    l0 = np.floor(lod).astype(np.int64)
    l1 = np.minimum(l0 + 1, n - 1)
    fl = (lod - l0)[:, None]
    c0, c1 = np.empty((tri.size, 3)), np.empty((tri.size, 3))
    for lvl in range(n):
        img = np.asarray(mips[lvl], np.float64)[..., :3]
        m0, m1 = l0 == lvl, l1 == lvl
        if m0.any():
            c0[m0] = R._bilinear_repeat(img, uv[m0, 0], uv[m0, 1])
        if m1.any():
            c1[m1] = R._bilinear_repeat(img, uv[m1, 0], uv[m1, 1])
    out = np.ones((tri.size, 4))
    br = float(F32(u.brightness))
    out[:, :3] = (c0 * (1.0 - fl) + c1 * fl) * br
    m0 = np.asarray(mips[0], np.float64)[..., :3]
    step = max(np.abs(np.diff(m0, axis=0)).max(initial=0.0), np.abs(np.diff(m0, axis=1)).max(initial=0.0),
               np.abs(m0[0] - m0[-1]).max(), np.abs(m0[:, 0] - m0[:, -1]).max())
    contrast = max(np.abs(np.asarray(mips[k], np.float64)[..., :3]).max() for k in range(n))
    du = uv_ulps * np.spacing(np.abs(uv).max(1).astype(F32)).astype(np.float64)
    dlod = np.where(rho > 1.0, 2.0 * np.sqrt(2.0) * du * size / (np.maximum(rho, 1.0) * np.log(2.0)), 0.0)
    return out, (du * size * step + np.minimum(dlod, 1.0) * contrast) * br


def reference(us, W, H, *, grid_dim, hm, mips, eps_edge=1e-4, fog=None):
    """The draws in order into one target (depth cleared to 1, colour = proxy_raster_ref.sky): final depth, colour, the union of the
    draws' ambiguity masks, the result dict per draw, and the per-pixel colour tolerance of the fragment each pixel kept."""
    depth, rgba = np.ones((H, W)), R.sky(W, H).astype(np.float64)
    amb, col_tol, res = np.zeros((H, W), bool), np.zeros((H, W)), []
    for u in us:
        r = render(u, W, H, grid_dim=grid_dim, height_map=hm, mips=mips, depth_in=depth, rgba_in=rgba, eps_edge=eps_edge, fog=fog)
        depth, rgba, amb = r["depth"], r["rgba"], amb | r["amb"]
        col_tol = np.where(r["written"], r["col_tol"], col_tol)
        res.append(r)
    return depth, rgba, amb, res, col_tol


# ---- scenes shared by tests/test_proxy_ortho_cpu.py (the reference's own conditions) and tests/test_proxy_ortho_gpu.py (k_proxy<., ORTHO>) --
W0, H0 = R.W0, R.H0
UPZ = (0.0, 0.0, 1.0)
FAR = dict(eps_edge=1e-2, colour="ulp", max_amb=0.1)          # proxy_raster_ref.FAR_OPT without its depth rule: here every scene has it


def _td(*a):
    return ("top_down",) + a


def _cam(eye, target, half_height, near, far, up=UPZ):
    return ("look", eye, target, up, half_height, near, far)


ISO = _cam((-40.0, -50.0, 40.0), (5.0, 3.0, 0.0), 35.0, 1.0, 160.0)
FAR_CAM = _cam((99863.0, 92452.0, 40.0), (99908.0, 92505.0, 0.0), 35.0, 1.0, 160.0)

# name: (camera, [draw fields], grid_dim, height-map size, options)
SCENES = {
    "top_down": (_td((1.3, 2.1), 30.0, 10.0, -10.0), [R._map()], 24, 16, {}),
    "top_down_hm12": (_td((1.3, 2.1), 30.0, 10.0, -10.0), [R._map()], 24, 12, {}),
    "top_down_near_cuts": (_td((1.3, 2.1), 30.0, 0.2, -1.0), [R._map()], 24, 16, {}),
    "isometric": (ISO, [R._map()], 24, 16, {}),
    "grazing": (_cam((-60.0, 0.7, 6.0), (0.0, 0.7, 0.0), 12.0, 1.0, 140.0), [R._map()], 24, 16, {}),
    "level_along_x": (_cam((-50.0, 0.3, 0.5), (0.0, 0.3, 0.5), 4.0, 1.0, 120.0), [R._map()], 24, 16, {}),
    "sun": (_cam((30.0, -60.0, 45.0), (0.0, 0.0, 0.0), 45.0, 10.0, 140.0), [R._map()], 24, 16, {}),
    "full_grid_flat": (_cam((3.0, -9.0, 20.0), (8.0, 20.0, -2.0), 40.0, 1.0, 120.0), [R._full(surface_type=0)], 24, 16, {}),
    "far_1e5": (FAR_CAM, [R._map(tile_width=3.7, center_coord=(27000, 25000))], 24, 16, FAR),
    # further scenes on the isometric camera
    "two_draws": (ISO, [R._full(), R._map(height_offset=-0.45)], 24, 16, {}),
    "two_draws_clip": (ISO, [R._full(use_clip=1, clip_height=0.3), R._map(use_clip=1, clip_height=0.3, height_offset=-0.45)], 24, 16, {}),
    "black_background": (ISO, [R._map(black_background=1, brightness=0.5)], 24, 16, {}),
    "far_1e5_full_grid": (FAR_CAM, [R._full(tile_width=3.7, width_scale=5.3, center_coord=(27000, 25000))], 24, 16, FAR),
}
TABULATED = ("top_down", "top_down_hm12", "top_down_near_cuts", "isometric", "grazing", "level_along_x", "sun", "full_grid_flat", "far_1e5")
# the issue's float64 prototype at 257 x 161: coverage of the reference per tabulated scene
COVERAGE = dict(top_down=0.875, top_down_hm12=0.875, top_down_near_cuts=0.677, isometric=0.448, grazing=0.370, level_along_x=0.248,
                sun=0.304, full_grid_flat=0.400, far_1e5=0.385)


def make_camera(spec, W, H, lod_pos=None):
    if spec[0] == "top_down":
        return ortho.top_down(spec[1], spec[2], spec[3], spec[4], W, H, lod_pos=lod_pos)
    _, eye, target, up, hh, near, far = spec
    return ortho.OrthoCamera(W, H, eye, target, up, hh, near, far, lod_pos=lod_pos)


def scene_uniforms(cam, draws):
    return [cam.proxy_uniforms(tile_width=d.get("tile_width", 4.0), width_scale=d.get("width_scale", 4.0),
                               **{k: v for k, v in d.items() if k not in ("tile_width", "width_scale")}) for d in draws]


_CACHE = {}


def scene_reference(name, fog=None, lod_pos=None):
    """(uniform blocks, grid_dim, height map, mips, options, reference(...) tuple) of a scene -- computed once per process and
    shared by the tests; nobody writes into it."""
    key = (name, None if fog is None else bytes(fog), None if lod_pos is None else tuple(lod_pos))
    if key not in _CACHE:
        spec, draws, grid_dim, hm_n, opt = SCENES[name]
        us = scene_uniforms(make_camera(spec, W0, H0, lod_pos=lod_pos), draws)
        hm, mips = R.height_map(n=hm_n), R.mip_chain()
        ref = reference(us, W0, H0, grid_dim=grid_dim, hm=hm, mips=mips, eps_edge=opt.get("eps_edge", 1e-4), fog=fog)
        _CACHE[key] = (us, grid_dim, hm, mips, opt, ref)
    return _CACHE[key]


DEPTH_FACTOR = 2.0          # tests/test_proxy_raster_cpu.py's far-scene rule, here for every scene


def depth_tol(us, W, H, res, amb, factor=DEPTH_FACTOR):
    """factor x the f32 rasteriser emulation's error + 1e-6, and that error."""
    emu = emulated_error(us, W, H, res, amb)
    return factor * emu + 1e-6, emu


def incidence(us, res, y, x):
    """|cos| of the angle between the view axis and the normal of the triangle the reference shows at pixel (y, x): small where the
    surface is seen edge-on, and a lateral rounding of the sample point moves the depth by 1 / tan of that."""
    for u, r in reversed(list(zip(us, res))):
        if r["written"][y, x]:
            p = r["tris"][r["tri"][y, x]]
            n = np.cross(p[1] - p[0], p[2] - p[0])
            a = np.array([u.view[2], u.view[6], u.view[10]], np.float64)
            return float(abs(n @ a) / np.linalg.norm(n) / np.linalg.norm(a))
    return float("nan")
