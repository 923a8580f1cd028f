"""Float64 rasterisation of one Proxy::render draw (proxy.rs:366-447 + proxy.wgsl), independent of the oracle's ray cast.

The reference draws the proxy as a triangle mesh (proxy.rs:136-163 for the GRID_DIM grid, proxy.rs:219-251 for the tile-map
grid): six vertices per cell, (p, p), (p+1, p), (p, p+1) and (p+1, p), (p+1, p+1), (p, p+1), so the diagonal of every cell
runs from (i+1, j) to (i, j+1).  vs_main (proxy.wgsl:40-95) places a vertex at
  * map grid (map_proxy 1):  f32(f32((i - half) * tile_width) + f32(center_coord * tile_width))           (proxy.rs:247-250, :50)
  * full grid (map_proxy 0): f32(f32((i - G/2) * width_scale) + f32(floor(f32(center_coord * tile_width) / width_scale)
                             * width_scale))                                                                   (:66-67)
  * height: height_offset + mapped_height, mapped_height = bilinear Repeat sample of the R32Float height map at
    h_u = (x + half_x * tile_width) / ((2 half_x + 1) tile_width hms.x) (and v likewise), times hms.z         (:73-82)
and its clip position is opengl_to_wgpu * projection * view * (x, y, height, 1) (:84-91).  The pipeline (proxy.rs:96-134) has
no culling, depth compare Less with depth write on, and fs_main (:97-111) discards where use_clip == 1 and the interpolated
mapped_height < clip_height; otherwise it writes black (black_background) or textureSample(proxy texture, tex_coords =
real_position / tile_width / 4) * brightness, alpha 1 (trilinear, Repeat, implicit LOD).

Here the vertex coordinates are the f32 values above; everything after them is float64.  Each pixel centre's ray is cut with
every candidate triangle (Moeller-Trumbore in camera space, where the ray of pixel (x, y) is s (ndc_x / P00, ndc_y / P11, -1),
s > 0); the nearest fragment with w > 0, NDC depth z / w in [0, 1] and no clip discard is what a depth-Less rasteriser keeps.
A brute-force ray test differs from exact edge functions only within ~1e-12 of an edge.  Candidates are culled by the
triangle's screen bounding box when all three vertices lie in front of the eye; a triangle with a vertex at w <= 0 is tested
against every pixel of the window.

Colour: trilinear Repeat sampling of the given mip chain at the f64 uv, with the kernel's stated LOD rule (gswt_passes.hip
k_proxy): rho = max |d uv| * tex_size over the rays of the right and the lower pixel cut with the hit triangle's plane,
lod = clamp(log2 rho, 0, n_mips - 1).
"""
import numpy as np

F32 = np.float32
NO_HIT = -1


def _f32(x):
    return np.asarray(x, dtype=F32)


def _bilinear_repeat(img, u, v):
    """WebGPU bilinear with Repeat addressing at texel centres (x = u * w - 0.5), float64.  img [h, w] or [h, w, c]."""
    h, w = img.shape[:2]
    x = np.asarray(u, np.float64) * w - 0.5
    y = np.asarray(v, np.float64) * h - 0.5
    x0, y0 = np.floor(x), np.floor(y)
    fx, fy = x - x0, y - y0
    xa = np.mod(x0, w).astype(np.int64)
    ya = np.mod(y0, h).astype(np.int64)
    xb, yb = (xa + 1) % w, (ya + 1) % h
    im = np.asarray(img, np.float64)
    if im.ndim == 3:
        fx, fy = fx[..., None], fy[..., None]
    return ((im[ya, xa] * (1 - fx) + im[ya, xb] * fx) * (1 - fy) + (im[yb, xa] * (1 - fx) + im[yb, xb] * fx) * fy)


def lattice(u, grid_dim, height_map):
    """Vertex lattice of one draw: (X [nx+1] f32, Y [ny+1] f32, Z [nx+1, ny+1] f32, M [nx+1, ny+1] float64 mapped height).
    Lattice point (a, b) is the vertex of cell corner (a, b); the per-cell six vertices of proxy.rs are points of it."""
    tw = F32(u.tile_width)
    if int(u.map_proxy) == 1:
        hx, hy = int(u.map_half_wh[0]), int(u.map_half_wh[1])
        nx, ny = 2 * hx + 1, 2 * hy + 1
        px = _f32(np.arange(nx + 1) - hx) * tw                                     # proxy.rs:249 (position *= tile_width)
        py = _f32(np.arange(ny + 1) - hy) * tw
        X = px + F32(u.center_coord[0]) * tw                                        # proxy.wgsl:50
        Y = py + F32(u.center_coord[1]) * tw
    else:
        ws = F32(u.width_scale)
        nx = ny = int(grid_dim)
        p = _f32(np.arange(nx + 1) - nx // 2)
        ox = np.floor(F32(u.center_coord[0]) * tw / ws) * ws                        # proxy.wgsl:66-67
        oy = np.floor(F32(u.center_coord[1]) * tw / ws) * ws
        X = p * ws + ox
        Y = p * ws + oy
    X, Y = _f32(X), _f32(Y)
    if int(u.surface_type) == 1:
        # h_u / h_v are vertex-shader values, so f32 as proxy.wgsl:76-79 writes them (far from the origin their rounding moves
        # the sample point by ~1e-4 texel); the bilinear filter itself is float64
        hms = [F32(u.height_map_scale[k]) for k in range(3)]
        hx, hy = F32(u.map_half_wh[0]), F32(u.map_half_wh[1])
        xr = (F32(2.0) * hx + F32(1.0)) * tw * hms[0]
        yr = (F32(2.0) * hy + F32(1.0)) * tw * hms[1]
        hu = _f32(_f32(X + hx * tw) / xr)
        hv = _f32(_f32(Y + hy * tw) / yr)
        HU, HV = np.meshgrid(hu, hv, indexing="ij")
        M = _bilinear_repeat(np.asarray(height_map, np.float64), HU, HV) * np.float64(hms[2])
    else:
        M = np.zeros((nx + 1, ny + 1))
    Z = _f32(F32(u.height_offset) + _f32(M))
    return X, Y, Z, M


def triangles(u, grid_dim, height_map):
    """World vertices [T, 3, 3] (f32 values as float64), mapped heights [T, 3], in the order cell (i, j) -> triangles
    2 (i ny + j) + 0 = (i, j), (i+1, j), (i, j+1) and + 1 = (i+1, j), (i+1, j+1), (i, j+1)."""
    X, Y, Z, M = lattice(u, grid_dim, height_map)
    nx, ny = X.shape[0] - 1, Y.shape[0] - 1
    I, J = np.meshgrid(np.arange(nx), np.arange(ny), indexing="ij")
    I, J = I.ravel(), J.ravel()
    corners = [((I, J), (I + 1, J), (I, J + 1)), ((I + 1, J), (I + 1, J + 1), (I, J + 1))]
    P = np.empty((nx * ny, 2, 3, 3))
    Mh = np.empty((nx * ny, 2, 3))
    for k, tri in enumerate(corners):
        for v, (a, b) in enumerate(tri):
            P[:, k, v] = np.stack([X[a], Y[b], Z[a, b]], -1)
            Mh[:, k, v] = M[a, b]
    return P.reshape(-1, 3, 3), Mh.reshape(-1, 3)


def camera(u):
    """(R [3, 3], t [3], GP [4, 4]) float64 from the uniform block's f32 view / projection (column-major); GP =
    opengl_to_wgpu * projection (proxy.wgsl:84-91)."""
    V = np.asarray(u.view[:], np.float64).reshape(4, 4).T
    P = np.asarray(u.projection[:], np.float64).reshape(4, 4).T
    G = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 0.5, 0.5], [0, 0, 0, 1]], np.float64)
    assert P[0, 1] == P[0, 2] == P[1, 0] == P[1, 2] == 0.0 and P[3, 2] == -1.0 and P[3, 3] == 0.0, "perspective() form"
    return V[:3, :3], V[:3, 3], G @ P


def pixel_dirs(u, W, H, xs, ys):
    """Camera-space ray directions (ndc_x / P00, ndc_y / P11, -1) of pixel centres (xs, ys)."""
    p00, p11 = float(u.projection[0]), float(u.projection[5])
    nx = (np.asarray(xs, np.float64) + 0.5) / W * 2.0 - 1.0
    ny = 1.0 - (np.asarray(ys, np.float64) + 0.5) / H * 2.0
    return np.stack([nx / p00, ny / p11, -np.ones_like(nx)], -1)


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def _dot(a, b):
    return np.einsum("...k,...k->...", a, b)


def _bary(d, A, E1, E2):
    """Moeller-Trumbore from the camera-space origin: (b1, b2, s) of ray s d against triangle (A, A + E1, A + E2)."""
    pv = _cross(d, E2)
    det = _dot(E1, pv)
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = 1.0 / det
        tv = -A
        b1 = _dot(tv, pv) * inv
        qv = _cross(tv, E1)
        b2 = _dot(d, qv) * inv
        s = _dot(E2, qv) * inv
    return b1, b2, s


def _candidates(Cv, GP, W, H, window):
    """Per triangle the pixel box [x0, x1] x [y0, y1] (window coordinates) to test, or None for no pixel at all."""
    wx0, wy0, ww, wh = window
    q = np.einsum("rc,tvc->tvr", GP, np.concatenate([Cv, np.ones(Cv.shape[:2] + (1,))], -1))
    front = np.all(q[..., 3] > 0.0, axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        ndc = q[..., :3] / q[..., 3:4]
    drop = front & (np.all(ndc[..., 2] < 0.0, axis=1) | np.all(ndc[..., 2] > 1.0, axis=1))
    behind = np.all(q[..., 3] <= 0.0, axis=1)          # every point of the triangle has w <= 0
    keep = ~(drop | behind)
    px = (ndc[..., 0] + 1.0) * 0.5 * W - 0.5            # pixel-centre coordinates, one pixel of slack each side
    py = (1.0 - ndc[..., 1]) * 0.5 * H - 0.5
    x0 = np.where(front, np.floor(np.nan_to_num(px.min(1), nan=0.0)) - 1, wx0)
    x1 = np.where(front, np.ceil(np.nan_to_num(px.max(1), nan=0.0)) + 1, wx0 + ww - 1)
    y0 = np.where(front, np.floor(np.nan_to_num(py.min(1), nan=0.0)) - 1, wy0)
    y1 = np.where(front, np.ceil(np.nan_to_num(py.max(1), nan=0.0)) + 1, wy0 + wh - 1)
    x0 = np.clip(x0, wx0, wx0 + ww) - wx0
    x1 = np.clip(x1, wx0 - 1, wx0 + ww - 1) - wx0
    y0 = np.clip(y0, wy0, wy0 + wh) - wy0
    y1 = np.clip(y1, wy0 - 1, wy0 + wh - 1) - wy0
    keep &= (x1 >= x0) & (y1 >= y0)
    return keep, x0.astype(np.int64), x1.astype(np.int64), y0.astype(np.int64), y1.astype(np.int64)


def render(u, W, H, *, grid_dim=2048, height_map=None, mips=None, depth_in=None, rgba_in=None, window=None,
           eps_edge=1e-4, eps_depth=1e-6, eps_clip=1e-5, uv_ulps=8.0, max_pairs=4_000_000):
    """One draw over the pixel window (x0, y0, w, h) of a W x H target (default: all of it).

    Returns a dict of [h, w] arrays:
      depth  -- the depth buffer after the draw (depth_in combined by Less; depth_in defaults to 1.0)
      rgba   -- [h, w, 4] colour after the draw (rgba_in where nothing was written; default 0)
      frag   -- the nearest fragment's depth (nan where the draw has none), tri -- its triangle (NO_HIT), margin -- its minimum
                barycentric coordinate, written -- fragment passed the Less test
      amb    -- a pixel whose outcome a rounding could flip: some candidate not behind the nearest fragment lies within
                eps_edge of a triangle edge, within eps_depth of the near / far plane or of the incoming depth, or within
                eps_clip of the clip height
      col_tol -- per pixel, how far the colour of an f32 evaluation of the same fragment may move: the uv rounding
                (ulp(uv), times the texture's steepest texel step) and the LOD it moves (times the contrast between levels)
    and 'tris' / 'mapped' (the mesh) and 'cam_hit' ([h, w, 3] camera-space fragment position)."""
    x0w, y0w, ww, wh = window if window is not None else (0, 0, W, H)
    tris, mapped = triangles(u, grid_dim, height_map)
    R, t, GP = camera(u)
    Cv = np.einsum("rc,tvc->tvr", R, tris) + t                          # camera space, float64
    keep, bx0, bx1, by0, by1 = _candidates(Cv, GP, W, H, (x0w, y0w, ww, wh))
    idx = np.nonzero(keep)[0]
    area = (bx1[idx] - bx0[idx] + 1) * (by1[idx] - by0[idx] + 1)
    use_clip = int(u.use_clip) == 1
    clip_h = float(F32(u.clip_height))

    npx = ww * wh
    best = np.full(npx, np.inf)
    best_tri = np.full(npx, NO_HIT, np.int64)
    best_margin = np.full(npx, np.nan)
    best_s = np.full(npx, np.nan)
    amb = np.zeros(npx, bool)
    band_pix, band_dep = [], []          # candidates a rounding could flip, kept if nothing visible lies in front of them
    start = 0
    csum = np.cumsum(area)
    while start < idx.size:
        base = csum[start - 1] if start else 0
        stop = int(np.searchsorted(csum, base + max_pairs, side="right"))
        stop = max(stop, start + 1)
        ti = idx[start:stop]
        a = area[start:stop]
        rep = np.repeat(np.arange(ti.size), a)
        loc = np.arange(rep.size) - np.repeat(np.cumsum(a) - a, a)
        bw = (bx1[ti] - bx0[ti] + 1)[rep]
        lx = bx0[ti][rep] + loc % bw
        ly = by0[ti][rep] + loc // bw
        tri = ti[rep]
        d = pixel_dirs(u, W, H, lx + x0w, ly + y0w)
        A = Cv[tri, 0]
        b1, b2, s = _bary(d, A, Cv[tri, 1] - A, Cv[tri, 2] - A)
        margin = np.minimum(np.minimum(b1, b2), 1.0 - b1 - b2)
        q2 = GP[2, 0] * s * d[:, 0] + GP[2, 1] * s * d[:, 1] + GP[2, 2] * s * d[:, 2] + GP[2, 3]
        q3 = GP[3, 0] * s * d[:, 0] + GP[3, 1] * s * d[:, 1] + GP[3, 2] * s * d[:, 2] + GP[3, 3]
        with np.errstate(divide="ignore", invalid="ignore"):
            dep = q2 / q3
        mh = mapped[tri, 0] + b1 * (mapped[tri, 1] - mapped[tri, 0]) + b2 * (mapped[tri, 2] - mapped[tri, 0])
        front = np.isfinite(s) & (s > 0.0) & (q3 > 0.0)
        in_depth = (dep >= 0.0) & (dep <= 1.0)
        kept = ~(use_clip & (mh < clip_h)) if use_clip else np.ones(mh.shape, bool)
        ok = front & (margin >= 0.0) & in_depth & kept
        pix = ly * ww + lx
        # anything a rounding could flip
        near = front & (margin > -eps_edge)
        a_edge = near & (margin < eps_edge) & (dep > -eps_depth) & (dep < 1.0 + eps_depth) & ((not use_clip) | (mh > clip_h - eps_clip))
        a_plane = near & ((np.abs(dep) < eps_depth) | (np.abs(dep - 1.0) < eps_depth))
        a_clip = near & use_clip & (np.abs(mh - clip_h) < eps_clip) & (dep > -eps_depth) & (dep < 1.0 + eps_depth)
        a_any = a_edge | a_plane | a_clip
        band_pix.append(pix[a_any])
        band_dep.append(dep[a_any])
        if np.any(ok):
            p, dd, tt, mm, ss = pix[ok], dep[ok], tri[ok], margin[ok], s[ok]
            order = np.lexsort((dd, p))
            p, dd, tt, mm, ss = p[order], dd[order], tt[order], mm[order], ss[order]
            first = np.r_[True, p[1:] != p[:-1]]
            p, dd, tt, mm, ss = p[first], dd[first], tt[first], mm[first], ss[first]
            better = dd < best[p]
            p, dd, tt, mm, ss = p[better], dd[better], tt[better], mm[better], ss[better]
            best[p], best_tri[p], best_margin[p], best_s[p] = dd, tt, mm, ss
        start = stop

    if band_pix:
        bp, bd = np.concatenate(band_pix), np.concatenate(band_dep)
        front_most = bd <= best[bp] + eps_depth                           # not hidden behind the visible fragment
        amb[bp[front_most]] = True
    shape = (wh, ww)
    dep_in = np.ones(shape) if depth_in is None else np.asarray(depth_in, np.float64).reshape(shape)
    out_d = dep_in.copy().ravel()
    hit = best_tri != NO_HIT
    written = hit & (best < dep_in.ravel())                               # CompareFunction::Less
    amb |= hit & (np.abs(best - dep_in.ravel()) < eps_depth)
    out_d[written] = best[written]
    rgba = np.zeros(shape + (4,)) if rgba_in is None else np.asarray(rgba_in, np.float64).reshape(shape + (4,)).copy()
    rgba = rgba.reshape(-1, 4)
    ys, xs = np.divmod(np.arange(npx), ww)
    cam_hit = np.full((npx, 3), np.nan)
    col_tol = np.zeros(npx)
    dpx = pixel_dirs(u, W, H, xs + x0w, ys + y0w)
    cam_hit[hit] = best_s[hit, None] * dpx[hit]
    if np.any(written):
        if int(u.black_background) == 1:
            rgba[written] = (0.0, 0.0, 0.0, 1.0)
        else:
            rgba[written], col_tol[written] = _shade(u, W, H, tris, Cv, best_tri[written], xs[written] + x0w,
                                                     ys[written] + y0w, mips, uv_ulps)
    frag = np.where(hit, best, np.nan)
    return dict(depth=out_d.reshape(shape), rgba=rgba.reshape(shape + (4,)), frag=frag.reshape(shape),
                tri=best_tri.reshape(shape), margin=best_margin.reshape(shape), written=written.reshape(shape),
                amb=amb.reshape(shape), col_tol=col_tol.reshape(shape), tris=tris, mapped=mapped, cam_hit=cam_hit.reshape(shape + (3,)))


def _uv_on_plane(u, W, H, tris, Cv, tri, xs, ys):
    """tex_coords (proxy.wgsl:92) where the ray of pixel (xs, ys) meets the plane of triangle `tri`: the barycentric blend of
    the f32 vertex positions / tile_width / 4."""
    d = pixel_dirs(u, W, H, xs, ys)
    A = Cv[tri, 0]
    b1, b2, _ = _bary(d, A, Cv[tri, 1] - A, Cv[tri, 2] - A)
    P = tris[tri]
    xy = P[:, 0, :2] + b1[:, None] * (P[:, 1, :2] - P[:, 0, :2]) + b2[:, None] * (P[:, 2, :2] - P[:, 0, :2])
    return xy / float(F32(u.tile_width)) / 4.0


def _shade(u, W, H, tris, Cv, tri, xs, ys, mips, uv_ulps):
    """(rgba [n, 4], colour tolerance [n]).  The tolerance: a uv off by du = uv_ulps ulp_f32(|uv|) moves a bilinear sample by at
    most du * size * (steepest step between neighbouring texels of level 0); the rho of the two uv differences moves by up to
    2 sqrt(2) du size, so the LOD by that / (rho ln 2), and a LOD step blends towards a level at most `contrast` away."""
    uv = _uv_on_plane(u, W, H, tris, Cv, tri, xs, ys)
    uvx = _uv_on_plane(u, W, H, tris, Cv, tri, xs + 1, ys)
    uvy = _uv_on_plane(u, W, H, tris, Cv, tri, xs, ys + 1)
    n = len(mips)
    size = np.asarray(mips[0]).shape[0]
    rho = np.maximum(np.linalg.norm((uvx - uv) * size, axis=1), np.linalg.norm((uvy - uv) * size, axis=1))
    with np.errstate(divide="ignore", invalid="ignore"):
        lod = np.log2(rho)
    lod = np.clip(np.nan_to_num(lod, nan=0.0, neginf=0.0), 0.0, n - 1)
    l0 = np.floor(lod).astype(np.int64)
    l1 = np.minimum(l0 + 1, n - 1)
    fl = (lod - l0)[:, None]
    c0 = np.empty((tri.size, 3))
    c1 = np.empty((tri.size, 3))
    for lvl in range(n):
        img = np.asarray(mips[lvl], np.float64)[..., :3]
        m0, m1 = l0 == lvl, l1 == lvl
        if m0.any():
            c0[m0] = _bilinear_repeat(img, uv[m0, 0], uv[m0, 1])
        if m1.any():
            c1[m1] = _bilinear_repeat(img, uv[m1, 0], uv[m1, 1])
    out = np.ones((tri.size, 4))
    br = float(F32(u.brightness))
    out[:, :3] = (c0 * (1.0 - fl) + c1 * fl) * br
    m0 = np.asarray(mips[0], np.float64)[..., :3]
    step = max(np.abs(np.diff(m0, axis=0)).max(initial=0.0), np.abs(np.diff(m0, axis=1)).max(initial=0.0),
               np.abs(m0[0] - m0[-1]).max(), np.abs(m0[:, 0] - m0[:, -1]).max())
    contrast = max(np.abs(np.asarray(mips[k], np.float64)[..., :3]).max() for k in range(n))
    du = uv_ulps * np.spacing(np.abs(uv).max(1).astype(F32)).astype(np.float64)
    dlod = np.where(rho > 1.0, 2.0 * np.sqrt(2.0) * du * size / (np.maximum(rho, 1.0) * np.log(2.0)), 0.0)
    tol = (du * size * step + np.minimum(dlod, 1.0) * contrast) * br
    return out, tol


def f32_clip_depth(u, W, H, tris, tri, xs, ys):
    """What a rasteriser working in f32 makes of triangle `tri` at pixel (xs, ys): clip = (opengl_to_wgpu * projection * view)
    * (x, y, z, 1) per vertex in f32 (the WGSL expression is evaluated left to right, matrix products first), z / w per vertex
    in f32, then the screen-space (affine) interpolation of z / w in float64.  nan where a vertex has w <= 0."""
    V = _f32(u.view[:]).reshape(4, 4).T
    P = _f32(u.projection[:]).reshape(4, 4).T
    G = _f32([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 0.5, 0.5], [0, 0, 0, 1]])

    def mul(a, b):                                     # f32 matrix product, each dot product summed left to right
        out = np.zeros((4, 4), F32)
        for r in range(4):
            for c in range(4):
                acc = F32(a[r, 0] * b[0, c])
                for k in range(1, 4):
                    acc = F32(acc + F32(a[r, k] * b[k, c]))
                out[r, c] = acc
        return out

    M = mul(mul(G, P), V)
    p = _f32(tris[tri])                                 # [n, 3, 3]
    clip = [None] * 4
    for r in range(4):
        acc = M[r, 0] * p[..., 0]
        acc = _f32(acc + M[r, 1] * p[..., 1])
        acc = _f32(acc + M[r, 2] * p[..., 2])
        clip[r] = _f32(acc + M[r, 3])
    with np.errstate(divide="ignore", invalid="ignore"):
        ndc = [_f32(clip[r] / clip[3]).astype(np.float64) for r in range(3)]
    sx = (np.asarray(xs, np.float64) + 0.5) / W * 2.0 - 1.0
    sy = 1.0 - (np.asarray(ys, np.float64) + 0.5) / H * 2.0
    x, y, z = ndc
    den = (y[:, 1] - y[:, 2]) * (x[:, 0] - x[:, 2]) + (x[:, 2] - x[:, 1]) * (y[:, 0] - y[:, 2])
    with np.errstate(divide="ignore", invalid="ignore"):
        l0 = ((y[:, 1] - y[:, 2]) * (sx - x[:, 2]) + (x[:, 2] - x[:, 1]) * (sy - y[:, 2])) / den
        l1 = ((y[:, 2] - y[:, 0]) * (sx - x[:, 2]) + (x[:, 0] - x[:, 2]) * (sy - y[:, 2])) / den
    out = l0 * z[:, 0] + l1 * z[:, 1] + (1.0 - l0 - l1) * z[:, 2]
    return np.where(np.all(clip[3] > 0, axis=1), out, np.nan)


# ---- scenes shared by tests/test_proxy_raster_cpu.py (oracle) and tests/test_proxy_raster_gpu.py (k_proxy) ----------------
W0, H0 = 257, 161          # odd: the centre column / row has ndc 0, so axis-aligned views give rays with dx or dy = 0


def height_map(n=16, seed=0):
    return np.random.default_rng(seed).uniform(-1.0, 1.0, (n, n)).astype(F32)


def mip_chain(ts=64):
    """A checker (8-texel squares) plus uv ramps; each level the 2x2 box average of the previous one."""
    yy, xx = np.mgrid[0:ts, 0:ts]
    cur = np.zeros((ts, ts, 4), F32)
    cur[..., 0] = ((xx // 8 + yy // 8) % 2) * 0.8 + 0.1
    cur[..., 1] = xx / ts
    cur[..., 2] = yy / ts
    cur[..., 3] = 1.0
    out = [cur.copy()]
    while cur.shape[0] > 1:
        cur = cur.reshape(cur.shape[0] // 2, 2, cur.shape[1] // 2, 2, 4).mean((1, 3)).astype(F32)
        out.append(cur.copy())
    return out


def _map(**kw):
    d = dict(map_proxy=1, height_offset=-0.5, surface_type=1, map_half_wh=(10, 10), height_map_scale=(1.0, 1.0, 1.5))
    d.update(kw)
    return d


def _full(**kw):
    d = dict(map_proxy=0, height_offset=-0.6, surface_type=1, width_scale=4.0, map_half_wh=(10, 10),
             height_map_scale=(1.0, 1.0, 1.5))
    d.update(kw)
    return d


FAR_OPT = dict(eps_edge=1e-2, depth_tol=None, colour="ulp", max_amb=0.1)

# name: (camera kwargs, [draw uniforms], grid_dim, options).  Options: eps_edge (rounding band at edges, barycentric),
# depth_tol (present: derived from the f32 rasteriser emulation), colour ("ulp": within 1e-4 + the reference's per-pixel col_tol,
# which far from the origin covers the f32 rounding of uv ~ 1e4), max_amb (bound on the band fraction).
SCENES = {
    "oblique": (dict(pos=(3.0, -5.0, 6.0), tgt=(10.0, 12.0, -2.0)), [_map()], 24, {}),
    "outside_footprint": (dict(pos=(-60.0, 5.0, 3.0), tgt=(0.0, 0.0, -1.0)), [_map()], 24, {}),
    "outside_oblique": (dict(pos=(-70.0, -50.0, 4.0), tgt=(-20.0, 30.0, -1.0)), [_map()], 24, {}),
    "outside_corner_low": (dict(pos=(-55.0, -61.0, 1.5), tgt=(0.0, 0.0, -0.5)), [_map()], 24, {}),
    "axis_plus_x": (dict(pos=(-5.0, 0.3, 2.5), tgt=(30.0, 0.3, -1.0)), [_map()], 24, {}),
    "axis_minus_x": (dict(pos=(30.0, -1.7, 3.0), tgt=(-10.0, -1.7, -1.0)), [_map()], 24, {}),
    "axis_plus_y": (dict(pos=(2.3, -35.0, 2.0), tgt=(2.3, 10.0, -1.0)), [_map()], 24, {}),
    "axis_minus_y": (dict(pos=(1.0, 30.0, 3.0), tgt=(1.0, -10.0, -1.0)), [_map()], 24, {}),
    # x = 8 is a line of the map grid (tile_width 4): the centre column's rays lie in that plane
    "on_grid_line": (dict(pos=(8.0, -30.0, 3.0), tgt=(8.0, 20.0, -1.0)), [_map()], 24, {}),
    "straight_down": (dict(pos=(1.3, 2.1, 25.0), tgt=(1.3001, 2.1002, -1.0)), [_map()], 24, {}),
    "below_surface": (dict(pos=(2.0, 3.0, -4.0), tgt=(15.0, 8.0, 0.5)), [_map()], 24, {}),
    "grazing": (dict(pos=(-38.0, -3.0, 0.4), tgt=(20.0, 2.0, 0.0)), [_map()], 24, {}),
    "cell_diagonal": (dict(pos=(30.0, -30.0, 3.0), tgt=(-30.0, 30.0, -1.0)), [_map()], 24, {}),
    "near_cuts_hill": (dict(pos=(0.5, 0.5, 1.2), tgt=(6.0, 3.0, -1.5), z_near=2.5), [_map()], 24, {}),
    "far_cuts_grid": (dict(pos=(-30.0, -10.0, 2.0), tgt=(30.0, 15.0, -1.0), z_far=40.0), [_map()], 24, {}),
    "flat_two_draws": (dict(pos=(3.0, -9.0, 5.0), tgt=(8.0, 20.0, -2.0)),
                       [_full(surface_type=0), _map(surface_type=0, height_offset=-0.45)], 24, {}),
    "hills_two_draws": (dict(pos=(-50.0, -40.0, 6.0), tgt=(0.0, 0.0, -1.0)),
                        [_full(), _map(height_offset=-0.45, center_coord=(1, -1))], 24, {}),
    "clip_two_draws": (dict(pos=(3.0, -5.0, 6.0), tgt=(10.0, 12.0, -2.0)),
                       [_full(use_clip=1, clip_height=0.3), _map(use_clip=1, clip_height=0.3, height_offset=-0.45)], 24, {}),
    "black_background": (dict(pos=(3.0, -5.0, 6.0), tgt=(10.0, 12.0, -2.0)), [_map(black_background=1, brightness=0.5)], 24, {}),
    # far from the origin: non-dyadic tile widths; the f32 rounding band at edges is wide (ulp(1e5) ~ 0.008 world units)
    "far_1e3": (dict(pos=(1115.0, -996.0, 1.2), tgt=(1085.0, -989.0, -0.2)), [_map(tile_width=3.7, center_coord=(300, -270))],
                24, FAR_OPT),
    "far_1e4": (dict(pos=(9255.0, -11098.0, 1.2), tgt=(9225.0, -11090.0, -0.2)),
                [_map(tile_width=3.7, center_coord=(2500, -3000))], 24, FAR_OPT),
    "far_1e5": (dict(pos=(-85770.0, 102302.0, 2.0), tgt=(-85800.0, 102300.0, -1.0)),
                [_map(tile_width=3.3, center_coord=(-26000, 31000))], 24, FAR_OPT),
    "far_1e5_map_3_7": (dict(pos=(99903.0, 92502.0, 5.0), tgt=(99920.0, 92530.0, -1.0)),
                        [_map(tile_width=3.7, center_coord=(27000, 25000))], 24, FAR_OPT),
    "far_1e5_full_grid": (dict(pos=(99903.0, 92502.0, 5.0), tgt=(99920.0, 92530.0, -1.0)),
                          [_full(tile_width=3.7, width_scale=5.3, center_coord=(27000, 25000))], 24,
                          FAR_OPT),
}

# the reference's own scale, cropped: the 129 x 129 tile map at 3840 x 2160 (proxy.rs:219-251), one 256 x 192 window
BIG = ((3840, 2160), (1800, 1100, 256, 192),
       dict(pos=(-20.0, -30.0, 12.0), tgt=(40.0, 60.0, -2.0)), [_map(map_half_wh=(64, 64), height_map_scale=(1.0, 1.0, 2.0))])


def scene_camera(cam, W, H):
    from oracle import gswt_oracle as orc       # the Camera (camera.rs) only: view / projection in f32
    return orc.Camera(W, H, cam["pos"], cam["tgt"], [0, 0, 1], z_near=cam.get("z_near", 0.1), z_far=cam.get("z_far", 2400.0))


def scene_uniforms(cam, draws):
    from oracle import gswt_oracle as orc       # the 224-byte proxy.wgsl Uniforms block
    return [orc.proxy_uniforms(cam, **d) for d in draws]


def sky(W, H, seed=1):
    return np.random.default_rng(seed).uniform(0.0, 1.0, (H, W, 4)).astype(F32)


def reference(us, W, H, *, grid_dim, hm, mips, window=None, eps_edge=1e-4):
    """The draws in order into one target (depth cleared to 1, colour = sky): final depth, colour, the union of the
    draws' ambiguity masks, the result dict per draw, and the per-pixel colour tolerance of the fragment each pixel kept."""
    x0, y0, w, h = window if window is not None else (0, 0, W, H)
    depth = np.ones((h, w))
    rgba = sky(W, H)[y0:y0 + h, x0:x0 + w].astype(np.float64)
    amb = np.zeros((h, w), bool)
    col_tol = np.zeros((h, w))
    res = []
    for u in us:
        r = render(u, W, H, grid_dim=grid_dim, height_map=hm, mips=mips, depth_in=depth, rgba_in=rgba, window=window,
                   eps_edge=eps_edge)
        depth, rgba, amb = r["depth"], r["rgba"], amb | r["amb"]
        col_tol = np.where(r["written"], r["col_tol"], col_tol)
        res.append(r)
    return depth, rgba, amb, res, col_tol


def emulated_error(us, W, H, res, amb, window=None):
    """max |f32-rasteriser depth - f64 depth| over the pixels each draw wrote and no rounding band touches."""
    x0, y0 = (window or (0, 0))[:2]
    err = 0.0
    for u, r in zip(us, res):
        m = r["written"] & ~amb
        if not m.any():
            continue
        ys, xs = np.nonzero(m)
        e = f32_clip_depth(u, W, H, r["tris"], r["tri"][m], xs + x0, ys + y0)
        err = max(err, float(np.nanmax(np.abs(e - r["frag"][m]))))
    return err


def compare(got_depth, got_rgba, ref_depth, ref_rgba, amb, *, depth_tol, colour=True, col_tol=1e-4, max_amb=0.02,
            ulp_tol=None):
    """Assertions shared by the oracle and the kernel tests; returns the max depth error off the rounding bands.
    colour: True -- within col_tol; "ulp" -- within col_tol + ulp_tol (the reference's per-pixel col_tol)."""
    got_depth = np.asarray(got_depth, np.float64)
    cov_g, cov_r = got_depth < 1.0, ref_depth < 1.0
    bad = (cov_g != cov_r) & ~amb
    assert not bad.any(), f"coverage differs off the edges at {bad.sum()} pixels, e.g. (y, x) = {np.argwhere(bad)[:4].tolist()}"
    assert amb.mean() < max_amb, f"rounding bands cover {amb.mean():.3%} of the window: the scene does not test much"
    both = cov_g & cov_r & ~amb
    derr = float(np.abs(got_depth - ref_depth)[both].max()) if both.any() else 0.0
    assert derr <= depth_tol, f"depth error {derr:.3e} > {depth_tol:.1e}"
    if colour:
        tol = col_tol + (ulp_tol if colour == "ulp" else 0.0)
        err = np.abs(np.asarray(got_rgba, np.float64) - ref_rgba).max(-1)
        over = (err > tol) & ~amb
        assert not over.any(), (f"colour off at {over.sum()} pixels, worst {err[over].max():.3e} "
                                f"(tolerance there {np.broadcast_to(tol, err.shape)[over][err[over].argmax()]:.1e})")
    return derr
