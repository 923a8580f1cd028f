"""CPU restatement of the reference's skybox bake (equirectangular HDR panorama -> cube map), in float64 from the f32 inputs.

Skybox::configure (skybox.rs:341-455) creates a CUBEMAP_RESO^2 x 6 Rgba32Float cube (skybox.rs:35) and, for an .exr panorama,
bake_skybox (skybox.rs:490-668) draws the unit cube (skybox.rs:36ff, 36 vertices, no culling, no depth attachment) once per
face with vs_bake / fs_bake (skybox.wgsl:62-96):

1. rasterisation: camera at the origin, perspective(90 deg, 1, 0.1, 10) and Mat4::look_at_rh(0, target_i, up_i) from the table
   at skybox.rs:584-617.  The interpolated `tex_coords` is the cube position along the ray through the pixel centre, so the
   baked direction is that ray, normalized (skybox.wgsl:76);
2. SampleSphericalMap (skybox.wgsl:89-96) with the truncated constants 0.1591 and 0.3183;
3. textureSampleLevel(t_equi, s_equi, uv, 0): Rgba32Float, Linear, Repeat in u and v (skybox.rs:544-555, texture.rs:47-51),
   one level, row 0 = v 0; WebGPU bilinear x = u * w - 0.5;
4. Reinhard c / (c + 1), then pow(c, 1.0/2.2) with an f32 exponent, alpha 1 (skybox.wgsl:77-84).
"""
import numpy as np

U_SCALE = 0.1591            # skybox.wgsl:94 -- not 1 / (2 pi)
V_SCALE = 0.3183            # skybox.wgsl:95 -- not 1 / pi
GAMMA = float(np.float32(1.0 / 2.2))      # the f32 constant of pow(color, vec3(1.0/2.2)), skybox.wgsl:81
FOVY_DEG, ASPECT, Z_NEAR, Z_FAR = 90.0, 1.0, 0.1, 10.0     # skybox.rs:582

# skybox.rs:584-617: (target, up) of look_at_rh(origin, target, up), faces +X -X +Y -Y +Z -Z.  +Z looks down -Z (as written).
BAKE_VIEWS = (((1.0, 0.0, 0.0), (0.0, 1.0, 0.0)),
              ((-1.0, 0.0, 0.0), (0.0, 1.0, 0.0)),
              ((0.0, 1.0, 0.0), (0.0, 0.0, 1.0)),
              ((0.0, -1.0, 0.0), (0.0, 0.0, -1.0)),
              ((0.0, 0.0, -1.0), (0.0, 1.0, 0.0)),
              ((0.0, 0.0, 1.0), (0.0, 1.0, 0.0)))


def _normalize(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def look_at_rh(eye, center, up):
    """cgmath Matrix4::look_at_rh as a row-major matrix acting on column vectors: rows s, u, -f (plus translation)."""
    eye = np.asarray(eye, np.float64)
    f = _normalize(np.asarray(center, np.float64) - eye)
    s = _normalize(np.cross(f, up))
    u = np.cross(s, f)
    m = np.eye(4)
    m[0, :3], m[1, :3], m[2, :3] = s, u, -f
    m[0, 3], m[1, 3], m[2, 3] = -s @ eye, -u @ eye, f @ eye
    return m


def perspective(fovy_deg, aspect, near, far):
    """cgmath perspective(Deg(fovy), aspect, near, far) (OpenGL clip space), row-major."""
    f = 1.0 / np.tan(np.radians(fovy_deg) / 2.0)
    return np.array([[f / aspect, 0, 0, 0], [0, f, 0, 0],
                     [0, 0, (far + near) / (near - far), 2 * far * near / (near - far)], [0, 0, -1, 0]], np.float64)


def bake_view(face):
    target, up = BAKE_VIEWS[face]
    return look_at_rh((0.0, 0.0, 0.0), target, up)


def bake_projection():
    return perspective(FOVY_DEG, ASPECT, Z_NEAR, Z_FAR)


def texel_ndc(y, x, n):
    """WebGPU pixel centre (x + 0.5, y + 0.5) of an n x n target in NDC (y up, framebuffer row 0 = top)."""
    x = np.asarray(x, np.float64)
    y = np.asarray(y, np.float64)
    return (x + 0.5) / n * 2.0 - 1.0, 1.0 - (y + 0.5) / n * 2.0


def texel_dirs(face, y, x, n):
    """Unit direction baked into texel (face, y, x): the view ray s * ndc_x / P00 + u * ndc_y / P11 + f."""
    v, p = bake_view(face), bake_projection()
    s, u, f = v[0, :3], v[1, :3], -v[2, :3]
    nx, ny = texel_ndc(y, x, n)
    d = (nx / p[0, 0])[..., None] * s + (ny / p[1, 1])[..., None] * u + f
    return _normalize(d)


def sample_spherical_map(d):
    """skybox.wgsl:89-96"""
    d = np.asarray(d, np.float64)
    u = np.arctan2(d[..., 2], d[..., 0]) * U_SCALE + 0.5
    v = np.arcsin(np.clip(d[..., 1], -1.0, 1.0)) * V_SCALE + 0.5
    return u, v


def bilinear_taps(coord, size):
    """WebGPU linear filter along one axis with Repeat: (first texel, second texel, weight of the second)."""
    x = np.asarray(coord, np.float64) * size - 0.5
    x0 = np.floor(x)
    a = np.mod(x0, size).astype(np.int64)
    return a, (a + 1) % size, x - x0


def sample_equi(equi, u, v):
    """textureSampleLevel(t_equi, s_equi, uv, 0) -> rgb, float64.  equi [h, w, 4]."""
    h, w = equi.shape[:2]
    xa, xb, tx = bilinear_taps(u, w)
    ya, yb, ty = bilinear_taps(v, h)
    e = np.asarray(equi)
    tx, ty = tx[..., None], ty[..., None]
    c = lambda yy, xx: e[yy, xx, :3].astype(np.float64)      # noqa: E731
    return (c(ya, xa) * (1 - tx) + c(ya, xb) * tx) * (1 - ty) + (c(yb, xa) * (1 - tx) + c(yb, xb) * tx) * ty


def tone_map(c):
    """skybox.wgsl:79-81: Reinhard, then pow(c, 1/2.2)."""
    c = c / (c + 1.0)
    return np.power(c, GAMMA)


def bake_texels(equi, face, y, x, n):
    """The baked RGBA (float64) of the texels (face, y, x) of an n x n cube; face / y / x broadcast."""
    face, y, x = np.broadcast_arrays(np.asarray(face), np.asarray(y), np.asarray(x))
    out = np.ones(face.shape + (4,), np.float64)
    for f in range(6):
        m = face == f
        if m.any():
            u, v = sample_spherical_map(texel_dirs(f, y[m], x[m], n))
            out[m, :3] = tone_map(sample_equi(equi, u, v))
    return out


def bake(equi, n):
    """All six faces, [6, n, n, 4] float64 (+X -X +Y -Y +Z -Z)."""
    yy, xx = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    return np.stack([bake_texels(equi, np.full_like(yy, f), yy, xx, n) for f in range(6)])
