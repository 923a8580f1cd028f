"""A cube map whose texels hold their own unit lookup direction, and the direction each skybox pixel must look up.

skybox.wgsl vs_main (:26-53) passes the cube's `position` through as tex_coords, re-ordered to (x, -z, y) and with y negated
again when the map is a cube map (equirectangular == 0); the rasterised position at a pixel is a positive multiple of the
pixel's world view direction (the translation is removed, :41-47).  fs_main (:55-59) samples the cube at that vector, level 0,
Linear, ClampToEdge (skybox.rs:420-426).

Faces are written from the WebGPU / Vulkan major-axis table (face, sc, tc, ma), s = (sc / |ma| + 1) / 2, t = (tc / |ma| + 1) / 2,
texel (row i, column j) centred at s = (j + 0.5) / n, t = (i + 0.5) / n:
    +X: (-z, -y, x)   -X: (z, -y, x)   +Y: (x, z, y)   -Y: (x, -z, y)   +Z: (x, -y, z)   -Z: (-x, -y, z)
so the texel of face f at (sc, tc) = (2s - 1, 2t - 1) looks along the directions below (inverting the table by hand)."""
import numpy as np

FACE_DIRS = (
    lambda sc, tc: (np.ones_like(sc), -tc, -sc),          # +X
    lambda sc, tc: (-np.ones_like(sc), -tc, sc),          # -X
    lambda sc, tc: (sc, np.ones_like(sc), tc),            # +Y
    lambda sc, tc: (sc, -np.ones_like(sc), -tc),          # -Y
    lambda sc, tc: (sc, -tc, np.ones_like(sc)),           # +Z
    lambda sc, tc: (-sc, -tc, -np.ones_like(sc)),         # -Z
)


def direction_cube(n):
    """[6, n, n, 4] f32: rgb = the unit direction of the texel centre, a = 1."""
    c = (np.arange(n) + 0.5) / n * 2.0 - 1.0
    tc, sc = np.meshgrid(c, c, indexing="ij")              # row i -> t, column j -> s
    faces = np.ones((6, n, n, 4), np.float32)
    for f, fn in enumerate(FACE_DIRS):
        d = np.stack(fn(sc, tc), -1)
        faces[f, ..., :3] = d / np.linalg.norm(d, axis=-1, keepdims=True)
    return faces


def lookup_dirs(cam, W, H, equirectangular):
    """[H, W, 3] float64 unit lookup vectors: the pixel's world view direction R^T (ndc_x / P00, ndc_y / P11, -1),
    re-ordered (x, -z, y), y negated for a cube map."""
    V = np.asarray(cam.view, np.float64).reshape(4, 4).T
    p00, p11 = float(cam.projection[0]), float(cam.projection[5])
    nx = (np.arange(W) + 0.5) / W * 2.0 - 1.0
    ny = 1.0 - (np.arange(H) + 0.5) / H * 2.0
    NY, NX = np.meshgrid(ny, nx, indexing="ij")
    v = np.stack([NX / p00, NY / p11, -np.ones_like(NX)], -1)
    d = v @ V[:3, :3]                                       # R^T v for every pixel
    t = np.stack([d[..., 0], -d[..., 2], d[..., 1]], -1)
    if not equirectangular:
        t[..., 1] = -t[..., 1]
    return t / np.linalg.norm(t, axis=-1, keepdims=True)


def tolerance(dirs, n):
    """Per pixel: how far a bilinear sample of the direction cube may lie from the exact unit direction.  Inside a face the
    bilinear error of f = normalize(sc, tc, 1) is <= (h^2 / 8)(|f_ss| + |f_tt|) + (h^2 / 4)|f_st| with h = 2 / n, and every
    second derivative of f has norm <= 1 on [-1, 1]^2, so <= h^2 / 2; within half a texel of a face edge ClampToEdge holds
    the edge texel, up to half a texel's angle (h / 2) away.  Plus f32 rounding."""
    h = 2.0 / n
    a = np.abs(dirs)
    ma = a.max(-1)
    srt = np.sort(a, -1)
    # the two minor face coordinates, in [0, 1]; near 1 = near a face edge
    near_edge = (srt[..., 1] / ma > 1.0 - h / 2.0 - 1e-9)
    return np.where(near_edge, 0.5 * h * 1.05, 0.5 * h * h) + 1e-5
