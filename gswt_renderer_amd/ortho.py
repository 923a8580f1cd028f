"""Orthographic cameras for GSWT_OPT_PROJECTION = 1 (include/gswt_hip.h): top-down maps, minimaps, sun-direction depth maps and
height fields of the splat terrain.

An orthographic frame is rendered with ``GSWTRenderer.render(cam.uniforms(), scene, W, H, projection=1, ...)``.  The uniform block
is the perspective one's 176 bytes with another meaning of three fields: `projection` is an affine OpenGL-convention `ortho`
matrix, `focal` is pixels per world unit (|0.5 P[0][0] W|, |0.5 P[1][1] H|), `htan_fov` is zero (ignored) and `cam_pos` is the
reference point of the LOD transition only.  NDC depth is LINEAR in the distance along the view direction,
depth = (d - near) / (far - near), so under a `top_down` camera the depth and pick images are height fields
(`height_from_depth`).

The matrices are evaluated in float64 and rounded to float32 once per element.  The ground under an orthographic frame is
the proxy pass's orthographic form: ``GSWTRenderer.proxy_render(cam.proxy_uniforms(...), W, H, rgba, depth, clear, projection=1)``
(gswt_proxy_render_ortho) writes the colour and depth images the frame then takes as bg_rgba / bg_depth, so a height field
holds the terrain where no splat covers it and a sun-direction depth map contains the ground (``shadows.from_ortho_camera``
turns such a frame's depth image into the shadow map of gswt_set_shadow_map).  The skybox has no orthographic form.
"""
from __future__ import annotations

import math

import numpy as np

from . import _lib as L

F32 = np.float32


def _look_at(eye, target, up) -> np.ndarray:
    """Right-handed look-at (the camera looks down its -z), column-major [4 c + r], float64.  Plain Python float arithmetic, sums
    left to right, so that the result does not depend on a BLAS."""
    ex, ey, ez = (float(v) for v in eye)
    tx, ty, tz = (float(v) for v in target)
    ux, uy, uz = (float(v) for v in up)
    fx, fy, fz = tx - ex, ty - ey, tz - ez
    n = math.sqrt(fx * fx + fy * fy + fz * fz)
    fx, fy, fz = fx / n, fy / n, fz / n
    sx, sy, sz = fy * uz - fz * uy, fz * ux - fx * uz, fx * uy - fy * ux          # s = f x up
    n = math.sqrt(sx * sx + sy * sy + sz * sz)
    sx, sy, sz = sx / n, sy / n, sz / n
    vx, vy, vz = sy * fz - sz * fy, sz * fx - sx * fz, sx * fy - sy * fx          # u = s x f
    m = np.zeros(16, dtype=np.float64)
    m[0], m[1], m[2] = sx, vx, -fx
    m[4], m[5], m[6] = sy, vy, -fy
    m[8], m[9], m[10] = sz, vz, -fz
    m[12] = -(sx * ex + sy * ey + sz * ez)
    m[13] = -(vx * ex + vy * ey + vz * ez)
    m[14] = fx * ex + fy * ey + fz * ez
    m[15] = 1.0
    return m


def _ortho(half_width: float, half_height: float, near: float, far: float) -> np.ndarray:
    """OpenGL `ortho(-hw, hw, -hh, hh, near, far)`, column-major, float64: clip z in [-1, 1], w = 1."""
    m = np.zeros(16, dtype=np.float64)
    m[0] = 1.0 / half_width
    m[5] = 1.0 / half_height
    m[10] = -2.0 / (far - near)
    m[14] = -(far + near) / (far - near)
    m[15] = 1.0
    return m


class OrthoCamera:
    """An orthographic view of width x height pixels: `eye` looking at `target`, the image spanning +-half_height world units
    vertically (and +-half_height * width / height horizontally) around the view axis, depth 0 at distance `near` and 1 at `far`
    along it.  lod_pos: the point LOD transitions are measured from (default: eye) -- for a map that shares the main view's draw
    set, the main view's eye."""

    def __init__(self, width: int, height: int, eye, target, up, half_height: float, near: float, far: float, lod_pos=None):
        self.width, self.height = int(width), int(height)
        self.eye = np.asarray(eye, dtype=np.float64)
        self.target = np.asarray(target, dtype=np.float64)
        self.up = np.asarray(up, dtype=np.float64)
        self.half_height = float(half_height)
        self.half_width = float(half_height) * self.width / self.height
        self.near, self.far = float(near), float(far)
        self.lod_pos = np.asarray(self.eye if lod_pos is None else lod_pos, dtype=np.float64)
        if not (self.half_height > 0.0 and self.far > self.near):
            raise ValueError("OrthoCamera: half_height must be > 0 and far > near")
        self.view = _look_at(self.eye, self.target, self.up).astype(F32)
        self.projection = _ortho(self.half_width, self.half_height, self.near, self.far).astype(F32)
        self.z_top = self.z_bottom = None          # set by top_down()

    def focal(self):
        """Pixels per world unit, the formula of CameraUniforms::from_camera (camera.rs:169-188) in binary32."""
        fx = (F32(0.5) * self.projection[0]) * F32(self.width)
        fy = (F32(0.5) * self.projection[5]) * F32(self.height)
        return abs(float(fx)), abs(float(fy))

    def uniforms(self) -> L.CameraUniforms:
        """The 176-byte camera block of an orthographic frame."""
        cu = L.CameraUniforms()
        cu.projection[:] = [float(x) for x in self.projection]
        cu.view[:] = [float(x) for x in self.view]
        cu.focal[:] = list(self.focal())
        cu.viewport[:] = [float(self.width), float(self.height)]
        cu.htan_fov[:] = [0.0, 0.0, 0.0, 0.0]
        p = self.lod_pos.astype(F32)
        cu.cam_pos[:] = [float(p[0]), float(p[1]), float(p[2]), 0.0]
        return cu

    def proxy_uniforms(self, **fields) -> L.ProxyUniforms:
        """The 224-byte proxy block of gswt_proxy_render_ortho for this camera: its view and projection, cam_pos = lod_pos (the
        reference point the fog distance is measured from) and the caller's remaining fields of gswt_proxy_uniforms by name --
        scalars, and map_half_wh / center_coord / height_map_scale (3 or 4 values) as sequences.  Defaults: tile_width, width_scale,
        brightness and height_map_scale 1, everything else 0."""
        u = L.ProxyUniforms()
        u.tile_width = u.width_scale = u.brightness = 1.0
        u.height_map_scale[:] = [1.0, 1.0, 1.0, 0.0]
        for name, value in fields.items():
            if name in ("view", "projection", "cam_pos", "_pad0") or not hasattr(u, name):
                raise TypeError(f"proxy_uniforms: {name!r} is not a field the caller sets")
            if name in ("map_half_wh", "center_coord", "height_map_scale"):
                vals = list(value)
                getattr(u, name)[:len(vals)] = [float(v) for v in vals] if name == "height_map_scale" else [int(v) for v in vals]
            else:
                setattr(u, name, value)
        u.view[:] = [float(x) for x in self.view]
        u.projection[:] = [float(x) for x in self.projection]
        p = self.lod_pos.astype(F32)
        u.cam_pos[:] = [float(p[0]), float(p[1]), float(p[2]), 0.0]
        return u

    def view_proj(self) -> np.ndarray:
        """projection * view, column-major float32[16], each element the left-to-right binary32 sum of its four products."""
        a, b = self.projection, self.view
        out = np.zeros(16, dtype=F32)
        for c in range(4):
            for r in range(4):
                acc = F32(a[r] * b[4 * c])
                for k in range(1, 4):
                    acc = F32(acc + F32(a[4 * k + r] * b[4 * c + k]))
                out[4 * c + r] = acc
        return out


def top_down(center_xy, half_extent: float, z_top: float, z_bottom: float, width: int, height: int, lod_pos=None) -> OrthoCamera:
    """A camera looking straight down -z over (cx, cy), world +y up the image and +x to the right, +-half_extent world units
    vertically.  The eye sits at z_top with near = 0 and far = z_top - z_bottom, so that world height z_top maps to depth 0 and
    z_bottom to depth 1 (splats above z_top or below z_bottom are not drawn)."""
    cx, cy = float(center_xy[0]), float(center_xy[1])
    z_top, z_bottom = float(z_top), float(z_bottom)
    if not z_top > z_bottom:
        raise ValueError("top_down: z_top must be above z_bottom")
    cam = OrthoCamera(width, height, (cx, cy, z_top), (cx, cy, z_top - 1.0), (0.0, 1.0, 0.0), half_extent, 0.0, z_top - z_bottom,
                      lod_pos=lod_pos)
    cam.z_top, cam.z_bottom = z_top, z_bottom
    return cam


def height_from_depth(cam: OrthoCamera, depth):
    """World z of an NDC depth under a `top_down` camera, z_top - d (z_top - z_bottom), in float64: turns the depth image or the
    `depth` field of the pick image into a height field (a pixel no splat covers holds the background depth, 1.0 -> z_bottom)."""
    if cam.z_top is None:
        raise ValueError("height_from_depth needs a camera made by top_down()")
    d = np.asarray(depth, dtype=np.float64)
    return cam.z_top - d * (cam.z_top - cam.z_bottom)
