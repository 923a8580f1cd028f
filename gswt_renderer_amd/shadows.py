"""gswt_set_shadow_map's map (include/gswt_hip.h): sun shadows on the splats and on the proxy ground.

A shadow map is the depth image of an orthographic frame along the light's direction (``render(cam.uniforms(), ..., projection=1,
depth=True)`` over ``proxy_render(..., projection=1)``'s ground), or the host's own occluders in the same convention, together
with the matrix that takes a world point into that image.  ``from_ortho_camera(cam, depth, ...)`` makes one from the
ortho.OrthoCamera that rendered the image; ``ShadowMap(world_to_light, depth, ...)`` takes any affine matrix.  ``OFF`` switches
shadows off.  ``GSWTRenderer.set_shadow_map(m)`` / ``render(..., shadow=m)`` hand it to the library, which copies the image inside
the call and validates the block again (GSWT_ERR_BAD_ARG names the field).
"""
from __future__ import annotations

import math
import struct

import numpy as np

BLOCK_BYTES = 96
_FMT = "<16f2f3f3I"       # world_to_light[16], bias, strength, shade_color[3], _pad[3]
MAX_SIZE = 4096


class ShadowMap:
    """world_to_light: 16 values, column-major [4 c + r], affine (bottom row exactly 0, 0, 0, 1); rows 0 and 1 give light NDC x, y
    (+y up, -1..1 over the image), row 2 the depth in the image's convention (0 near .. 1 far).
    depth: the image, [height, width] float32 with row 0 at the top -- a numpy array (copied by the library inside the call), or a
    CUDA / HIP tensor (anything with ``is_cuda``, ``data_ptr()`` and ``shape``: contiguous float32, copied device to device on the
    context's stream).
    bias >= 0 in depth units; strength in (0, 1]; shade_color: what a fully shadowed colour goes toward, each in [0, 1].
    ``ShadowMap()`` without an image is OFF."""

    def __init__(self, world_to_light=None, depth=None, bias: float = 0.0, strength: float = 1.0, shade_color=(0.0, 0.0, 0.0)):
        if depth is None:
            if world_to_light is not None:
                raise ValueError("ShadowMap: world_to_light without a depth image")
            self.world_to_light = self.depth = None
            self.width = self.height = 0
            self.on_device = False
            self.bias, self.strength, self.shade_color = 0.0, 1.0, (0.0, 0.0, 0.0)
            return
        m = np.asarray(world_to_light, dtype=np.float64).reshape(-1)
        if m.shape[0] != 16:
            raise ValueError("ShadowMap: world_to_light is 16 values, column-major")
        m32 = m.astype(np.float32)
        if not np.all(np.isfinite(m32)):
            raise ValueError("ShadowMap: world_to_light is not finite")
        if not (m32[3] == 0.0 and m32[7] == 0.0 and m32[11] == 0.0 and m32[15] == 1.0):
            raise ValueError("ShadowMap: world_to_light must be affine, bottom row (0, 0, 0, 1)")
        self.world_to_light = m32
        self.on_device = bool(getattr(depth, "is_cuda", False))
        if self.on_device:
            if "float32" not in str(depth.dtype) or not depth.is_contiguous():
                raise ValueError("ShadowMap: a device depth image is a contiguous float32 tensor")
            shape = tuple(depth.shape)
            self.depth = depth
        else:
            a = np.asarray(depth)
            if a.dtype != np.float32:
                raise ValueError("ShadowMap: the depth image is float32")
            shape = a.shape
            self.depth = np.ascontiguousarray(a)
        if len(shape) != 2:
            raise ValueError("ShadowMap: the depth image is [height, width]")
        self.height, self.width = int(shape[0]), int(shape[1])
        if not (1 <= self.width <= MAX_SIZE and 1 <= self.height <= MAX_SIZE):
            raise ValueError(f"ShadowMap: width and height are 1..{MAX_SIZE}")
        self.bias, self.strength = float(bias), float(strength)
        col = tuple(float(x) for x in shade_color)
        if len(col) != 3:
            raise ValueError("ShadowMap: shade_color is (r, g, b)")
        self.shade_color = col
        if not (math.isfinite(self.bias) and self.bias >= 0.0):
            raise ValueError("ShadowMap: bias must be finite and >= 0")
        if not (0.0 < self.strength <= 1.0):
            raise ValueError("ShadowMap: strength must be in (0, 1]")
        if not all(0.0 <= x <= 1.0 for x in col):
            raise ValueError("ShadowMap: every shade_color component must be in [0, 1]")

    @property
    def is_off(self) -> bool:
        return self.depth is None

    def pack(self) -> bytes:
        """The 96-byte gswt_shadow_params block, fields in declaration order, binary32 little-endian."""
        m = [0.0] * 16 if self.is_off else [float(x) for x in self.world_to_light]
        return struct.pack(_FMT, *m, self.bias, self.strength, *self.shade_color, 0, 0, 0)

    def __bytes__(self) -> bytes:
        return self.pack()

    def depth_ptr(self) -> int:
        """The address the library copies the image from (host or device, see on_device)."""
        return int(self.depth.data_ptr()) if self.on_device else int(self.depth.ctypes.data)


OFF = ShadowMap()
assert len(OFF.pack()) == BLOCK_BYTES


def world_to_light(cam) -> np.ndarray:
    """M = opengl_to_wgpu * projection * view of an ortho.OrthoCamera, column-major float32[16]: evaluated in float64 from the
    camera's binary32 matrices (the ones the frame that rendered the map was given) and rounded once.  opengl_to_wgpu takes clip
    z to (z + w) / 2: the depth the frame writes."""
    P = np.asarray(cam.projection, dtype=np.float64).reshape(4, 4).T       # [r, c]
    V = np.asarray(cam.view, dtype=np.float64).reshape(4, 4).T
    G = np.eye(4, dtype=np.float64)
    G[2, 2], G[2, 3] = 0.5, 0.5
    PV = np.zeros((4, 4), dtype=np.float64)
    for r in range(4):               # plain sums, left to right: the result does not depend on a BLAS
        for c in range(4):
            PV[r, c] = ((P[r, 0] * V[0, c] + P[r, 1] * V[1, c]) + P[r, 2] * V[2, c]) + P[r, 3] * V[3, c]
    M = np.zeros((4, 4), dtype=np.float64)
    for r in range(4):
        for c in range(4):
            M[r, c] = ((G[r, 0] * PV[0, c] + G[r, 1] * PV[1, c]) + G[r, 2] * PV[2, c]) + G[r, 3] * PV[3, c]
    return np.ascontiguousarray(M.T.reshape(-1)).astype(np.float32)


def from_ortho_camera(cam, depth, bias: float = 0.0, strength: float = 1.0, shade_color=(0.0, 0.0, 0.0)) -> ShadowMap:
    """The shadow map of the orthographic frame `cam` rendered: depth is that frame's depth image, [cam.height, cam.width]."""
    shape = tuple(depth.shape)
    if shape != (cam.height, cam.width):
        raise ValueError(f"from_ortho_camera: the depth image is {shape}, the camera's frame [{cam.height}, {cam.width}]")
    return ShadowMap(world_to_light(cam), depth, bias, strength, shade_color)
