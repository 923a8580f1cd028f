"""gswt_set_clip_volumes' volumes (include/gswt_hip.h): cut splats and proxy ground by boxes, ellipsoids and half-spaces.

A volume is an affine map from world coordinates into its unit frame and a shape there: the box ``max|u| <= 1``, the ellipsoid
``u.u <= 1`` or the half-space ``u2 <= 0``.  A cut volume (the default) hides what is inside it, a keep volume (``keep=True``)
hides what is outside every keep volume; ``ground=True`` lets the proxy passes apply the volume to the ground too.  The
constructors build the map in float64 and round it once:

    ClipVolume.box(center, half_extents, rotation=None)         rotation: 3 x 3, its columns the box's axes in the world
    ClipVolume.ellipsoid(center, radii, rotation=None)
    ClipVolume.half_space(point, normal)                        inside: the side the normal points away from

``GSWTRenderer.set_clip_volumes(volumes)`` / ``render(..., clip_volumes=[...])`` hand up to MAX_VOLUMES of them to the library,
which validates the records again (GSWT_ERR_BAD_ARG names the volume and the field); an empty list switches the mode off.
"""
from __future__ import annotations

import struct

import numpy as np

MAX_VOLUMES = 8
BOX, ELLIPSOID, HALFSPACE = 0, 1, 2
KEEP, GROUND = 1, 2
VOLUME_BYTES = 64
_FMT = "<12f2I2I"         # world_to_unit[12] (rows 0..2, row-major 3 x 4), shape, flags, reserved[2]


class ClipVolume:
    """world_to_unit: 12 values, rows 0..2 of the affine map, row-major; shape: BOX, ELLIPSOID or HALFSPACE; flags: KEEP | GROUND."""

    def __init__(self, world_to_unit, shape: int, flags: int = 0):
        m = np.asarray(world_to_unit, dtype=np.float64).reshape(-1)
        if m.shape[0] != 12:
            raise ValueError("ClipVolume: world_to_unit is 12 values, rows 0..2 of a 3 x 4 affine map")
        if shape not in (BOX, ELLIPSOID, HALFSPACE):
            raise ValueError(f"ClipVolume: unknown shape {shape}")
        if flags & ~(KEEP | GROUND):
            raise ValueError(f"ClipVolume: unknown flag bits in {flags:#x}")
        self.world_to_unit = m.astype(np.float32)
        if not np.all(np.isfinite(self.world_to_unit)):
            raise ValueError("ClipVolume: world_to_unit is not finite")
        self.shape, self.flags = int(shape), int(flags)

    @property
    def keep(self) -> bool:
        return bool(self.flags & KEEP)

    @property
    def ground(self) -> bool:
        return bool(self.flags & GROUND)

    @staticmethod
    def _flags(keep: bool, ground: bool) -> int:
        return (KEEP if keep else 0) | (GROUND if ground else 0)

    @staticmethod
    def _scaled_frame(center, scale, rotation, what: str) -> np.ndarray:
        """Rows of u = diag(1 / scale) R^T (x - center): R's columns are the volume's axes in the world."""
        c = np.asarray(center, dtype=np.float64).reshape(-1)
        s = np.asarray(scale, dtype=np.float64).reshape(-1)
        if c.shape[0] != 3 or s.shape[0] != 3:
            raise ValueError(f"ClipVolume.{what}: center and {'half_extents' if what == 'box' else 'radii'} are three values each")
        if not np.all(s > 0.0):
            raise ValueError(f"ClipVolume.{what}: every extent must be > 0")
        R = np.eye(3) if rotation is None else np.asarray(rotation, dtype=np.float64).reshape(3, 3)
        A = R.T / s[:, None]
        m = np.zeros((3, 4), dtype=np.float64)
        m[:, :3] = A
        for r in range(3):           # plain sums, left to right: the result does not depend on a BLAS
            m[r, 3] = -((A[r, 0] * c[0] + A[r, 1] * c[1]) + A[r, 2] * c[2])
        return m

    @classmethod
    def box(cls, center, half_extents, rotation=None, *, keep: bool = False, ground: bool = False) -> "ClipVolume":
        return cls(cls._scaled_frame(center, half_extents, rotation, "box"), BOX, cls._flags(keep, ground))

    @classmethod
    def ellipsoid(cls, center, radii, rotation=None, *, keep: bool = False, ground: bool = False) -> "ClipVolume":
        return cls(cls._scaled_frame(center, radii, rotation, "ellipsoid"), ELLIPSOID, cls._flags(keep, ground))

    @classmethod
    def half_space(cls, point, normal, *, keep: bool = False, ground: bool = False) -> "ClipVolume":
        """Inside is the side the normal points away from: n . (x - point) <= 0, n normalised.  Rows 0 and 1 are zero (not read)."""
        p = np.asarray(point, dtype=np.float64).reshape(-1)
        n = np.asarray(normal, dtype=np.float64).reshape(-1)
        if p.shape[0] != 3 or n.shape[0] != 3:
            raise ValueError("ClipVolume.half_space: point and normal are three values each")
        ln = float(np.sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]))
        if not (ln > 0.0 and np.isfinite(ln)):
            raise ValueError("ClipVolume.half_space: the normal must be finite and not zero")
        n = n / ln
        m = np.zeros((3, 4), dtype=np.float64)
        m[2, :3] = n
        m[2, 3] = -((n[0] * p[0] + n[1] * p[1]) + n[2] * p[2])
        return cls(m, HALFSPACE, cls._flags(keep, ground))

    def pack(self) -> bytes:
        """The 64-byte gswt_clip_volume record, fields in declaration order, little-endian."""
        return struct.pack(_FMT, *[float(x) for x in self.world_to_unit], self.shape, self.flags, 0, 0)

    def __bytes__(self) -> bytes:
        return self.pack()


def pack(volumes) -> bytes:
    """The gswt_clip_volume array of `volumes` (ClipVolume objects, at most MAX_VOLUMES), 64 bytes each; b"" for none."""
    vols = list(volumes)
    if len(vols) > MAX_VOLUMES:
        raise ValueError(f"clip.pack: {len(vols)} volumes, more than MAX_VOLUMES = {MAX_VOLUMES}")
    for v in vols:
        if not isinstance(v, ClipVolume):
            raise TypeError("clip.pack: every entry is a ClipVolume")
    return b"".join(v.pack() for v in vols)


assert struct.calcsize(_FMT) == VOLUME_BYTES
