"""gswt_set_atmosphere's block (include/gswt_hip.h): the per-splat far fade and distance fog, and the fogged proxy ground.

``Atmosphere(fade=(start, end), fog=(density, start, max, (r, g, b)))``; either part may be ``None`` (off).  ``OFF`` switches the
atmosphere off.  ``GSWTRenderer.set_atmosphere(a)`` / ``render(..., atmosphere=a)`` hand the packed block to the library, which
validates it (GSWT_ERR_BAD_ARG names the field)."""
from __future__ import annotations

import struct
from dataclasses import dataclass

BLOCK_BYTES = 32
_FMT = "<8f"       # fade_start, fade_end, fog_density, fog_start, fog_max, fog_color[3]


@dataclass(frozen=True)
class Atmosphere:
    fade: tuple | None = None          # (fade_start, fade_end) in world units from the eye; None: no fade
    fog: tuple | None = None           # (density per world unit, start distance, cap on the fog amount, (r, g, b)); None: no fog

    def pack(self) -> bytes:
        """The 32-byte gswt_atmosphere block, fields in declaration order, binary32 little-endian."""
        fs, fe = (0.0, 0.0) if self.fade is None else (float(self.fade[0]), float(self.fade[1]))
        if self.fog is None:
            dens, start, mx, col = 0.0, 0.0, 0.0, (0.0, 0.0, 0.0)
        else:
            dens, start, mx = float(self.fog[0]), float(self.fog[1]), float(self.fog[2])
            col = tuple(float(x) for x in self.fog[3])
            if len(col) != 3:
                raise ValueError("fog colour is (r, g, b)")
        return struct.pack(_FMT, fs, fe, dens, start, mx, *col)

    def __bytes__(self) -> bytes:
        return self.pack()


OFF = Atmosphere()
assert len(OFF.pack()) == BLOCK_BYTES
