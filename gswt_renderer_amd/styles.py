"""gswt_set_tile_styles' table (include/gswt_hip.h): hide, dim and tint map cells per splat.

``TileStyle(tint=(r, g, b), strength=0, dim=0)`` is one cell's entry (8 bytes, all zero: neutral); ``HIDE`` hides the cell.
``TileStyles`` maps WORLD cells ``(cx, cy)`` to styles and packs the table the library takes, which is indexed by map cell -- the
``map_index`` the pick image reports: ``table(center_coord, map_half_wh, surface_type)``.  Map indices move with the map window at a
build event; ``GSWTPipeline.set_tile_styles`` re-packs the table after each one, so that a styled world cell stays styled.
``cell_of(map_index, ...)`` goes from a pick record back to the world cell."""
from __future__ import annotations

import struct
from dataclasses import dataclass

ENTRY_BYTES = 8
SURFACE_SPHERE = 2
_FMT = "<5B3x"     # tint[3], tint_strength, dim, _pad[3]


@dataclass(frozen=True)
class TileStyle:
    tint: tuple = (0, 0, 0)      # R, G, B of the tint colour, 0..255
    strength: int = 0            # 0: no tint ... 255: the tint colour replaces the splat's
    dim: int = 0                 # 0: opacity unchanged ... 254; 255: the cell is hidden

    def __post_init__(self):
        vals = tuple(self.tint) + (self.strength, self.dim)
        if len(self.tint) != 3 or any(int(v) != v or not 0 <= v <= 255 for v in vals):
            raise ValueError("TileStyle: tint is (r, g, b), and every field an integer in 0..255")

    @property
    def neutral(self) -> bool:
        return self.strength == 0 and self.dim == 0

    def pack(self) -> bytes:
        """The 8-byte gswt_tile_style entry."""
        return struct.pack(_FMT, int(self.tint[0]), int(self.tint[1]), int(self.tint[2]), int(self.strength), int(self.dim))

    def __bytes__(self) -> bytes:
        return self.pack()


NEUTRAL = TileStyle()
HIDE = TileStyle(dim=255)
assert len(NEUTRAL.pack()) == ENTRY_BYTES and NEUTRAL.pack() == bytes(ENTRY_BYTES)


def map_height(map_half_wh, surface_type: int) -> int:
    """Cells per map column: 2 half_h + 1, and 2 half_h on the Sphere surface (tile_offset, A3 of the vertex stage)."""
    return 2 * int(map_half_wh[1]) + (0 if int(surface_type) == SURFACE_SPHERE else 1)


def map_width(map_half_wh, surface_type: int) -> int:
    return 2 * int(map_half_wh[0]) + (0 if int(surface_type) == SURFACE_SPHERE else 1)


def index_of(cell, center_coord, map_half_wh, surface_type: int = 0):
    """The map index of world cell (cx, cy) in the window around center_coord, or None when the cell is outside it."""
    ix = int(cell[0]) - int(center_coord[0]) + int(map_half_wh[0])
    iy = int(cell[1]) - int(center_coord[1]) + int(map_half_wh[1])
    if not (0 <= ix < map_width(map_half_wh, surface_type) and 0 <= iy < map_height(map_half_wh, surface_type)):
        return None
    return ix * map_height(map_half_wh, surface_type) + iy


def cell_of(map_index: int, center_coord, map_half_wh, surface_type: int = 0):
    """The world cell (cx, cy) of a map index -- tile_offset's arithmetic: from a pick record to the cell to style."""
    q, r = divmod(int(map_index), map_height(map_half_wh, surface_type))
    return (q - int(map_half_wh[0]) + int(center_coord[0]), r - int(map_half_wh[1]) + int(center_coord[1]))


class TileStyles(dict):
    """World cell (cx, cy) -> TileStyle.  A plain dict with the packing of the library's table."""

    def table(self, center_coord, map_half_wh, surface_type: int = 0) -> bytes:
        """The table for the map window around center_coord: entries up to the last styled cell inside the window (cells past the
        table read as neutral); a styled cell outside the window has no entry.  Empty when nothing inside is styled."""
        entries = {}
        for cell, st in self.items():
            i = index_of(cell, center_coord, map_half_wh, surface_type)
            if i is not None and not st.neutral:
                entries[i] = st
        if not entries:
            return b""
        buf = bytearray(ENTRY_BYTES * (max(entries) + 1))
        for i, st in entries.items():
            buf[ENTRY_BYTES * i:ENTRY_BYTES * (i + 1)] = st.pack()
        return bytes(buf)
