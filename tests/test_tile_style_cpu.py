"""gswt_set_tile_styles without a GPU: the symbol and its struct through header, library and binding; the Python table's cell
arithmetic against tile_offset's; the float32 reference's fixed points."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from gswt_renderer_amd import _lib as L
from gswt_renderer_amd import styles as ST
from tests import ortho_ref as OR
from tests import pick_ref as PR
from tests import tile_style_ref as TR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


def test_symbol_is_declared_exported_and_bound():
    src = open(os.path.join(ROOT, "include", "gswt_hip.h")).read()
    assert re.search(r"GSWT_API\s+int\s+gswt_set_tile_styles\s*\(\s*gswt_ctx\s*\*ctx,\s*const\s+gswt_tile_style\s*\*styles,\s*size_t\s+n_styles\s*\)\s*;", src)
    lib = C.CDLL(os.path.join(ROOT, "gswt_renderer_amd", "lib", "libgswt_hip.so"))
    assert hasattr(lib, "gswt_set_tile_styles")
    restype, argtypes = L.SYMBOLS["gswt_set_tile_styles"]
    assert restype is C.c_int and argtypes == [C.c_void_p, C.c_void_p, C.c_size_t]
    assert L.load().gswt_set_tile_styles.argtypes == argtypes


def test_struct_layout():
    assert C.sizeof(L.TileStyle) == 8 == ST.ENTRY_BYTES
    assert (L.TileStyle.tint.offset, L.TileStyle.tint_strength.offset, L.TileStyle.dim.offset, L.TileStyle._pad.offset) == (0, 3, 4, 5)
    s = ST.TileStyle(tint=(1, 2, 3), strength=4, dim=5)
    c = L.TileStyle.from_buffer_copy(s.pack())
    assert (tuple(c.tint), c.tint_strength, c.dim, tuple(c._pad)) == ((1, 2, 3), 4, 5, (0, 0, 0))
    assert ST.HIDE.pack() == bytes([0, 0, 0, 0, 255, 0, 0, 0]) and ST.NEUTRAL.pack() == bytes(8) and ST.NEUTRAL.neutral and not ST.HIDE.neutral
    assert TR.pack(TR.entries({1: TR.entry((1, 2, 3), 4, 5)}, 2)) == bytes(8) + s.pack()
    for bad in (dict(tint=(0, 0)), dict(strength=256), dict(dim=-1), dict(tint=(0, 0, 300)), dict(dim=1.5)):
        with pytest.raises(ValueError):
            ST.TileStyle(**bad)


def _tile_offset_cell(map_id, center, half, surface_type):
    """A3 of the vertex stage (gswt.wgsl:52-65) in cells: the quotient and remainder by the map's height, shifted to the window's centre."""
    map_wh_y = 2 * half[1] + (1 if surface_type != 2 else 0)
    return (map_id // map_wh_y - half[0] + center[0], map_id % map_wh_y - half[1] + center[1])


@pytest.mark.parametrize("surface_type", [0, 1, 2])
@pytest.mark.parametrize("center,half", [((0, 0), (2, 2)), ((-7, 12), (3, 1)), ((100, -3), (1, 4))])
def test_table_and_cell_of_round_trip(center, half, surface_type):
    w, h = ST.map_width(half, surface_type), ST.map_height(half, surface_type)
    assert (w, h) == ((2 * half[0], 2 * half[1]) if surface_type == 2 else (2 * half[0] + 1, 2 * half[1] + 1))
    seen = set()
    for i in range(w * h):
        cell = ST.cell_of(i, center, half, surface_type)
        assert cell == _tile_offset_cell(i, center, half, surface_type)
        assert ST.index_of(cell, center, half, surface_type) == i
        seen.add(cell)
    assert len(seen) == w * h
    # cells outside the window have no index and no entry
    outside = (center[0] - half[0] - 1, center[1]), (center[0], center[1] - half[1] - 1), (center[0] + half[0] + 1, center[1]), (center[0], center[1] + half[1] + 1)
    assert all(ST.index_of(c, center, half, surface_type) is None for c in outside)
    first, last = ST.cell_of(0, center, half, surface_type), ST.cell_of(w * h - 1, center, half, surface_type)
    mid = ST.cell_of(h + 1, center, half, surface_type)
    tint = ST.TileStyle(tint=(9, 8, 7), strength=200, dim=3)
    t = ST.TileStyles({first: ST.HIDE, mid: tint, outside[0]: ST.HIDE, outside[3]: tint})
    raw = t.table(center, half, surface_type)
    assert len(raw) == 8 * (h + 2) and raw[:8] == ST.HIDE.pack() and raw[8 * (h + 1):] == tint.pack() and raw[8:8 * (h + 1)] == bytes(8 * h)
    t[last] = ST.TileStyle(dim=1)
    assert len(t.table(center, half, surface_type)) == 8 * w * h
    # a window that moved one cell: the same world cells, other indices
    moved = (center[0] + 1, center[1])
    raw2 = t.table(moved, half, surface_type)
    assert ST.index_of(mid, moved, half, surface_type) == ST.index_of(mid, center, half, surface_type) - h
    assert raw2[8 * (1):8 * 2] == tint.pack()
    assert ST.TileStyles({outside[0]: ST.HIDE, mid: ST.NEUTRAL}).table(center, half, surface_type) == b""


def test_cells_agree_with_the_golden_draws():
    """The map_index of every static draw of the golden plane case is the index of the world cell its tile offset names."""
    g = OR.golden("case_plane")
    su = OR.scene_of(g)
    center, half = tuple(su.center_coord), tuple(su.map_half_wh)
    n = 0
    for d in g["draws"]:
        if d.tile.single_draw == 1:
            continue
        cell = (int(round(d.tile.offset[0] / su.tile_width)), int(round(d.tile.offset[1] / su.tile_width)))
        assert ST.cell_of(d.tile.map_index, center, half, su.surface_type) == cell
        assert ST.index_of(cell, center, half, su.surface_type) == d.tile.map_index
        n += 1
    assert n >= 4
    mi, _ = PR.identities(g["draws"])
    assert mi.shape[0] == 510 and int(mi.max()) < TR.MAIN_N == ST.map_width(half, 0) * ST.map_height(half, 0)
    merged = [d for d in g["draws"] if d.tile.single_draw == 1]
    assert len(merged) == 1 and sorted(set(np.asarray(merged[0].map_id).tolist())) == [9, 14]


def test_reference_fixed_points():
    rng = np.random.default_rng(3)
    n = 400
    rgba = (rng.integers(0, 256, (n, 4)).astype(F32) / F32(255.0)).astype(F32)
    vis = rng.integers(0, 2, n)
    # neutral entries: the identity, bit for bit
    v, out = TR.apply(rgba, vis, np.zeros((n, 5), np.uint8))
    assert np.array_equal(v, vis == 1) and np.array_equal(out.view(np.uint32), rgba.view(np.uint32))
    # a tint colour without strength is neutral too
    sty = np.zeros((n, 5), np.uint8)
    sty[:, :3] = rng.integers(0, 256, (n, 3))
    assert np.array_equal(TR.apply(rgba, vis, sty)[1].view(np.uint32), rgba.view(np.uint32))
    # strength 255: exactly the tint colour, whatever the splat's; alpha untouched
    sty[:, 3] = 255
    v, out = TR.apply(rgba, vis, sty)
    assert np.array_equal(np.rint(out[:, :3].astype(np.float64) * 255.0), sty[:, :3].astype(np.float64))
    assert np.array_equal(out[:, :3], (sty[:, :3].astype(F32) / F32(255.0)).astype(F32)) and np.array_equal(out[:, 3], rgba[:, 3]) and np.array_equal(v, vis == 1)
    # dim 128 is exactly 127 / 255 of the alpha; dim 255 hides; dim never touches the colour
    sty[:] = 0
    sty[:, 4] = 128
    v, out = TR.apply(rgba, vis, sty)
    assert np.array_equal(out[:, 3], (rgba[:, 3] * (F32(127) / F32(255))).astype(F32)) and np.array_equal(out[:, :3], rgba[:, :3])
    sty[::2, 4] = 255
    v, _ = TR.apply(rgba, vis, sty)
    assert not v[::2].any() and np.array_equal(v[1::2], vis[1::2] == 1)
    # lookups past the table are neutral
    e = TR.entries(TR.MAIN, TR.MAIN_N)
    got = TR.lookup(e, [8, 14, 24, 25, 4000])
    assert [tuple(r) for r in got] == [TR.HIDE, TR.MAIN[14], TR.MAIN[24], TR.NEUTRAL, TR.NEUTRAL]
    assert len(TR.pack(e)) == 8 * TR.MAIN_N
