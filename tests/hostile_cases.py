"""The hostile golden cases: tests/golden/make_golden.py's case_plane and case_hmap -- configuration, camera position, target and sort
event -- over special_splats.hostile_tileset in the place of synth.make_tileset (no tests here; tests/test_hostile_modes_cpu.py pins the
cases, tests/test_hostile_modes_gpu.py runs the frame modes over them).  About a tenth of every tile's rows are the record classes of
special_splats.CLASSES: floaters, needles and discs, exactly isotropic covariances, alpha bytes 0 / 1 / 254 / 255, saturated and NaN
colours, exact duplicates, cell-edge positions, extreme heights and NaN / +-Inf positions.

tests/ortho_ref.golden, tests/frame_modes.view and tests/mode_stack_ref know the two names; the cameras are the benign cases' own."""
from __future__ import annotations

import numpy as np

from oracle import gswt_oracle as orc
from tests import special_splats as S

# name -> (the golden case it restates, the tile set's seed).  500 LOD-0 rows per tile, as the hostile tests of
# tests/test_special_splats_gpu.py; the seeds are the ones under which tests/test_hostile_modes_cpu.py's populations hold.
CASES = {"case_plane_hostile": ("case_plane", 3), "case_hmap_hostile": ("case_hmap", 1)}
LOD0_COUNT = 500
N_LOD = 2
# Three rows in ten are hostile, so that a 125-row LOD-1 tile holds two or three non-finite positions (special_splats cycles NaN, +Inf
# and -Inf over a tile's own).  A duplicate group takes two or three rows, so the cycle over the classes always steps over the class behind
# "duplicate": in special_splats.CLASSES that is edge_xy, which all but two tiles then lack.  Here "duplicate" stands last with a second
# "floater_one" behind it to be stepped over, and "nonfinite_pos" stands in the cycle twice.
FRAC = 0.3
_REST = tuple(c for c in S.CLASSES if c != "duplicate")
CLASS_ORDER = _REST[:8] + ("nonfinite_pos",) + _REST[8:] + ("duplicate", "floater_one")
# The frames' splat scale: tests/ortho_ref.SPLAT_SCALE, unless tests/test_hostile_modes_cpu.py's margin test asks for a smaller one
SPLAT_SCALE = 24.0


def is_hostile(name) -> bool:
    return name in CASES


def benign(name) -> str:
    """The golden case whose cameras, light and tables a case shares: itself, or the case a hostile one restates."""
    return CASES[name][0] if name in CASES else name


def build(name) -> dict:
    """tests/depth_ref.golden_case of the restated case over the hostile tile set, with `labels` (special_splats.hostile_tileset's) and
    `tex_class` [records of pp.tex]: the index into special_splats.CLASSES of every texture record, -1 for a synthetic row."""
    from tests import depth_ref as DR
    base, seed = CASES[name]
    verts, labels = S.hostile_tileset(seed=seed, n_lod=N_LOD, lod0_count=LOD0_COUNT, frac=FRAC, classes=CLASS_ORDER)
    g = DR.golden_case(base, verts=verts)
    g["labels"] = labels
    g["tex_class"] = _tex_classes(verts, labels, g["pp"])
    return g


def _tex_classes(verts, labels, pp):
    """Scene::load orders a tile's rows by importance, so a replaced row is found again by its 32 loaded bytes (a row's bytes do not depend
    on its neighbours: each is loaded on its own here; preprocess moves z, bytes 8 .. 11, alone)."""
    out = np.full(pp.tex.shape[0], -1, np.int64)
    keep = np.r_[0:8, 12:32]
    for l, lod in enumerate(verts):
        for t, v in enumerate(lod):
            if not labels[l][t]:
                continue
            want = {bytes(orc.scene_load(v[r:r + 1])[0][keep]): S.CLASSES.index(c) for r, c in labels[l][t]}
            rows = orc.scene_load(v)
            found = 0
            for k, row in enumerate(rows):
                c = want.get(bytes(row[keep]))
                if c is not None:
                    out[int(pp.merge_offset[l, t]) + k] = c
                    found += 1
            assert found >= len(want), (l, t, found, len(want))
    return out


def instance_classes(g) -> np.ndarray:
    """The class index of every instance of the case's draws, in draw order (the order of the varyings); -1 synthetic."""
    return np.concatenate([g["tex_class"][np.asarray(d.gs_index, np.int64)] for d in g["draws"]])


# ---- what the modes read over the hostile plane case (tests/mode_stack_ref.inputs; tests/test_hostile_modes_cpu.py holds the conditions) ----
# The benign plane case's ramp, 4 .. 8, keeps too few of the rare alpha bytes; this one spans the frame's distances.
PLANE_FADE = (3.0, 12.0)
# Every cell the sort event draws is styled (25 cells; the draws use 7, 8, 9, 12, 13, 14, 17, 18, 19 and 24): four tints, one of them at
# full strength and one with a dim, four dims without a tint, and two hidden cells.
PLANE_CELLS = {13: (0, 255, 64, 160, 0), 8: (255, 64, 0, 160, 96), 17: (10, 20, 250, 200, 0), 9: (255, 0, 255, 255, 0), 18: (0, 0, 0, 0, 128),
               14: (0, 0, 0, 0, 64), 19: (0, 0, 0, 0, 200), 24: (0, 0, 0, 0, 254), 12: (0, 0, 0, 0, 255), 7: (0, 0, 0, 0, 255)}
PLANE_N_STYLES = 25
LIGHT_W, LIGHT_H = 32, 24


def plane_light():
    """A sun straight above the plane map whose depth range, z = 2 .. -2, ends inside the scene: the z_extreme rows at z = +-3 fall outside it on
    either side (ld < 0, ld > 1), the ones at +-0.6 inside."""
    from gswt_renderer_amd import ortho
    return ortho.top_down((4.0, 6.0), 6.5, 2.0, -2.0, LIGHT_W, LIGHT_H)


def plane_map(light):
    """tests/shadow_ref.plane_map's three kinds of 4 x 4 texel blocks (0.0, 1.0, the depth of the plane z = 0) with a NaN texel in every
    fifth column of every third row: a NaN texel is lit."""
    from tests import shadow_ref as SR
    Z = SR.plane_map(light)
    Z[::3, ::5] = np.nan
    return Z


def plane_clip_volumes():
    """One keep box over the whole map; a cut box whose faces are the edges x = 0, 4 and y = 4, 8 of one map cell, in coordinates exact in
    binary32 (u0 = 0.5 x - 1, u1 = 0.5 y - 3, u2 = 0.125 z), so that edge_xy rows lie on its boundary, which is inside; a cut half-space
    below z = -1.5, tilted, with z_extreme rows on both sides; and a cut ellipsoid."""
    from gswt_renderer_amd import clip as CL
    V = CL.ClipVolume
    return [V.box((4.0, 6.0, 0.0), (16.0, 16.0, 8.0), keep=True),
            V.box((2.0, 6.0, 0.0), (2.0, 2.0, 8.0)),
            V.half_space((4.0, 6.0, -1.5), (0.05, 0.02, 1.0)),
            V.ellipsoid((7.0, 3.0, 0.0), (1.5, 1.0, 2.0))]
