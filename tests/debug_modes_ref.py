"""The debug draw modes (scene block draw_mode 1 .. 4: TileID, TileLOD, LOD, View) and the point-cloud radius under the frame modes of the
strict vertex stage: the expected projected records of a golden case at one point of tests/mode_stack_ref.py's lattice.  numpy only, no
tests here: tests/test_debug_modes_cpu.py pins this module and its inputs without a GPU, tests/test_debug_modes_gpu.py compares the device
with it.

Nothing is restated here.  The oracle projects every draw_mode and the point cloud under oracle.frame_mode(ortho, aa_s, fade); what the
header (include/gswt_hip.h) promises on top of that is composed from the references the tree already has:

  base           MS.base_records on a copy of the view's scene block carrying draw_mode and point_cloud_radius: `visible` the pair
                 rectangles', geometry, alpha with the LOD-transition share, the filter's comp and the fade's fs, and the debug colours.
  styles         hidden cells are not visible; alpha = TR.dimmed_alpha(base alpha); in a debug draw mode the tint does nothing.
  shadow, fog    in a debug draw mode: nothing.
  clip volumes   CR.expected's hidden set is removed; on the HeightMap and Sphere surfaces a splat inside its margins' mask (`open`) may
                 go either way.  The plain surface has no mask.

draw_mode != 0: colour is the base record's three floats untouched, and the comparison is "exact" on all three surfaces whatever modes
are on.  draw_mode == 0 with a point cloud: colour follows MS.stack's own rule on the point-cloud base records (the point cloud replaces
the covariance and moves no centre: what the world gives -- distance, shadow -- stays the case's own)."""
from __future__ import annotations

import numpy as np

from oracle import gswt_oracle as orc
from tests import atmosphere_ref as AR
from tests import clip_ref as CR
from tests import frame_modes as FM
from tests import mode_stack_ref as MS
from tests import ortho_ref as OR
from tests import pick_ref as PR
from tests import tile_style_ref as TR

F32 = np.float32
DRAW_MODES = (1, 2, 3, 4)
STAGES = ("tint", "shadow", "fog")
VIEWS = [(case, cam) for case, cams in MS.CAMERAS.items() for cam in cams]


def scene(su, draw_mode=0, point_cloud_radius=0.0) -> orc.Scene160:
    """A copy of the scene block `su` carrying the draw mode and the point-cloud radius."""
    s = orc.Scene160.from_buffer_copy(bytes(su))
    s.draw_mode, s.point_cloud_radius = int(draw_mode), float(point_cloud_radius)
    return s


def expected(pt: MS.Point, draw_mode, point_cloud_radius=0.0, clip_volumes=None) -> dict:
    """The expected records of the point in MS.stack's form (MS.check_records reads it), with `open` [n]: the splats the clip margins
    leave undecided (none without volumes, none on the plain surface)."""
    base = MS.base_records(pt.case, pt.cam, pt.aa, pt.fade, int(draw_mode), float(point_cloud_radius))
    n = base.shape[0]
    if draw_mode == 0:
        out = dict(MS.stack(pt, base))
        if out["how"] != "exact" and pt.case != "case_plane":
            # the unprojected distance and shadow exist for the splats the unmoded frame shows
            out["masked"] = out["masked"] | ((base["visible"] == 1) & (MS.base_records(pt.case, pt.cam, False, False)["visible"] != 1))
    else:
        ids = PR.identities(OR.golden(pt.case)["draws"])[0]
        sty = TR.lookup(MS.inputs(pt.case).entries, ids) if pt.sty else np.zeros((n, 5), np.uint8)
        visible = (base["visible"] == 1) & ~TR.classes(sty)[0]
        out = dict(point=pt, base=base, visible=visible, alpha=TR.dimmed_alpha(base["rgba"][:, 3], sty), sty=sty, how="exact",
                   rgb=np.ascontiguousarray(base["rgba"][:, :3]).copy(), masked=np.zeros(n, bool), bound=np.zeros(n))
    out["open"] = np.zeros(n, bool)
    if clip_volumes is not None:
        hid, msk, _ = CR.expected(pt.case, pt.cam, clip_volumes)
        out["open"] = msk & out["visible"]
        out["visible"] = out["visible"] & ~hid
    return out


def check_records(got, n_visible, st):
    """MS.check_records with the clip margins' mask: a splat inside it takes the device's side; at most AR.MAX_MASKED of the visible."""
    st = dict(st)
    open_ = st["open"]
    if not (st["visible"] | open_).any():                       # nothing to compare field by field: the frame shows no splat
        assert not (got["visible"] == 1).any() and n_visible == 0, st["point"].id
        return f"{st['point'].id}: no splat visible"
    if open_.any():
        assert st["point"].case != "case_plane"
        assert open_.sum() <= AR.MAX_MASKED * max(1, int((st["visible"] | open_).sum())), int(open_.sum())
        st["visible"] = np.where(open_, got["visible"] == 1, st["visible"])
    return MS.check_records(got, n_visible, st)


def counterfactual(pt: MS.Point, draw_mode, stages=STAGES) -> dict:
    """What the draw_mode == 0 colour rules would make of the debug colours: the point's tint, shadow and fog (those named in `stages`)
    through MS.colour_f32 / MS.codes_f64 over the debug base records.  `rgb` [n, 3] float64, what the record would report, and `differs`
    [n]: the splats on which that cannot be the expected colour -- in the exact chain a different float, in the float64 one a code
    farther from 255 x the expected colour than the byte's half code and the point's own bound (MS.stack); masked splats never differ."""
    st = expected(pt, draw_mode)
    exp = st["rgb"].astype(np.float64)
    n = exp.shape[0]
    wd = MS.world(pt.case, pt.cam)
    sty = st["sty"] if (pt.sty and "tint" in stages) else np.zeros((n, 5), np.uint8)
    shd = pt.shd and "shadow" in stages
    fog = pt.fog and "fog" in stages
    sh = wd["sh"] if shd else np.zeros(n, wd["sh"].dtype)
    if not fog and (wd["exact"] or not shd):
        rgb = MS.colour_f32(st["rgb"], sty, sh, wd["p"])
        return dict(rgb=rgb.astype(np.float64), differs=(rgb != st["rgb"]).any(1))
    atm_p = AR.params(MS.atmosphere_of(pt))
    dist = np.where(np.isfinite(wd["dist"]), wd["dist"], 0.0)
    codes = MS.codes_f64(st["rgb"], sty, sh if shd else None, wd["p"], dist, atm_p if fog else None)
    ms = MS.stack(pt)
    bound = ms["bound"] if ms["how"] == "bound" else np.full(n, 0.5 + AR.FOG_MARGIN)
    differs = (np.abs(codes - 255.0 * exp) > bound[:, None]).any(1) & ~ms["masked"]
    return dict(rgb=np.rint(codes) / 255.0, differs=differs)


def off_grid(rgb):
    """Per splat, whether a colour channel is no multiple of 1 / 255 in binary32 ((float)byte / 255.0f): a quantisation would move it."""
    rgb = np.asarray(rgb, F32)
    b = np.rint(np.clip(rgb, F32(0.0), F32(1.0)) * F32(255.0)).astype(F32)
    return ((b / F32(255.0)).astype(F32) != rgb).any(1)
