"""tests/debug_modes_ref.py and its inputs, without a GPU: what tests/test_debug_modes_gpu.py compares the device with can tell a device
that honours the header's promises about the debug draw modes and the point-cloud radius from one that does not.

The visible set of every view is that of draw_mode 0; the draw_mode guards of the tint, the shade and the fog can be observed (applied to
the debug colours, each of the three alone would change a visible splat's colour); the debug colours are mostly no multiples of 1 / 255
(a quantisation would show); and the point cloud's known answers under the orthographic cameras, from the oracle alone."""
import numpy as np
import pytest

from oracle import gswt_oracle as orc
from tests import antialias_ref as AAR
from tests import clip_ref as CR
from tests import debug_modes_ref as DM
from tests import frame_modes as FM
from tests import mode_stack_ref as MS
from tests import ortho_ref as OR
from tests import tile_style_ref as TR

W, Hh = OR.W, OR.H
VIEW_IDS = [f"{case[5:]}-{cam}" for case, cam in DM.VIEWS]
RADII = (1e-4, 0.002, 0.02)


def _vis(rec):
    return rec["visible"] == 1


@pytest.mark.parametrize("case,cam", DM.VIEWS, ids=VIEW_IDS)
def test_the_visible_set_is_that_of_draw_mode_0(case, cam):
    v0 = MS.base_records(case, cam, False, False)["visible"]
    assert _vis(MS.base_records(case, cam, False, False)).sum() >= 100
    for dm in DM.DRAW_MODES:
        b = MS.base_records(case, cam, False, False, dm)
        assert np.array_equal(b["visible"], v0), dm
        for fld in MS.GEOMETRY:                              # ... and a debug draw mode moves nothing
            assert FM.bits_equal(np.ascontiguousarray(b[fld]), np.ascontiguousarray(MS.base_records(case, cam, False, False)[fld])), (dm, fld)
        assert FM.bits_equal(b["rgba"][:, 3].copy(), MS.base_records(case, cam, False, False)["rgba"][:, 3].copy()), dm


@pytest.mark.parametrize("dm", [1, 4])
@pytest.mark.parametrize("case,cam", DM.VIEWS, ids=VIEW_IDS)
def test_the_guards_can_be_observed(case, cam, dm):
    """At the corner (all modes on), the draw_mode == 0 rule of each colour stage alone, applied to the debug colours, gives at least one
    visible splat another colour than the expected one: a device without that stage's draw_mode guard fails the GPU comparison."""
    pt = MS.corner(case, cam)
    st = DM.expected(pt, dm)
    counts = {}
    for stage in DM.STAGES:
        cf = DM.counterfactual(pt, dm, (stage,))
        counts[stage] = int((cf["differs"] & st["visible"]).sum())
    both = DM.counterfactual(pt, dm)
    counts["all"] = int((both["differs"] & st["visible"]).sum())
    print(f"{pt.id} draw_mode {dm}: of {int(st['visible'].sum())} visible splats the colour would change on " + ", ".join(f"{k} {v}" for k, v in counts.items()))
    assert min(counts.values()) > 0, counts


@pytest.mark.parametrize("case,cam", DM.VIEWS, ids=VIEW_IDS)
def test_debug_colours_lie_off_the_byte_grid(case, cam):
    for dm, radius in [(m, 0.0) for m in DM.DRAW_MODES] + [(3, 0.02)]:
        b = MS.base_records(case, cam, False, False, dm, radius)
        vis = _vis(b)
        if not vis.any():                                   # (the point cloud under the plane's oblique camera: below)
            assert (case, cam, radius) == ("case_plane", "oblique", 0.02)
            continue
        off = DM.off_grid(b["rgba"][:, :3])[vis]
        print(f"{case} {cam} draw_mode {dm} radius {radius}: {int(off.sum())} of {int(vis.sum())} visible debug colours off the 1 / 255 grid ({off.mean():.2f})")
        assert off.sum() > 0
    assert not DM.off_grid(MS.base_records(case, cam, False, False)["rgba"][:, :3])[_vis(MS.base_records(case, cam, False, False))].any()


def test_expected_composes_the_promises():
    """Debug colours are the oracle's whatever is on; hidden cells go, dimmed ones keep their colour; clip volumes remove their hidden set."""
    for case, cam in DM.VIEWS:
        pt = MS.corner(case, cam)
        for dm in DM.DRAW_MODES:
            st = DM.expected(pt, dm)
            base = MS.base_records(case, cam, True, True, dm)
            assert st["how"] == "exact" and FM.bits_equal(st["rgb"], np.ascontiguousarray(base["rgba"][:, :3]))
            hidden, _, tinted, _ = TR.classes(st["sty"])
            assert (hidden & _vis(base)).sum() > 0 and not (st["visible"] & hidden).any() and (st["visible"] & tinted).sum() > 0
            assert np.array_equal(st["visible"], _vis(base) & ~hidden) and not st["open"].any()
            dim = st["visible"] & (st["sty"][:, 4] > 0) & (base["rgba"][:, 3] > 0)
            assert dim.sum() > 0 and (st["alpha"][dim] < base["rgba"][dim, 3]).all()
            assert FM.bits_equal(st["alpha"][~dim & st["visible"]].copy(), base["rgba"][~dim & st["visible"], 3].copy())
    for case, cam in (("case_plane", "persp"), ("case_sphere", "top")):
        vols = CR.volume_sets(case)["eight"]
        hid = CR.expected(case, cam, vols)[0]
        for pt in (MS.Point(case, cam), MS.corner(case, cam)):
            full, cut = DM.expected(pt, 1), DM.expected(pt, 1, clip_volumes=vols)
            assert np.array_equal(cut["visible"], full["visible"] & ~hid) and 0 < cut["visible"].sum() < full["visible"].sum()
            assert (case != "case_plane" or not cut["open"].any()) and cut["open"].sum() <= 0.02 * full["visible"].sum()


def test_a_point_cloud_at_draw_mode_0_follows_the_stack():
    for case, cam in DM.VIEWS:
        for pt in (MS.Point(case, cam), MS.Point(case, cam, aa=True), MS.corner(case, cam)):
            st = DM.expected(pt, 0, 0.02)
            base = MS.base_records(case, cam, pt.aa, pt.fade, 0, 0.02)
            assert st["base"] is base and st["how"] == MS.stack(pt)["how"]
            assert not (st["masked"] & st["visible"]).any() or st["how"] == "bound"
            if pt == MS.Point(case, cam):
                assert np.array_equal(st["visible"], _vis(base)) and FM.bits_equal(st["rgb"], np.ascontiguousarray(base["rgba"][:, :3]))
            # the splats the point cloud shows are among those the unmoded frame shows: the world's rows exist for all of them
            assert not (_vis(base) & ~_vis(MS.base_records(case, cam, False, False))).any()


# ---- the point cloud's known answers ------------------------------------------------------------------------------------------------------
def _project(case, cam, radius, dm, aa):
    """(project_draws' own records, the pair rectangles) of the view with the point cloud."""
    g, cu, su, proj, _ = FM.view(case, cam)
    su = DM.scene(su, dm, radius)
    block = orc.Camera176.from_buffer_copy(bytes(cu))
    with orc.frame_mode(ortho=int(proj == FM.ORTHO), aa_s=float(AAR.aa_s(MS.AA_VALUE, su.splat_scale)) if aa else 0.0):
        sp = orc.project_draws(block, su, g["pp"].tex, g["draws"], height_map=g["hm"]).copy()
        rc = orc.pair_rects(block, su, g["pp"].tex, g["draws"], W, Hh, height_map=g["hm"]).copy()
    return sp, rc


@pytest.mark.parametrize("aa", [False, True], ids=["plain", "antialias"])
@pytest.mark.parametrize("radius", RADII)
def test_an_isotropic_covariance_seen_orthographically_on_the_plain_surface_has_no_axes(radius, aa):
    """cov2d is exactly isotropic there: the eigenvector (c01, l1 - c00) is (0, 0), its normalisation 0 / 0, both axes NaN; the pair
    rectangles mark every survivor of the vertex stage invisible."""
    for dm in (0, 3):
        sp, rc = _project("case_plane", "oblique", radius, dm, aa)
        kept = _vis(sp)
        assert kept.sum() == 367
        assert np.isnan(sp["major"][kept]).all() and np.isnan(sp["minor"][kept]).all()
        assert not _vis(rc).any() and ((rc["tx1"] < rc["tx0"]) & (rc["ty1"] < rc["ty0"])).all()
        assert not _vis(MS.base_records("case_plane", "oblique", aa, False, dm, radius)).any()


def test_at_a_large_radius_rounding_breaks_the_tie():
    sp, rc = _project("case_plane", "oblique", 0.2, 0, False)
    assert _vis(sp).sum() == 367 and _vis(rc).sum() == 367 and np.isfinite(sp["major"][_vis(sp)]).all()


@pytest.mark.parametrize("radius", RADII)
def test_elsewhere_the_point_cloud_loses_nothing(radius):
    for case, cam in DM.VIEWS:
        if (case, cam) == ("case_plane", "oblique"):
            continue
        n0 = int(_vis(MS.base_records(case, cam, False, False)).sum())
        for dm in (0, 3):
            for aa in (False, True):
                sp, rc = _project(case, cam, radius, dm, aa)
                assert _vis(rc).sum() == n0 and np.array_equal(_vis(rc), _vis(MS.base_records(case, cam, False, False))), (case, cam, dm, aa)
                assert np.isfinite(sp["major"][_vis(rc)]).all() and np.isfinite(sp["minor"][_vis(rc)]).all()
    assert int(_vis(MS.base_records("case_sphere", "top", False, False, 0, radius)).sum()) == 2400


@pytest.mark.parametrize("case,cam", [("case_plane", "persp"), ("case_hmap", "persp")], ids=["plane-persp", "hmap-persp"])
def test_a_debug_draw_mode_scales_the_radius_by_the_tile_lod(case, cam):
    """pr = point_cloud_radius 2^tile_lod with draw_mode > 0: the axes of the draws with tile_lod > 0 differ from the draw_mode 0 ones, the
    others are the same bits.  (Every visible splat of the Sphere case belongs to a draw of tile_lod 0.)"""
    idx, _ = MS.draw_index(case)
    lod = np.array([int(d.tile.tile_id[0]) for d in OR.golden(case)["draws"]])[idx]
    a, b = MS.base_records(case, cam, False, False, 0, 0.02), MS.base_records(case, cam, False, False, 3, 0.02)
    vis = _vis(a) & _vis(b)
    up, flat = vis & (lod > 0), vis & (lod == 0)
    print(f"{case} {cam}: {int(up.sum())} visible splats in draws with tile_lod > 0, {int(flat.sum())} with tile_lod 0")
    assert up.sum() > 0 and flat.sum() > 0
    assert (np.abs(b["major"][up]).max(1) > np.abs(a["major"][up]).max(1)).all()
    for fld in ("major", "minor"):
        assert FM.bits_equal(np.ascontiguousarray(a[fld][flat]), np.ascontiguousarray(b[fld][flat])), fld


def test_a_mode_state_may_carry_its_scene_block():
    s = dict(cu="cu", su="su")
    mode = FM.Mode({"a": (None, dict(k=1)), "b": ("cam", dict(k=2), "scene")}, lambda r, name: None)
    assert FM._submit_kw(s, mode, "a") == ("cu", dict(k=1), "su") and FM._submit_kw(s, mode, "b") == ("cam", dict(k=2), "scene")
