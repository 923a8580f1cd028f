"""The hostile golden cases (tests/hostile_cases.py) and what tests/test_hostile_modes_gpu.py compares over them, checked without a GPU.

  * The cases: case_plane_hostile and case_hmap_hostile are make_golden.py's case_plane and case_hmap -- configuration, camera position,
    target, sort event -- over special_splats.hostile_tileset.
  * Populations, from the references alone: conditions on the seed, the ramp, the style table, the light and the clip volumes, not
    measurements.  Every count is printed.
  * Margin: the binary32 CPU compositor (tests/depth_ref.py) stays within FM.TOL / FM.ZTOL of tests/ortho_ref.composite_f64 on the hostile
    records at the cases' splat scale, so the image comparison of the GPU half needs no wider tolerance.
  * Mutations: a header promise broken in the reference must show on visible records, or the population does not discriminate it.  The
    ones that cannot show are named in test_what_no_visible_record_can_show, with the reason."""
import numpy as np
import pytest

from gswt_renderer_amd import _lib as L
from oracle import gswt_oracle as orc
from tests import atmosphere_ref as AR
from tests import clip_ref as CR
from tests import depth_ref as DR
from tests import frame_modes as FM
from tests import hostile_cases as HC
from tests import mode_stack_ref as MS
from tests import ortho_ref as OR
from tests import pick_ref as PR
from tests import shadow_ref as SR
from tests import special_splats as S
from tests import tile_style_ref as TR

F32 = np.float32
PLANE, HMAP = "case_plane_hostile", "case_hmap_hostile"
# every camera a hostile case is seen through; the GPU half runs the frame modes under MS.HOSTILE_CAMERAS' two per case
VIEWS = [(PLANE, "persp"), (PLANE, "top"), (PLANE, "oblique"), (HMAP, "persp"), (HMAP, "top")]
STACKED = [(case, cam) for case in (PLANE, HMAP) for cam in MS.HOSTILE_CAMERAS[case]]
CLS = {c: k for k, c in enumerate(S.CLASSES)}


def _ids(views):
    return [f"{case[5:]}-{cam}" for case, cam in views]


@pytest.fixture(autouse=True)
def _oracle_left_in_its_default_mode():
    yield
    assert orc.frame_mode_is_default()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _classes(case):
    return HC.instance_classes(OR.golden(case))


def _colour_words(case):
    g = OR.golden(case)
    gi = np.concatenate([np.asarray(d.gs_index, np.int64) for d in g["draws"]])
    return g["pp"].tex[gi][:, 7]


def _centres(case):
    """Plain surface: the binary32 centre of every instance."""
    g, _, su, _, _ = FM.view(case, "persp")
    return SR.centres_f32(su, g["pp"].tex, g["draws"])


# ---- the cases -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [PLANE, HMAP])
def test_a_hostile_case_is_its_golden_case_over_another_tile_set(case):
    g, b = OR.golden(case), OR.golden(HC.benign(case))
    assert g["cfg"] == b["cfg"] and g["pos"] == b["pos"] and g["tgt"] == b["tgt"] and (g["W"], g["H"]) == (b["W"], b["H"])
    assert bytes(g["cam"].uniforms()) == bytes(b["cam"].uniforms())
    # the same sort event over the same map: the same cells are drawn (which LOD a cell gets follows the tile set's own average scales)
    assert np.array_equal(np.unique(PR.identities(g["draws"])[0]), np.unique(PR.identities(b["draws"])[0]))
    assert any(d.tile.single_draw == 1 for d in g["draws"]) and any(d.tile.changing == 1 for d in g["draws"])
    verts = g["verts"]
    assert len(verts) == HC.N_LOD and verts[0][0].shape[0] == HC.LOD0_COUNT
    n = sum(len(x) for lod in g["labels"] for x in lod)
    assert (g["tex_class"] >= 0).sum() == n
    print(f"{case}: {sum(len(d.gs_index) for d in g['draws'])} instances in {len(g['draws'])} draws, {n} hostile rows of {g['pp'].tex.shape[0]}")


# ---- populations -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,cam", VIEWS, ids=_ids(VIEWS))
def test_every_class_is_instanced_and_all_but_the_non_finite_positions_are_visible(case, cam):
    cls = _classes(case)
    vis = MS.base_records(case, cam, False, False)["visible"] == 1
    counts = {c: (int((cls == k).sum()), int((vis & (cls == k)).sum())) for c, k in CLS.items()}
    print(f"{case} {cam}: {int(vis.sum())} of {vis.shape[0]} visible; instanced / visible per class: {counts}")
    for c, (n, v) in counts.items():
        assert n > 0, c
        assert (v == 0) if c == "nonfinite_pos" else (v > 0), (c, n, v)


def test_non_finite_positions_reach_every_stage_of_the_plane_case():
    """They are instanced in styled cells, in cells the light covers, and inside the keep volume but for the one coordinate that is not
    finite: the style lookup, the shadow's loads, the clip test and the fade all see them before the depth test rejects them."""
    g = OR.golden(PLANE)
    cls, ids = _classes(PLANE), PR.identities(g["draws"])[0]
    c = _centres(PLANE)
    nf = cls == CLS["nonfinite_pos"]
    bad = [~np.isfinite(x) for x in c]
    assert (bad[0] | bad[1])[nf].all() and not bad[2][nf].any() and not (bad[0] | bad[1])[~nf].any()
    kinds = [int((nf & np.isnan(c[0])).sum()), int((nf & np.isposinf(c[1])).sum()), int((nf & np.isneginf(c[0])).sum())]
    inp = MS.inputs(PLANE)
    sty = TR.lookup(inp.entries, ids)
    styled = ~TR.classes(sty)[3]
    # the row with its non-finite coordinate replaced by its cell's centre
    tw = F32(FM.view(PLANE, "persp")[2].tile_width)
    cell_mid = [c[0].copy(), c[1].copy(), c[2]]
    for cell in np.unique(ids):
        for k in range(2):
            cell_mid[k][(ids == cell) & bad[k]] = np.median(c[k][(ids == cell) & ~bad[k]])
    _, _, outside, _ = SR.lookup_f32(cell_mid, SR.params(inp.shadow))
    vols = CR.params(HC.plane_clip_volumes())
    keep = [v for v in vols if v["flags"] & 1]
    in_keep = CR.inside_f32(keep[0], *cell_mid)
    n = int(nf.sum())
    print(f"{n} instanced rows with a non-finite centre (NaN x {kinds[0]}, +Inf y {kinds[1]}, -Inf x {kinds[2]}; tile width {float(tw)}): {int((nf & styled).sum())} in a styled cell, "
          f"{int((nf & ~outside).sum())} in a cell the light covers, {int((nf & in_keep).sum())} inside the keep volume by their finite coordinates")
    assert n >= 10 and min(kinds) >= 1
    assert (nf & styled).sum() >= 5 and (nf & ~outside).sum() >= 5 and (nf & in_keep).sum() >= 5
    assert len(keep) == 1 and not CR.inside_f32(keep[0], *c)[nf].any()             # "a NaN coordinate is not inside" (an infinite one neither)


@pytest.mark.parametrize("case,cam", VIEWS, ids=_ids(VIEWS))
def test_a_record_is_visible_only_with_the_filter_on_and_its_alpha_is_zero(case, cam):
    unf = MS.base_records(case, cam, False, False)
    aa = MS.base_records(case, cam, True, False)
    only = (aa["visible"] == 1) & (unf["visible"] != 1)
    cls = _classes(case)
    print(f"{case} {cam}: visible {int((unf['visible'] == 1).sum())} -> {int((aa['visible'] == 1).sum())} with the filter; only with it: "
          f"{[S.CLASSES[k] for k in cls[only]]}, alpha bits {[hex(int(b)) for b in _bits(aa['rgba'][only][:, 3].copy())]}")
    assert only.sum() >= 1
    assert (_bits(aa["rgba"][only][:, 3].copy()) == 0).all()                        # +0.0 exactly
    assert not ((unf["visible"] == 1) & (aa["visible"] != 1)).any()


@pytest.mark.parametrize("case,cam", STACKED[:2], ids=_ids(STACKED[:2]))
def test_edge_bytes_meet_the_modes_on_the_plane_case(case, cam):
    st = MS.stack(MS.corner(case, cam))
    vis = st["visible"]
    w = _colour_words(case)
    ab = w >> 24
    ramp = (st["t"] > 0) & (st["t"] < 1)
    dim = (st["sty"][:, 4] > 0) & (st["sty"][:, 4] < 255)
    alpha = {b: int((vis & ramp & dim & (ab == b)).sum()) for b in (0, 1, 254, 255)}
    cb = np.stack([(w >> (8 * k)) & 0xFF for k in range(3)], 1)
    sets = dict(tinted=TR.classes(st["sty"])[2], shadowed=st["sh"] != 0, fogged=st["F"] > 0)
    colour = {name: {b: int((vis & m & (cb == b).any(1)).sum()) for b in (0, 255)} for name, m in sets.items()}
    print(f"{case} {cam}: visible splats on the ramp in a dimmed cell per alpha byte {alpha}; visible splats with a colour byte 0 / 255: {colour}")
    assert min(alpha.values()) >= 1
    assert all(v >= 1 for d in colour.values() for v in d.values())


def test_heights_and_cell_edges_meet_the_light_and_the_volumes():
    cls, c = _classes(PLANE), _centres(PLANE)
    _, _, outside, (_, _, ld) = SR.lookup_f32(c, SR.params(MS.inputs(PLANE).shadow))
    z = cls == CLS["z_extreme"]
    vols = CR.params(HC.plane_clip_volumes())
    box, half = vols[1], vols[2]
    assert box["shape"] == 0 and half["shape"] == 2 and not (box["flags"] | half["flags"]) & 1
    below = CR.inside_f32(half, *c)
    e = cls == CLS["edge_xy"]
    u0, u1, u2 = CR._unit(box, *c, F32)
    on_boundary = e & CR.inside_f32(box, *c) & (np.maximum(np.abs(u0), np.abs(u1)) == 1)
    vis = {cam: MS.base_records(PLANE, cam, False, False)["visible"] == 1 for cam in MS.HOSTILE_CAMERAS[PLANE]}
    print(f"z_extreme rows: {int((z & (ld < 0)).sum())} with ld < 0, {int((z & (ld > 1)).sum())} with ld > 1, {int((z & below).sum())} inside the cut half-space and "
          f"{int((z & ~below).sum())} outside; edge_xy rows on the cut box's boundary: {int(on_boundary.sum())}, visible "
          f"{ {cam: int((on_boundary & v).sum()) for cam, v in vis.items()} }")
    assert (z & (ld < 0)).sum() >= 5 and (z & (ld > 1)).sum() >= 5 and (z & below).sum() >= 5 and (z & ~below).sum() >= 5
    assert on_boundary.sum() >= 10 and all((on_boundary & v).sum() >= 5 for v in vis.values())
    assert CR.hidden(vols, *c)[on_boundary].all()                                   # the boundary is inside: the cut hides them


@pytest.mark.parametrize("case,cam", VIEWS, ids=_ids(VIEWS))
def test_duplicate_groups_tie_in_depth_bits(case, cam):
    unf = MS.base_records(case, cam, False, False)
    d = (unf["visible"] == 1) & (_classes(case) == CLS["duplicate"])
    _, cnt = np.unique(_bits(unf["depth"][d].copy()), return_counts=True)
    print(f"{case} {cam}: {int((cnt >= 2).sum())} groups of visible duplicates with one depth ({int((cnt >= 3).sum())} of three)")
    assert (cnt >= 2).sum() >= 10


RINT = [pt for cam in MS.HOSTILE_CAMERAS[PLANE] for pt in MS.square(PLANE, cam) if pt.fog]


@pytest.mark.parametrize("pt", RINT, ids=[pt.id for pt in RINT])
def test_the_fog_margin_masks_few_channels(pt):
    st = MS.stack(pt)
    assert st["how"] == "rint"
    near = AR.fog_bytes(st["codes"][st["visible"]])[1]
    print(f"{pt.id}: {int(near.sum())} of {near.size} channels inside AR.FOG_MARGIN")
    assert st["visible"].sum() >= 50 and near.mean() <= AR.MAX_MASKED
    assert np.isfinite(st["codes"][st["visible"]]).all()


@pytest.mark.parametrize("pt", [pt for case, cam in STACKED for pt in MS.square(case, cam)], ids=lambda pt: pt.id)
def test_visible_records_hold_no_nan_and_no_non_finite_centre(pt):
    """The GPU half compares NaN fields of visible records by _assert_varyings_equal's rule; on these cases the reference holds none, so
    the rule relaxes nothing here.  And no row with a non-finite centre is visible at any lattice point."""
    st = MS.stack(pt)
    vis = st["visible"]
    for fld in FM.FIELDS:
        assert not np.isnan(st["base"][fld][vis]).any(), fld
    assert not np.isnan(st["alpha"][vis]).any()
    assert not (vis & (_classes(pt.case) == CLS["nonfinite_pos"])).any() and vis.sum() >= 50


# ---- the CPU compositor's margin ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,cam", STACKED, ids=_ids(STACKED))
def test_the_binary32_compositor_stays_within_the_tolerances_on_hostile_records(case, cam):
    """Kilometre-wide floaters fill the frame and stack per pixel.  tests/depth_ref.py's binary32 blend against ortho_ref.composite_f64 over
    the same records, in depth order over the background, at HC.SPLAT_SCALE: within FM.TOL and FM.ZTOL on every pixel, so FM.image_case's
    comparison needs neither a lower splat scale nor its 2e-3 share of pixels for the reference's own error."""
    bgc, bgd = DR.bg_images(FM.W, FM.Hh)
    kw = dict(splat_scale=HC.SPLAT_SCALE, order_mode=L.GSWT_ORDER_DEPTH, bg_rgba=bgc, bg_depth=bgd)
    for name, sp in (("no mode", MS.base_records(case, cam, False, False)), ("filter and fade", MS.base_records(case, cam, True, True))):
        img, z, cover = DR.composite(sp, FM.W, FM.Hh, with_cover=True, **kw)
        i64, z64 = OR.composite_f64(sp, FM.W, FM.Hh, **kw)
        di, dz = float(np.abs(img - i64).max()), float(np.abs(z - z64).max())
        print(f"{case} {cam} {name}: splat scale {HC.SPLAT_SCALE}, up to {int(cover.max())} splats on a pixel ({float((cover > 0).mean()):.2f} of the frame covered); "
              f"binary32 against float64 max |colour| {di:.3e} (FM.TOL {FM.TOL:.0e}: margin x{FM.TOL / di:.0f}), max |depth| {dz:.3e} (FM.ZTOL {FM.ZTOL:.0e}: x{FM.ZTOL / dz:.0f})")
        assert di <= 0.1 * FM.TOL and dz <= 0.1 * FM.ZTOL
        assert (cover > 0).mean() > 0.3


# ---- mutations ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cam", MS.HOSTILE_CAMERAS[PLANE])
def test_a_light_coordinate_out_of_range_counted_as_shadowed_shows(cam):
    """`outside ... -> lit = 1` broken: a point outside the image or the depth range takes the full shade.  Colour is compared bit for bit
    at the points without fog, so every changed record would fail there."""
    st = MS.stack(MS.Point(PLANE, cam, shd=True))
    assert st["how"] == "exact"
    wd = MS.world(PLANE, cam)
    p = wd["p"]
    sh, _, outside, (u, v, ld) = SR.lookup_f32(_centres(PLANE), p)
    assert np.array_equal(_bits(sh), _bits(wd["sh"].astype(F32)))
    wrong = MS.colour_f32(st["base"]["rgba"][:, :3], st["sty"], np.where(outside, p["strength"], sh).astype(F32), p)
    changed = st["visible"] & (_bits(wrong) != _bits(st["rgb"])).any(1)
    by_depth = st["visible"] & ~((ld >= 0) & (ld <= 1))
    print(f"{PLANE} {cam}: {int((st['visible'] & outside).sum())} visible splats outside the light ({int(by_depth.sum())} by ld alone), {int(changed.sum())} records change")
    assert changed.sum() >= 1 and (changed & by_depth).sum() >= 1 and not (changed & ~outside).any()


@pytest.mark.parametrize("case,cam", STACKED, ids=_ids(STACKED))
def test_what_no_visible_record_can_show(case, cam):
    """Four of the promises act only on records that no frame shows, whatever the population:

      * comp "a NaN gives 0", "A NaN dist clamps to 0", "a NaN coordinate is not inside", and the NaN half of "outside -> lit = 1".  The
        half decode reads an Inf / NaN covariance half as 0 and the largest finite one is 65504, so with a finite centre cov2d, l1 and l2
        are finite and comp, dist and every coordinate are numbers; with a non-finite centre ndc and depth are not finite either and A10's
        depth test (0 <= depth <= 1, false for a NaN) rejects the record behind all of them.  Mapping comp's NaN to 1, keeping a NaN
        distance or counting a NaN coordinate as inside or as shadowed changes no visible record and no n_visible: asserted here as "no row
        with a non-finite centre is visible", under the filter and the fade too.  What the GPU half can and does see of these promises is
        that such rows, which reach every stage (test_non_finite_positions_reach_every_stage_of_the_plane_case), leave `visible`, n_visible
        and every other record as the reference has them; the known answers pin the arithmetic (comp's zero, the NaN texel).
      * the requantisers' clamp.  Tint, shade and fog are convex mixes of numbers in 0 .. 1 in this order, so the float colour stays in
        0 .. 1 up to rounding, and rint(255 c) is the same byte with and without the clamp: asserted on the unclamped float64 chain."""
    cls = _classes(case)
    nf = cls == CLS["nonfinite_pos"]
    shown = sum(int(((MS.base_records(case, cam, aa, fade)["visible"] == 1) & nf).sum()) for aa in (False, True) for fade in (False, True))
    st = MS.stack(MS.corner(case, cam))
    vis = st["visible"]
    wd = MS.world(case, cam)
    dist = np.where(np.isfinite(wd["dist"]), wd["dist"], 0.0)
    # the chain without its final clip: staged, with the clip undone by comparing against the unclipped float colour
    sty, s, p, fog_p = st["sty"], st["sh"], wd["p"], AR.params(MS.atmosphere_of(st["point"]))
    tinted = TR.classes(sty)[2]
    c = st["base"]["rgba"][:, :3].astype(np.float64)
    k = (sty[:, 3].astype(np.float64) / 255.0)[:, None] * tinted[:, None]
    c = c * (1.0 - k) + sty[:, :3].astype(np.float64) / 255.0 * k
    c = c * (1.0 - s[:, None]) + p["shade"].astype(np.float64)[None, :] * s[:, None]
    dry = c                                                                         # what tint_requantise quantises with the fog off
    F = AR.fog_amount_f64(dist, fog_p)[:, None]
    c = c * (1.0 - F) + fog_p["fog_color"].astype(np.float64)[None, :] * F
    lo, hi = float(min(c[vis].min(), dry[vis].min())), float(max(c[vis].max(), dry[vis].max()))
    print(f"{case} {cam}: {int(nf.sum())} rows with a non-finite centre, visible in any of the four filter / fade frames: {shown}; the unclamped colour of the "
          f"{int(vis.sum())} visible splats spans {lo:.6f} .. {hi:.6f}, bytes 0 and 255 among them in front of the fog: {int((np.rint(255 * dry[vis]) == 0).sum())}, {int((np.rint(255 * dry[vis]) == 255).sum())}")
    assert nf.sum() >= 5 and shown == 0
    for x in (c, dry):
        assert np.array_equal(np.rint(255.0 * x[vis]), np.rint(255.0 * np.clip(x[vis], 0.0, 1.0)))
    assert (np.rint(255 * dry[vis]) == 0).any() and (np.rint(255 * dry[vis]) == 255).any()
