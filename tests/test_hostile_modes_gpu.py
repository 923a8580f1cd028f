"""Splat records outside the benign region under every frame mode, on the GPU.  The mode tests (tests/test_ortho_gpu.py ...
tests/test_mode_stack_gpu.py) run on the benign golden cases, the special-splat tests (tests/test_special_splats_gpu.py) as perspective
frames with no mode on; here the two meet.  The cases are tests/hostile_cases.py's (pinned without a GPU by
tests/test_hostile_modes_cpu.py), the references tests/mode_stack_ref.py's and the oracle's; frames are 72 x 40 and 32 x 32.

  a. the lattice on the hostile plane case: test_mode_stack_gpu.test_lattice_point's procedure at all sixteen (AA, ATM, STY, SHD) points
     under the perspective and the oblique camera, then the clip volumes alone and on the all-on corner;
  b. the hostile HeightMap case under the perspective and the top camera: records bit for bit where colour is "exact"; at the all-on
     corner `visible`, n_visible, geometry and alpha bit for bit and colour NOT compared: mode_stack_ref's "bound" derivation unprojects
     finite, well-conditioned records, which these are not (a floater's record is finite, but the bound's per-splat terms assume a
     footprint that its centre's neighbourhood represents);
  c. every f16 pattern of a covariance slot under ORTHO, under AA at 102 and 2048, and under both, bit for bit against the oracle;
  d. known answers, one per promise of include/gswt_hip.h;
  e. the same bytes every way (tests/frame_modes.py's battery) over the hostile plane case.

A field of a visible record that is a NaN on both sides counts as equal whatever its payload, and nothing else is relaxed
(FM.bits_equal_or_nan; on these cases the reference holds no NaN in a visible record, tests/test_hostile_modes_cpu.py)."""
import functools

import numpy as np
import pytest

from gswt_renderer_amd import _lib as L
from gswt_renderer_amd import atmosphere as A
from gswt_renderer_amd import ortho, shadows
from oracle import gswt_oracle as orc
from tests import antialias_ref as AAR
from tests import atmosphere_ref as AR
from tests import clip_ref as CR
from tests import depth_ref as DR
from tests import frame_modes as FM
from tests import hostile_cases as HC
from tests import mode_stack_ref as MS
from tests import ortho_ref as OR
from tests import shadow_ref as SR
from tests import special_splats as S
from tests import tile_style_ref as TR
from tests.test_special_splats_gpu import _assert_varyings_equal

pytestmark = pytest.mark.gpu
W, Hh = OR.W, OR.H
F32 = np.float32
ORTHO, PERSP = L.GSWT_PROJECTION_ORTHO, L.GSWT_PROJECTION_PERSPECTIVE
PLANE, HMAP = "case_plane_hostile", "case_hmap_hostile"
MIN_COVER = 0.3


@pytest.fixture(autouse=True)
def _defaults(renderer):
    """FM.restore_defaults knows neither the shadow map nor the clip volumes: the shared context goes back without them as well."""
    yield
    renderer.set_shadow_map(None)
    renderer.set_clip_volumes(None)
    FM.restore_defaults(renderer)


# ---- a. the lattice on the hostile plane case ---------------------------------------------------------------------------------------------------
PLANE_LATTICE = MS.square(PLANE, "persp") + MS.square(PLANE, "oblique")


@pytest.mark.parametrize("pt", PLANE_LATTICE, ids=[pt.id for pt in PLANE_LATTICE])
def test_lattice_point_on_the_hostile_plane(renderer, pt):
    st = MS.stack(pt)
    print(f"{pt.id}: {pt.instantiation(True)} and DEBUG=0 [{st['how']}]: " + ", ".join(f"{k} {v}" for k, v in MS.populations(st).items()))
    c = FM.image_case(renderer, pt.cam, L.GSWT_ORDER_DEPTH, True, HC.SPLAT_SCALE, MS.render_kw(pt), "hostile " + pt.id, min_cover=MIN_COVER, name=PLANE)
    print(MS.check_records(c["sp"], c["t_debug"]["n_visible"], st, nan_equal=True))
    assert (c["t"]["n_visible"], c["t"]["n_pairs"]) == (c["t_debug"]["n_visible"], c["t_debug"]["n_pairs"]) and c["t"]["n_pairs"] > 0


def clipped_stack(pt):
    """mode_stack_ref's records of a plane point with the splats tests/clip_ref.py's binary32 restatement hides under
    HC.plane_clip_volumes() removed: exact, no mask."""
    g, _, su, _, _ = FM.view(pt.case, pt.cam)
    hid = CR.hidden(CR.params(HC.plane_clip_volumes()), *SR.centres_f32(su, g["pp"].tex, g["draws"]))
    st = dict(MS.stack(pt))
    full = int(st["visible"].sum())
    st["visible"] = st["visible"] & ~hid
    return st, full


CLIPPED = [MS.Point(PLANE, cam) for cam in MS.HOSTILE_CAMERAS[PLANE]] + [MS.corner(PLANE, cam) for cam in MS.HOSTILE_CAMERAS[PLANE]]


@pytest.mark.parametrize("pt", CLIPPED, ids=[pt.id + "+clip" for pt in CLIPPED])
def test_clip_volumes_on_the_hostile_plane(renderer, pt):
    """The volumes alone and on top of the all-on corner: edge_xy rows on the cut box's boundary (inside), z_extreme rows on both sides of
    the half-space, and rows with a NaN or infinite coordinate, which are inside nothing -- not in the keep box either."""
    st, full = clipped_stack(pt)
    kept = int(st["visible"].sum())
    print(f"{pt.id} + clip: {full} -> {kept} visible")
    assert 0 < kept < full
    kw = dict(MS.render_kw(pt), clip_volumes=HC.plane_clip_volumes())
    c = FM.image_case(renderer, pt.cam, L.GSWT_ORDER_DEPTH, True, HC.SPLAT_SCALE, kw, "hostile " + pt.id + "+clip", min_cover=MIN_COVER, name=PLANE)
    print(MS.check_records(c["sp"], c["t_debug"]["n_visible"], st, nan_equal=True))
    assert (c["t"]["n_visible"], c["t"]["n_pairs"]) == (c["t_debug"]["n_visible"], c["t_debug"]["n_pairs"]) and c["t"]["n_pairs"] > 0


# ---- b. the hostile HeightMap case -----------------------------------------------------------------------------------------------------------------
def _hmap_points(cam):
    P = MS.Point
    return [P(HMAP, cam), P(HMAP, cam, aa=True), P(HMAP, cam, atm="fade"), P(HMAP, cam, sty=True), P(HMAP, cam, aa=True, atm="fade", sty=True), MS.corner(HMAP, cam)]


HMAP_POINTS = _hmap_points("persp") + _hmap_points("top")


@pytest.mark.parametrize("pt", HMAP_POINTS, ids=[pt.id for pt in HMAP_POINTS])
def test_point_on_the_hostile_height_map(renderer, pt):
    st = MS.stack(pt)
    exact = st["how"] == "exact"
    assert exact == (not pt.shd and not pt.fog)
    g, cu, su, proj, _ = FM.view(pt.case, pt.cam)
    FM.bind(renderer, g)
    got, t = FM.varyings(renderer, cu, su, projection=proj, **MS.render_kw(pt))
    print(f"{pt.id}: {pt.instantiation(True)} [{st['how']}]: " + ", ".join(f"{k} {v}" for k, v in MS.populations(st).items()))
    # with the shadow or the fog on, colour hangs on the float64 unprojection of records that are not well conditioned: not compared
    print(MS.check_records(got, t["n_visible"], st, nan_equal=True, colour=exact))
    # ... and the normal instantiation over k_cull's live table counts the same
    renderer.render(cu, su, W, Hh, projection=proj)
    tn = renderer.timings()
    assert (tn["n_visible"], tn["n_pairs"]) == (t["n_visible"], t["n_pairs"]) and t["n_pairs"] > 0


# ---- c. every f16 pattern under the modes -------------------------------------------------------------------------------------------------------------
HALF_W = HALF_H = 32
HALF_MODES = {"ortho": (True, 0), "aa102": (False, 102), "aa2048": (False, 2048), "ortho+aa102": (True, 102), "ortho+aa2048": (True, 2048)}


@functools.lru_cache(maxsize=None)
def half_pattern_scene(slot):
    """test_every_half_pattern_through_the_vertex_stage's scene of the slot, its perspective camera and an orthographic one along the same
    line of sight (16 px per world unit): for xy the diagonal view, which keeps xy in the 2D covariance."""
    pats = np.arange(65536)
    rows = np.tile(S.tex_row((0.0, 4.0, 5.0), [0] * 6, (200, 100, 50, 255)), (65536, 1))
    if slot == "xx":
        eye = (0.0, 0.0, 5.0)
        base = S.cov_halves(yy=1e-3, zz=1e-3)
        halves = [pats] + [np.full(65536, h) for h in base[1:]]
    else:
        eye = (-3.0, 1.0, 5.0)
        base = S.cov_halves(xx=1.0, yy=1.0, zz=0.5)
        halves = [np.full(65536, base[0]), pats] + [np.full(65536, h) for h in base[2:]]
    xx, xy, xz, yy, yz, zz = [np.asarray(h, np.uint32) & 0xFFFF for h in halves]
    rows[:, 4], rows[:, 5], rows[:, 6] = xx | xy << 16, xz | yy << 16, yz | zz << 16
    persp = orc.Camera(HALF_W, HALF_H, eye, (0.0, 4.0, 5.0), [0, 0, 1]).uniforms()
    orth = OR.camera_block(HALF_W, HALF_H, eye, (0.0, 4.0, 5.0), (0.0, 0.0, 1.0), 1.0, 0.5, 20.0)
    return S.raw_scene(rows), persp, orth


def half_pattern_reference(slot, mode):
    sc, persp, orth = half_pattern_scene(slot)
    is_ortho, value = HALF_MODES[mode]
    su = orc.scene_uniforms(num_lod=1)
    od, pd = sc.draws(valid_lod_id=0)
    cu = orth if is_ortho else persp
    with orc.frame_mode(ortho=int(is_ortho), aa_s=float(AAR.aa_s(value, su.splat_scale)) if value else 0.0):
        want = orc.project_draws(cu, su, sc.tex, od).copy()
    return sc, pd, cu, su, want


@pytest.mark.parametrize("mode", list(HALF_MODES))
@pytest.mark.parametrize("slot", ["xx", "xy"])
def test_every_half_pattern_under_the_modes(renderer, slot, mode):
    sc, pd, cu, su, want = half_pattern_reference(slot, mode)
    is_ortho, value = HALF_MODES[mode]
    with renderer.options(NO_LOD_PREFILTER=1, DEBUG_VARYINGS=1):          # (the option is read when the draws are set)
        renderer.configure(None)
        sc.upload(renderer)
        renderer.set_draws(pd)
        renderer.render(cu, su, HALF_W, HALF_H, projection=ORTHO if is_ortho else PERSP, antialias=value / 1024.0)
        got = renderer.read_projected()
    n_vis = _assert_varyings_equal(got, want, (slot, mode))
    print(f"{slot} {mode}: {n_vis} of 65536 patterns visible")
    assert n_vis > 1000, n_vis
    vis = want["visible"] == 1
    assert vis[0x0001:0x0400].sum() > 500 and vis[0x0400]
    if slot == "xy":
        assert vis[0x7C00] and vis[0x7E00] and vis[0xFC00]


# ---- d. known answers, one per header promise -------------------------------------------------------------------------------------------------------------
def _bind_raw(renderer, scene, **tile_kw):
    od, pd = scene.draws(**tile_kw)
    renderer.configure(None)
    scene.upload(renderer)
    renderer.set_draws(pd)
    return od


def _top_down():
    return ortho.top_down((2.0, 2.0), 3.0, 5.0, -5.0, W, Hh).uniforms()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def test_a_zero_minor_eigenvalue_shows_only_under_the_filter_with_alpha_zero(renderer):
    """comp = clamp(sqrtf(l1 / l1f) * sqrtf(l2 / l2f), 0, 1) at l2 == 0.  A flat splat, xx = 0, seen straight down: cov2d is diag(0, c11),
    l2 = 0 exactly and the direction (0, 1) is well defined.  Without the filter its minor axis is zero and F2 rejects it.  With the filter the
    axes are sqrt(2 s), sqrt(2 (l1 + s)), the record is visible and comp = sqrt(l1 / l1f) * sqrt(0 / s) = +0.0: alpha is exactly 0.0, the
    frame is the empty frame byte for byte, the depth image the background's, and no pick record names the splat."""
    scene = S.raw_scene([((2.0, 2.0, 0.0), S.cov_halves(yy=4.0 * 0.3 ** 2, zz=4.0 * 0.25 ** 2), (255, 128, 0, 255))])
    od = _bind_raw(renderer, scene, map_index=7)
    su, cu = orc.scene_uniforms(num_lod=1), _top_down()
    bgc, bgd = DR.bg_images(W, Hh)
    kw = dict(projection=ORTHO, order_mode=L.GSWT_ORDER_DEPTH, bg_rgba=bgc, bg_depth=bgd, depth=True, pick=True)
    off, t_off = FM.varyings(renderer, cu, su, projection=ORTHO, antialias=0.0)
    assert off[0]["visible"] == 0 and t_off["n_visible"] == 0
    empty = renderer.render(cu, su, W, Hh, antialias=0.0, **kw)
    assert FM.same(empty[0], bgc) and FM.same(empty[1], bgd) and not (empty[2]["weight"] > 0).any()
    for value in (102, 307, 2048):
        with orc.frame_mode(ortho=1, aa_s=float(AAR.aa_s(value, su.splat_scale))):
            want = orc.project_draws(cu, su, scene.tex, od)
        got, t = FM.varyings(renderer, cu, su, projection=ORTHO, antialias=value / 1024.0)
        assert want[0]["visible"] == 1 and _bits(want["rgba"][:, 3].copy())[0] == 0
        assert got[0]["visible"] == 1 and t["n_visible"] == 1, value
        assert _bits(got["rgba"][:, 3].copy())[0] == 0, value                    # +0.0, not -0.0 and not a NaN
        for fld in FM.FIELDS:
            assert FM.bits_equal(np.ascontiguousarray(got[fld]), np.ascontiguousarray(want[fld])), (value, fld)
        img, z, pick = renderer.render(cu, su, W, Hh, antialias=value / 1024.0, **kw)
        assert renderer.timings()["n_visible"] == 1 and renderer.timings()["n_pairs"] > 0
        for a, b in zip((img, z, pick), empty):
            assert FM.same(a, b), value
        assert not (pick["weight"] > 0).any() and not (pick["map_index"] == 7).any()


@pytest.mark.parametrize("value", [307, 2048])
def test_k9_exactly_isotropic_centred_splat_draws_nothing_under_the_filter(renderer, value):
    """The NaN axes of K9's splat come from the direction, normalize(vec2(0, 0)), which stays the unfiltered cov2d's: the filter's finite
    lengths times a NaN direction are NaN, F1 / F2 reject the record, nothing is drawn."""
    Wk = Hk = 64
    cu = orc.default_camera(Wk, Hk).uniforms()
    su = orc.scene_uniforms(num_lod=1)
    scene = S.raw_scene([((0.0, 4.0, 5.0), S.diag_halves((0.05, 0.05, 0.05)), (255, 128, 0, 255))])
    od, _ = scene.draws(valid_lod_id=0)
    with orc.frame_mode(aa_s=float(AAR.aa_s(value, su.splat_scale))):
        want = orc.project_draws(cu, su, scene.tex, od)
    assert np.isnan(want[0]["major"]).all() and np.isnan(want[0]["minor"]).all()
    with renderer.options(NO_LOD_PREFILTER=1, DEBUG_VARYINGS=1):
        _bind_raw(renderer, scene, valid_lod_id=0)
        renderer.render(cu, su, Wk, Hk, antialias=value / 1024.0)
        got = renderer.read_projected()
    assert _assert_varyings_equal(got, want, value) == 0
    _bind_raw(renderer, scene, valid_lod_id=0)
    for order_mode in (L.GSWT_ORDER_REFERENCE, L.GSWT_ORDER_DEPTH):
        img = renderer.render(cu, su, Wk, Hk, antialias=value / 1024.0, order_mode=order_mode)
        t = renderer.timings()
        assert (t["n_visible"], t["n_pairs"]) == (0, 0) and not img.any()


def test_a_nan_texel_is_lit(renderer):
    """tests/test_shadow_gpu.py's known-answer scene under the unit light, with NaN in the two columns of texels that shadow its points
    there: r > NaN is false, the texel is lit, every record's colour is the unshadowed one bit for bit.  With 0.25 in their place the same
    points are shadowed (the control)."""
    from tests.test_shadow_gpu import BIAS, POINTS
    halves = S.diag_halves((0.03, 0.06, 0.03))
    colours = [(200, 96 + 8 * k, 48, 255) for k in range(len(POINTS))]
    scene = S.raw_scene([(p, halves, c) for p, c in zip(POINTS, colours)])
    _bind_raw(renderer, scene, map_index=7)
    su, cu = orc.scene_uniforms(num_lod=1), _top_down()
    base, _ = FM.varyings(renderer, cu, su, projection=ORTHO, shadow=shadows.OFF)
    assert (base["visible"] == 1).all()
    c = [np.array([q[k] for q in POINTS], F32) for k in range(3)]
    changed = {}
    for name, left in (("nan", np.nan), ("control", 0.25), ("mixed", None)):
        Z = np.ones((4, 4), F32)
        Z[:, :2] = 0.25 if left is None else left
        if left is None:
            Z[:, 0] = np.nan                                   # column 0 NaN beside a shadowing column 1: the mix of a lit and a shadowed texel
        m = SR.unit_light(Z, bias=BIAS, strength=0.5)
        p = SR.params(m)
        sh = SR.lookup_f32(c, p)[0]
        got, t = FM.varyings(renderer, cu, su, projection=ORTHO, shadow=m)
        assert t["n_visible"] == len(POINTS) and np.array_equal(got["visible"], base["visible"])
        want = SR.shaded_rgb_f32(base["rgba"][:, :3], sh, p)
        assert FM.bits_equal(np.ascontiguousarray(got["rgba"][:, :3]), want), name
        for fld in ("ndc", "depth", "major", "minor"):
            assert FM.bits_equal(np.ascontiguousarray(got[fld]), np.ascontiguousarray(base[fld])), (name, fld)
        changed[name] = (_bits(got["rgba"]) != _bits(base["rgba"])).any(1)
        if name == "nan":
            assert (sh == 0).all()
            for fld in FM.FIELDS:
                assert FM.bits_equal(np.ascontiguousarray(got[fld]), np.ascontiguousarray(base[fld])), fld
    assert not changed["nan"].any() and changed["control"][[1, 2, 7, 8]].all() and changed["mixed"].any()
    assert changed["mixed"].sum() < changed["control"].sum() or not np.array_equal(changed["mixed"], changed["control"])


def test_colour_bytes_0_and_255_through_tint_shadow_and_fog_at_full_strength(renderer):
    """q(x): the requantisers on the bytes' ends.  Opaque splats of colour (0, 255, 0) in a cell tinted (255, 0, 255) at strength 255,
    under a map that shadows everything at strength 1 towards (1, 0, 0), through a fog of fog_max 1 towards (0, 1, 1): each stage alone
    and all three, at five distances.  Every byte stays in 0 .. 255 and is shadow_ref.chain_codes_f64's rint (within one code inside
    AR.FOG_MARGIN of a half-integer)."""
    zs = (2.0, 1.0, 0.0, -1.0, -1.75)
    scene = S.raw_scene([((2.0, 2.0, z), S.diag_halves((0.03, 0.06, 0.03)), (0, 255, 0, 255)) for z in zs])
    _bind_raw(renderer, scene, map_index=7)
    su, cu = orc.scene_uniforms(num_lod=1), _top_down()
    block = orc.Camera176.from_buffer_copy(bytes(cu))
    dist = np.array([abs(float(block.cam_pos[2]) - z) for z in zs])
    assert float(block.cam_pos[0]) == 2.0 and float(block.cam_pos[1]) == 2.0
    tint = (255, 0, 255, 255)
    table = TR.pack(TR.entries({7: TR.entry(tint[:3], tint[3])}, 8))
    m = SR.unit_light(np.zeros((4, 4), F32), bias=0.0, strength=1.0, shade_color=(1.0, 0.0, 0.0))
    fog = A.Atmosphere(fog=(0.35, 2.0, 1.0, (0.0, 1.0, 1.0)))
    p, fog_p = SR.params(m), AR.params(fog)
    centres = [np.full(len(zs), 2.0, F32), np.full(len(zs), 2.0, F32), np.array(zs, F32)]
    sh = SR.lookup_f32(centres, p)[0].astype(np.float64)
    assert (sh[1:] == 1.0).all()                                # (the topmost splat sits on the light's near plane, r = 0 > 0 is false: lit)
    base, _ = FM.varyings(renderer, cu, su, projection=ORTHO, shadow=shadows.OFF, atmosphere=A.OFF, tile_styles=b"")
    assert (base["visible"] == 1).all() and np.array_equal(AR.bytes_of(base["rgba"]), np.tile([0.0, 255.0, 0.0], (len(zs), 1)))
    seen = set()
    for sty_on in (False, True):
        for shd_on in (False, True):
            for fog_on in (False, True):
                got, t = FM.varyings(renderer, cu, su, projection=ORTHO, shadow=m if shd_on else shadows.OFF, atmosphere=fog if fog_on else A.OFF,
                                     tile_styles=table if sty_on else b"")
                label = (sty_on, shd_on, fog_on)
                assert t["n_visible"] == len(zs) and (got["visible"] == 1).all(), label
                codes = SR.chain_codes_f64(base["rgba"][:, :3], tint if sty_on else None, sh if shd_on else np.zeros(len(zs)), p, dist if fog_on else None,
                                           fog_p if fog_on else None)
                have = got["rgba"][:, :3].astype(np.float64) * 255.0
                assert np.abs(have - np.rint(have)).max() < 1e-4 and have.min() >= 0.0 and have.max() <= 255.0, label
                want, near = AR.fog_bytes(codes)
                assert np.abs(np.rint(have) - want).max() <= 1.0 and np.array_equal(np.rint(have)[~near], want[~near]), (label, have, codes)
                assert FM.bits_equal(got["rgba"][:, 3].copy(), base["rgba"][:, 3].copy()), label
                seen |= set(np.rint(have).ravel().tolist())
    assert {0.0, 255.0} <= seen and len(seen) > 4


def test_alpha_bytes_0_and_255_through_dim_fade_and_comp(renderer):
    """The dim x fade x comp x LOD-share product on the alpha byte's ends: splats of alpha 0, 1, 254 and 255 in a dimmed cell, on the fade's
    ramp, under the filter.  Bit for bit tile_style_ref.dimmed_alpha of the oracle's alpha, which holds (alpha . comp) . fs."""
    alphas = (0, 1, 254, 255)
    zs = (1.0, 0.0, -1.0)
    scene = S.raw_scene([((1.0 + 0.5 * k, 2.0, z), S.diag_halves((0.03, 0.06, 0.03)), (200, 100, 50, a)) for z in zs for k, a in enumerate(alphas)])
    od = _bind_raw(renderer, scene, map_index=7)
    su, cu = orc.scene_uniforms(num_lod=1), _top_down()
    fade = A.Atmosphere(fade=(3.0, 7.0))
    fp = AR.params(fade)
    sty = np.tile(np.array(TR.entry(dim=77), np.uint8), (len(zs) * len(alphas), 1))
    table = TR.pack(TR.entries({7: TR.entry(dim=77)}, 8))
    for value in (0, 307):
        with orc.frame_mode(ortho=1, aa_s=float(AAR.aa_s(value, su.splat_scale)) if value else 0.0, fade=(float(fp["fade_end"]), float(fp["fade_inv"]))):
            want = orc.project_draws(cu, su, scene.tex, od)
        assert (want["visible"] == 1).all()
        alpha = TR.dimmed_alpha(want["rgba"][:, 3], sty)
        got, t = FM.varyings(renderer, cu, su, projection=ORTHO, antialias=value / 1024.0, atmosphere=fade, tile_styles=table)
        assert t["n_visible"] == len(sty) and (got["visible"] == 1).all()
        assert FM.bits_equal(got["rgba"][:, 3].copy(), alpha.copy()), (value, got["rgba"][:, 3], alpha)
        a = alpha.reshape(len(zs), len(alphas))
        assert (_bits(a[:, 0].copy()) == 0).all() and (a[:, 1] > 0).all() and (a[:, 1] < a[:, 2]).all() and (a[:, 3] < 1).all()
        for fld in ("ndc", "depth", "major", "minor"):
            assert FM.bits_equal(np.ascontiguousarray(got[fld]), np.ascontiguousarray(want[fld])), (value, fld)
        assert FM.bits_equal(np.ascontiguousarray(got["rgba"][:, :3]), np.ascontiguousarray(want["rgba"][:, :3])), value


# ---- e. the same bytes every way -------------------------------------------------------------------------------------------------------------------------
def _states(cam, proj):
    on = MS.render_kw(MS.corner(PLANE, cam))
    off = MS.render_kw(MS.Point(PLANE, cam))
    wide = dict(on, antialias=2048 / 1024.0)                  # 2 px^2, the largest value the tests use, over the floaters
    states = {"off": dict(off, clip_volumes=[]), "all_on": dict(on, clip_volumes=[]), "all_on_clip": dict(on, clip_volumes=HC.plane_clip_volumes()),
              "all_on_aa2048": dict(wide, clip_volumes=[])}
    return {name: (None, dict(kw, projection=proj)) for name, kw in states.items()}


def _set_state(states):
    def set_state(r, name):
        kw = states[name][1]
        r._set_frame_modes(kw["projection"], kw["antialias"], kw["atmosphere"], kw["tile_styles"], kw["shadow"], kw["clip_volumes"])
    return set_state


def _plain(renderer, cam):
    """The hostile plane case bound under the camera, depth order over a background, and the plain synchronous frames (colour, depth,
    pick) of the states."""
    g, cu, su, proj, _ = FM.view(PLANE, cam, HC.SPLAT_SCALE)
    states = _states(cam, proj)
    mode = FM.Mode(states, _set_state(states), on="all_on")
    s = FM.plain_frames(renderer, mode, g, su, cu)
    assert len({bytes(np.ascontiguousarray(f[0])) for f in s["frames"].values()}) == len(states)
    assert 0 < s["pairs"]["all_on_clip"] < s["pairs"]["all_on"] < s["pairs"]["all_on_aa2048"]
    for f in s["frames"].values():
        assert np.isfinite(f[0]).all() and np.isfinite(f[1]).all()
    return dict(s, mode=mode, cam=cam)


@pytest.fixture(params=["persp", "oblique"])
def plain(renderer, request):
    return _plain(renderer, request.param)


NAMES = ["off", "all_on", "all_on_clip"]


def test_the_chunk_cull_off_changes_nothing(renderer, plain):
    FM.check_with_option_on(renderer, plain, plain["mode"], L.GSWT_OPT_NO_CHUNK_CULL, NAMES)


def test_row_shards_tile_the_frame(renderer, plain):
    FM.check_row_shards(renderer, plain, plain["mode"], 3, NAMES)


def test_column_bands_unite_to_the_frame(renderer):
    """The band cull's per-record extent bound is computed at upload, without the filter's widening: the filter at 2048 over the floaters
    is the point.  Perspective only: orthographic column bands are refused."""
    plain = _plain(renderer, "persp")
    FM.check_column_bands(renderer, plain, plain["mode"], 3, NAMES + ["all_on_aa2048"])


def test_pair_buffer_overflow_rerun(renderer, plain):
    FM.check_overflow_rerun(renderer, plain, plain["mode"], "all_on_clip", then="off")


def test_graph_replay_with_alternating_states(renderer, plain):
    seq1 = ["off", "all_on", "all_on_clip", "all_on", "off", "all_on_clip"]
    seq2 = ["all_on_clip", "off", "all_on", "all_on_clip", "off", "all_on"]
    FM.check_graph_replay(renderer, plain, plain["mode"], seq1, seq2)


def test_output_formats(renderer, plain):
    FM.check_output_formats(renderer, plain, plain["mode"], NAMES)
