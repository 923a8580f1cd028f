"""Clip volumes (gswt_set_clip_volumes, include/gswt_hip.h) on the GPU: boxes, ellipsoids and half-spaces cut the splats by centre.
Frames are 72 x 40 (tests/ortho_ref.py) on the golden cases with the draws of their own perspective sort event.

The clipped vertex stage against tests/clip_ref.py: on the plain surface `visible` is the unclipped frame's minus the binary32
restatement's hidden splats, with no mask, and every field of a surviving splat is the unclipped frame's bit for bit (DEBUG and normal
instantiation, perspective and orthographic, pixel filter off and on); on the HeightMap and Sphere surfaces the same with the float64
unprojection and the margins' mask.  Known answers; image, depth and pick against the CPU references over the surviving records; the
same bytes through graphs, frames in flight, a pair-buffer overflow, the chunk cull off, output formats and shards; off leaves
every output as it was; the refusals; clip stacked on the other four modes; and a sun map rendered with a cut volume, from which the
cut-away part casts no shadow."""
import ctypes as C

import numpy as np
import pytest

from gswt_renderer_amd import _lib as L
from gswt_renderer_amd import clip as CL
from gswt_renderer_amd import ortho, shadows
from gswt_renderer_amd.renderer import GSWTError
from oracle import gswt_oracle as orc
from tests import antialias_ref as AAR
from tests import atmosphere_ref as AR
from tests import clip_ref as CR
from tests import depth_ref as DR
from tests import frame_modes as FM
from tests import mode_stack_ref as MS
from tests import ortho_ref as OR
from tests import shadow_ref as SR
from tests import special_splats as S

pytestmark = pytest.mark.gpu
W, Hh = OR.W, OR.H
F32 = np.float32
ORTHO, PERSP = L.GSWT_PROJECTION_ORTHO, L.GSWT_PROJECTION_PERSPECTIVE
AA_VALUE = 307
AA = AA_VALUE / 1024.0
PLANE = CR.volume_sets("case_plane")
V = CL.ClipVolume


@pytest.fixture(autouse=True)
def _defaults(renderer):
    """FM.restore_defaults knows neither the clip volumes nor the shadow map: the shared context goes back without them as well."""
    yield
    renderer.set_clip_volumes(None)
    renderer.set_shadow_map(None)
    FM.restore_defaults(renderer)


def _same_fields(got, base, m, label):
    for fld in FM.FIELDS:
        assert FM.bits_equal(np.ascontiguousarray(got[fld][m]), np.ascontiguousarray(base[fld][m])), (label, fld)


# ---- 1. the plain surface, bit for bit ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CR.SET_NAMES)
@pytest.mark.parametrize("aa", [0.0, AA], ids=["plain", "antialias"])
@pytest.mark.parametrize("cam", ["persp", "oblique"])
def test_plain_surface_is_bit_exact(renderer, cam, aa, name):
    g, cu, su, proj, unf = FM.view("case_plane", cam)
    FM.bind(renderer, g)
    hid, _, _ = CR.expected("case_plane", cam, PLANE[name])
    base, t0 = FM.varyings(renderer, cu, su, projection=proj, antialias=aa, clip_volumes=[])
    got, t = FM.varyings(renderer, cu, su, projection=proj, antialias=aa, clip_volumes=PLANE[name])
    assert got.shape == base.shape == hid.shape == (510,)
    vis0 = base["visible"] == 1
    if aa == 0.0:
        assert np.array_equal(vis0, unf["visible"] == 1)
    want = vis0 & ~hid
    assert np.array_equal(got["visible"] == 1, want), (cam, aa, name)          # no mask
    _same_fields(got, base, want, (cam, aa, name))
    pairs = CR.pair_counts("case_plane", cam, AAR.aa_s(AA_VALUE, su.splat_scale) if aa else 0.0)
    n_vis, n_pairs = int(want.sum()), int(pairs[want].sum())
    print(f"{cam} aa={aa:.3f} {name}: {int(vis0.sum())} visible, {n_vis} kept; pairs {t0['n_pairs']} -> {n_pairs}")
    assert (t0["n_visible"], t0["n_pairs"]) == (int(vis0.sum()), int(pairs[vis0].sum()))
    assert (t["n_visible"], t["n_pairs"]) == (n_vis, n_pairs) and 0 < n_vis < int(vis0.sum())
    # the normal instantiation (DEBUG = false, over k_cull's live table): the context keeps the set
    renderer.render(cu, su, W, Hh, projection=proj, antialias=aa)
    tn = renderer.timings()
    assert (tn["n_visible"], tn["n_pairs"]) == (n_vis, n_pairs)


# ---- 2. the surfaces ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CR.SET_NAMES)
@pytest.mark.parametrize("case,cam", [("case_hmap", "persp"), ("case_sphere", "persp"), ("case_sphere", "top")])
def test_surfaces(renderer, case, cam, name):
    g, cu, su, proj, unf = FM.view(case, cam)
    FM.bind(renderer, g)
    vols = CR.volume_sets(case)[name]
    hid, msk, _ = CR.expected(case, cam, vols)
    base, _ = FM.varyings(renderer, cu, su, projection=proj, clip_volumes=[])
    got, t = FM.varyings(renderer, cu, su, projection=proj, clip_volumes=vols)
    vis0 = base["visible"] == 1
    assert np.array_equal(vis0, unf["visible"] == 1)
    share = (msk & vis0).sum() / vis0.sum()
    print(f"{case} {cam} {name}: {int(vis0.sum())} visible, {int((hid & vis0).sum())} hidden, {int((msk & vis0).sum())} masked")
    assert share <= AR.MAX_MASKED
    want, have = vis0 & ~hid, got["visible"] == 1
    assert np.array_equal(have[~msk], want[~msk]), (case, cam, name)
    assert not (have & ~vis0).any()
    _same_fields(got, base, have, (case, cam, name))                            # everything that survives, masked or not, is exact
    assert t["n_visible"] == int(have.sum())
    pairs = CR.pair_counts(case, cam)
    assert t["n_pairs"] == int(pairs[have].sum())
    renderer.render(cu, su, W, Hh, projection=proj)
    tn = renderer.timings()
    assert (tn["n_visible"], tn["n_pairs"]) == (t["n_visible"], t["n_pairs"])


# ---- 3. known answers -----------------------------------------------------------------------------------------------------------------------
def _frame(renderer, cu, su, proj, bgc, bgd, **kw):
    out = renderer.render(cu, su, W, Hh, projection=proj, order_mode=L.GSWT_ORDER_DEPTH, bg_rgba=bgc, bg_depth=bgd, depth=True, pick=True, **kw)
    t = renderer.timings()
    return out, (t["n_visible"], t["n_pairs"])


@pytest.mark.parametrize("cam", ["persp", "oblique"])
def test_a_set_that_hides_everything_and_one_that_hides_nothing(renderer, cam):
    g, cu, su, proj, _ = FM.view("case_plane", cam)
    FM.bind(renderer, g)
    bgc, bgd = DR.bg_images(W, Hh)
    off, n_off = _frame(renderer, cu, su, proj, bgc, bgd, clip_volumes=[])
    assert n_off[0] > 0 and (off[2]["weight"] > 0).mean() > 0.3
    (img, z, pick), n = _frame(renderer, cu, su, proj, bgc, bgd, clip_volumes=PLANE["all"])
    assert n == (0, 0)
    assert FM.same(img, bgc) and FM.same(z, bgd) and not (pick["weight"] > 0).any()
    none, n = _frame(renderer, cu, su, proj, bgc, bgd, clip_volumes=PLANE["none"])
    assert n == n_off
    for a, b in zip(none, off):
        assert FM.same(a, b)


@pytest.mark.parametrize("h", [1.0, -1.0], ids=["above", "below"])
def test_a_half_space_below_h_is_clip_by_z(renderer, h):
    """The half-space z <= h as a cut volume against use_clip = 1, clip_height = h on the plain surface.  There the clip test's mapped_z
    is the SURFACE's height under the splat, 0 for every splat (map_height_surface / map_sphere_surface set it; without a surface it
    stays 0), not the centre's z, which spreads over -0.47 .. 0.43: the two frames are the same frame exactly for the h beyond that
    spread -- above it both hide everything, below it neither hides anything -- and both are checked.  In between they differ by
    definition; what the half-space does there is test_plain_surface_is_bit_exact's "half" set.  No mapped_z equals either h."""
    g, cu, su, proj, _ = FM.view("case_plane", "persp")
    FM.bind(renderer, g)
    z = SR.centres_f32(su, g["pp"].tex, g["draws"])[2]
    assert (z < F32(h)).all() or (z > F32(h)).all()
    su_clip = orc.Scene160.from_buffer_copy(bytes(su))
    su_clip.use_clip, su_clip.clip_height = 1, h
    bgc, bgd = DR.bg_images(W, Hh)
    want, n_want = _frame(renderer, cu, su_clip, proj, bgc, bgd, clip_volumes=[])
    cut = [V.half_space((0.0, 0.0, h), (0.0, 0.0, 1.0))]
    assert CR.params(cut)[0]["M"][2].tolist() == [0.0, 0.0, 1.0, -h]
    got, n_got = _frame(renderer, cu, su, proj, bgc, bgd, clip_volumes=cut)
    off, n_off = _frame(renderer, cu, su, proj, bgc, bgd, clip_volumes=[])
    assert n_got == n_want == ((0, 0) if h > 0 else n_off) and n_off[0] > 0
    for a, b in zip(got, want):
        assert FM.same(a, b)
    a, _ = FM.varyings(renderer, cu, su, projection=proj, clip_volumes=cut)
    b, _ = FM.varyings(renderer, cu, su_clip, projection=proj, clip_volumes=[])
    assert np.array_equal(a["visible"], b["visible"])
    _same_fields(a, b, a["visible"] == 1, "clip by z")


# ---- 4. image, depth and pick over the surviving records ------------------------------------------------------------------------------------
def _image_case(renderer, cam, order_mode, bg, splat_scale, name="eight"):
    c = FM.image_case(renderer, cam, order_mode, bg, splat_scale, dict(clip_volumes=PLANE[name]), "clip " + name)
    hid, _, unf = CR.expected("case_plane", cam, PLANE[name])
    sp = c["sp"]
    assert not ((sp["visible"] == 1) & hid).any() and 0 < (sp["visible"] == 1).sum()
    off = c["again"](clip_volumes=[], depth=True, pick=True)
    assert not FM.same(c["img"], off[0]) and renderer.timings()["n_pairs"] > c["t"]["n_pairs"] > 0
    return c["t"]


@pytest.mark.parametrize("bg", [False, True], ids=["clear", "bg"])
@pytest.mark.parametrize("order_mode", [0, 1], ids=["reference", "depth"])
def test_image_depth_and_pick_match_the_references(renderer, order_mode, bg):
    _image_case(renderer, "persp", order_mode, bg, OR.SPLAT_SCALE, "cut")


def test_image_depth_and_pick_with_several_segments_per_tile(renderer):
    renderer.set_option(L.GSWT_OPT_SEGMENT, 256)
    t = _image_case(renderer, "oblique", L.GSWT_ORDER_DEPTH, True, OR.SPLAT_SCALE_DENSE, "cut")
    lens = renderer.read_ranges().astype(np.int64)
    assert ((lens[:, 1] - lens[:, 0]) > 256).sum() >= 1 and t["n_pairs"] > 256


# ---- 5. the same bytes every way ----------------------------------------------------------------------------------------------------------------
STATES = {"off": [], "cut": PLANE["cut"], "keep": PLANE["keep"], "eight": PLANE["eight"]}
MODE = FM.Mode({name: (None, dict(clip_volumes=vols)) for name, vols in STATES.items()}, lambda r, name: r.set_clip_volumes(STATES[name]), on="eight")


@pytest.fixture()
def plain(renderer):
    """The plane case bound under its perspective camera, depth order over a background, and the plain synchronous frames (colour,
    depth, pick) under each set of STATES."""
    g, cu, su, proj, _ = FM.view("case_plane", "persp")
    s = FM.plain_frames(renderer, MODE, g, su, cu)
    renderer.set_clip_volumes(None)
    pairs = s["pairs"]
    assert len({bytes(np.ascontiguousarray(f[0])) for f in s["frames"].values()}) == len(STATES)
    assert all(0 < pairs[k] < pairs["off"] for k in ("cut", "keep", "eight"))
    return s


def test_graph_replay_with_alternating_sets(renderer, plain):
    seq1 = ["off", "eight", "cut", "eight", "off", "keep"]
    seq2 = ["eight", "off", "keep", "cut", "off", "eight"]
    _, rebuilds, _ = FM.check_graph_replay(renderer, plain, MODE, seq1, seq2)
    assert rebuilds >= 4                                   # on <-> off is another k_project instantiation: the slot's graph is rebuilt


def test_async_frames_in_flight_keep_their_set(renderer, plain):
    assert renderer.frame_slots() >= 4
    FM.check_in_flight(renderer, plain, MODE, ["eight", "off", "keep", "cut"], waves=4, then="keep")
    FM.check_in_flight(renderer, plain, MODE, ["cut", "eight", "eight", "keep"], waves=4, then="off", what="async, then off")


@pytest.mark.parametrize("opt", [L.GSWT_OPT_NO_CHUNK_CULL], ids=["no_chunk_cull"])
def test_compositor_and_cull_variants(renderer, plain, opt):
    FM.check_with_option_on(renderer, plain, MODE, opt, [MODE.on])


def test_pair_buffer_overflow_rerun_keeps_the_set(renderer, plain):
    FM.check_overflow_rerun(renderer, plain, MODE, MODE.on, then="cut")


def test_output_formats(renderer, plain):
    FM.check_output_formats(renderer, plain, MODE, [MODE.on])


@pytest.mark.parametrize("n", [2, 3])
def test_row_shards_tile_the_frame(renderer, plain, n):
    FM.check_row_shards(renderer, plain, MODE, n, [MODE.on])


@pytest.mark.parametrize("n", [2, 3, 5])
def test_column_bands_unite_to_the_frame(renderer, plain, n):
    FM.check_column_bands(renderer, plain, MODE, n, [MODE.on])


def _null(r):
    r.set_clip_volumes(PLANE["cut"])
    assert r._lib.gswt_set_clip_volumes(r._h, None, 0) == L.GSWT_OK
    return {}


def _n_zero(r):
    r.set_clip_volumes(PLANE["cut"])
    buf = (C.c_char * 64).from_buffer_copy(PLANE["cut"][0].pack())
    assert r._lib.gswt_set_clip_volumes(r._h, buf, 0) == L.GSWT_OK
    return {}


def test_off_is_untouched():
    """A context on which no volume was ever set; then NULL, n = 0 and an empty Python list: byte-identical colour, depth, pick and counts
    every time, and the vertex stage is still the oracle's, bit for bit."""
    FM.check_off_is_untouched("persp", dict(clip_volumes=PLANE["eight"]), [("NULL", _null), ("n = 0", _n_zero), ("empty list", lambda r: dict(clip_volumes=[]))])


def test_sequence_v2_is_refused_at_submit(renderer, plain):
    FM.check_v2_refused_at_submit(renderer, plain, MODE, ("cut", "eight"), (b"GSWT_OPT_STRICT_VS", b"gswt_set_clip_volumes"))


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------------------------------
def test_refused_sets_leave_the_set_in_force(renderer, plain):
    lib, h = renderer._lib, renderer._h
    renderer.set_clip_volumes(PLANE["eight"])
    good = np.frombuffer(CL.pack(PLANE["eight"]), np.uint32).reshape(8, 16).copy()

    def refused(rec, n, needles):
        rec = np.ascontiguousarray(rec)
        assert lib.gswt_set_clip_volumes(h, rec.ctypes.data_as(C.c_void_p), n) == L.GSWT_ERR_BAD_ARG, needles
        assert all(x in lib.gswt_last_error(h) for x in needles), (needles, lib.gswt_last_error(h))

    assert lib.gswt_set_clip_volumes(h, None, 3) == L.GSWT_ERR_BAD_ARG and b"NULL" in lib.gswt_last_error(h)
    nine = np.concatenate([good, good[:1]])
    refused(nine, 9, (b"n = 9", b"GSWT_MAX_CLIP_VOLUMES"))
    for k, (col, val, needles) in enumerate([(12, 3, (b"shape",)), (13, 4, (b"flags",)), (13, 0x80000001, (b"flags",)), (14, 1, (b"reserved",)),
                                             (15, 7, (b"reserved",))]):
        bad = good.copy()
        bad[5, col] = val
        refused(bad, 8, (b"v[5]",) + needles)
    for value in (np.inf, -np.inf, np.nan):
        bad = good.copy()
        bad[2].view(F32)[7] = value
        refused(bad, 8, (b"v[2]", b"world_to_unit[7]", b"finite"))
    half = int(np.flatnonzero(good[:, 12] == CL.HALFSPACE)[0])
    bad = good.copy()
    bad[half].view(F32)[10] = np.nan                          # a half-space's row 2 is read ...
    refused(bad, 8, (f"v[{half}]".encode(), b"world_to_unit[10]"))
    with pytest.raises(GSWTError):
        renderer.set_clip_volumes(bad.tobytes())
    with pytest.raises(ValueError):
        renderer.set_clip_volumes(b"\0" * 65)
    with pytest.raises(ValueError):
        renderer.set_clip_volumes(PLANE["eight"] + PLANE["cut"])
    got = renderer.render(plain["cu"], plain["su"], W, Hh, depth=True, pick=True, **plain["kw"])
    FM.assert_frames([got], ["eight"], plain, "after refused sets")
    ok = good.copy()
    ok[half].view(F32)[:8] = np.nan                           # ... its rows 0 and 1 are not, whatever they hold
    assert lib.gswt_set_clip_volumes(h, ok.ctypes.data_as(C.c_void_p), 8) == L.GSWT_OK
    got = renderer.render(plain["cu"], plain["su"], W, Hh, depth=True, pick=True, **plain["kw"])
    FM.assert_frames([got], ["eight"], plain, "junk in a half-space's unread rows")


# ---- 7. stacked with the other modes ------------------------------------------------------------------------------------------------------------------
def _stack_points(case, cam):
    P = MS.Point
    return [P(case, cam, aa=True), P(case, cam, atm="both"), P(case, cam, sty=True), P(case, cam, shd=True), MS.corner(case, cam)]


STACK = _stack_points("case_plane", "persp") + _stack_points("case_sphere", "top")


@pytest.mark.parametrize("pt", STACK, ids=[pt.id for pt in STACK])
def test_stacked_with_the_other_modes(renderer, pt):
    """mode_stack_ref's composed records with the hidden splats removed; on the Sphere surface a splat inside the margins' mask may go either way."""
    g, cu, su, proj, _ = FM.view(pt.case, pt.cam)
    FM.bind(renderer, g)
    vols = CR.volume_sets(pt.case)["eight"]
    hid, msk, _ = CR.expected(pt.case, pt.cam, vols)
    st = dict(MS.stack(pt))
    got, t = FM.varyings(renderer, cu, su, projection=proj, clip_volumes=vols, **MS.render_kw(pt))
    open_ = msk & st["visible"]
    assert open_.sum() <= AR.MAX_MASKED * st["visible"].sum() and (pt.case != "case_plane" or not open_.any())
    want = st["visible"] & ~hid
    st["visible"] = np.where(open_, got["visible"] == 1, want)
    assert 0 < want.sum() < MS.stack(pt)["visible"].sum()
    print(f"{pt.id} + clip: {int(MS.stack(pt)['visible'].sum())} -> {int(want.sum())} visible, {int(open_.sum())} inside the margins")
    print(MS.check_records(got, t["n_visible"], st))


# ---- 8. the shadow loop ---------------------------------------------------------------------------------------------------------------------------------
def test_a_cut_away_occluder_casts_no_shadow(renderer):
    """Two opaque splats one above the other on the plain surface; the sun looks straight down and its depth frame, rendered by the
    library, is the shadow map.  Rendered with a cut box around the upper splat, the map no longer holds it: the lower splat, which
    tests/shadow_ref.py shades under the full map, is lit -- its record is the unshadowed one bit for bit."""
    halves = S.diag_halves((0.3, 0.45, 0.3))
    scene = S.raw_scene([((2.0, 2.0, 1.0), halves, (200, 120, 48, 255)), ((2.0, 2.0, -1.0), halves, (200, 120, 48, 255))])
    _, pd = scene.draws(map_index=7)
    renderer.configure(None)
    scene.upload(renderer)
    renderer.set_draws(pd)
    su = orc.scene_uniforms(num_lod=1)
    sun = ortho.top_down((2.0, 2.0), 2.0, 3.0, -3.0, 64, 64)
    cut = [V.box((2.0, 2.0, 1.0), (1.0, 1.0, 0.5), CR.rot_z(30.0))]
    centres = [np.array([2.0, 2.0], F32), np.array([2.0, 2.0], F32), np.array([1.0, -1.0], F32)]
    assert CR.hidden(CR.params(cut), *centres).tolist() == [True, False]
    sun_map = lambda vols: renderer.render(sun.uniforms(), su, 64, 64, projection=ORTHO, order_mode=L.GSWT_ORDER_DEPTH, depth=True, clip_volumes=vols)[1]
    z_full, z_cut = sun_map([]), sun_map(cut)
    assert (z_cut >= z_full).all() and (z_cut > z_full).any() and z_cut.max() == 1.0
    cu = ortho.top_down((2.0, 2.0), 3.0, 5.0, -5.0, W, Hh).uniforms()
    base, _ = FM.varyings(renderer, cu, su, projection=ORTHO, shadow=shadows.OFF, clip_volumes=[])
    assert (base["visible"] == 1).all()
    shade = dict(bias=0.02, strength=0.6, shade_color=(0.0, 0.0, 0.0))
    for label, zmap, lower_shaded in (("full map", z_full, True), ("map with the cut", z_cut, False)):
        m = shadows.from_ortho_camera(sun, zmap, **shade)
        p = SR.params(m)
        sh = SR.lookup_f32(centres, p)[0]
        assert sh[0] == 0 and (sh[1] != 0) == lower_shaded, (label, sh)
        got, tm = FM.varyings(renderer, cu, su, projection=ORTHO, shadow=m, clip_volumes=[])
        assert tm["n_visible"] == 2 and np.array_equal(got["visible"], base["visible"])
        want = SR.shaded_rgb_f32(base["rgba"][:, :3], sh, p)
        assert FM.bits_equal(np.ascontiguousarray(got["rgba"][:, :3]), want), label
        for fld in ("ndc", "depth", "major", "minor"):
            assert FM.bits_equal(np.ascontiguousarray(got[fld]), np.ascontiguousarray(base[fld])), (label, fld)
        if not lower_shaded:
            _same_fields(got, base, np.array([True, True]), label)
    # ... and the main frame under the same cut shows the lower splat alone, lit
    got, tm = FM.varyings(renderer, cu, su, projection=ORTHO, shadow=shadows.from_ortho_camera(sun, z_cut, **shade), clip_volumes=cut)
    assert list(got["visible"]) == [0, 1] and tm["n_visible"] == 1
    _same_fields(got, base, np.array([False, True]), "clipped frame under its own sun map")
