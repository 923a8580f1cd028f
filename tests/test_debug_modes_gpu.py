"""The debug draw modes (draw_mode 1 .. 4) and the point-cloud radius under the frame modes, on the GPU, against tests/debug_modes_ref.py
(pinned without a GPU by tests/test_debug_modes_cpu.py).  Frames are 72 x 40 (tests/ortho_ref.py) on the golden cases with the draws of
their own perspective sort event.

What include/gswt_hip.h promises: under the atmosphere the debug colours stay and only the fade applies; under tile styles they stay and
hide and dim still apply; under the sun shadow they keep their colour word; the anti-alias filter holds for the point-cloud radius and
the debug draw modes.  A debug draw mode forces k_project's FULL form on the plain and HeightMap surfaces too, and the compositor's
float-colour form k_composite<E = 0, D, COLF = 1, OUTF, ZOUT, PICK>.

  1. the vertex stage: k_project<DEBUG, FULL = 1, STRICT = 1, ORTHO, AA, ATM, STY, SHD[, CLIP]> as its DEBUG and as its normal
     instantiation, records bit for bit -- `visible`, geometry, alpha and the three colour floats -- on all three surfaces;
  2. point clouds under every view, with the known answer of the plane's oblique camera: NaN axes, an empty frame;
  3. the float-colour compositor against tests/depth_ref.py and tests/pick_ref.py: COLF = 1 with D = 0 / 1, ZOUT = PICK = 1 and 0,
     k_combine over float partials with depth and pick;
  4. the same bytes through graphs, frames in flight, an overflow re-run, the chunk cull off, the 8-bit and video stores and shards,
     with byte-colour and float-colour frames alternating in one slot; and plain frames untouched by debug frames in between."""
import numpy as np
import pytest

from gswt_renderer_amd import _lib as L
from gswt_renderer_amd.renderer import GSWTRenderer
from tests import clip_ref as CR
from tests import debug_modes_ref as DM
from tests import depth_ref as DR
from tests import frame_modes as FM
from tests import mode_stack_ref as MS
from tests import ortho_ref as OR
from tests import yuv_ref as YUV

pytestmark = pytest.mark.gpu
W, Hh = OR.W, OR.H
P = MS.Point


@pytest.fixture(autouse=True)
def _defaults(renderer):
    """FM.restore_defaults knows neither the clip volumes nor the shadow map: the shared context goes back without them as well."""
    yield
    renderer.set_clip_volumes(None)
    renderer.set_shadow_map(None)
    FM.restore_defaults(renderer)


def _ids(cases):
    return [f"{pt.id}-dm{dm}" + (f"-r{radius}" if radius else "") for pt, dm, radius in cases]


def _vertex_case(renderer, pt, dm, radius=0.0, vols=None):
    """The DEBUG_VARYINGS frame's records against DM.expected, then the normal frame (the DEBUG = false instantiation over k_cull's live
    table; the context keeps the modes): the same n_visible and n_pairs.  Returns the debug frame's timings and what the frames need."""
    g, cu, su, proj, _ = FM.view(pt.case, pt.cam)
    FM.bind(renderer, g)
    su = DM.scene(su, dm, radius)
    st = DM.expected(pt, dm, radius, vols)
    got, t = FM.varyings(renderer, cu, su, projection=proj, clip_volumes=vols if vols is not None else [], **MS.render_kw(pt))
    print(f"draw_mode {dm} radius {radius}: " + DM.check_records(got, t["n_visible"], st))
    renderer.render(cu, su, W, Hh, projection=proj)
    tn = renderer.timings()
    assert (tn["n_visible"], tn["n_pairs"]) == (t["n_visible"], t["n_pairs"]), pt.id
    return t, st, (cu, su, proj)


# ---- 1. the vertex stage --------------------------------------------------------------------------------------------------------------------
LATTICE = (MS.square("case_plane", "persp") + MS.square("case_plane", "oblique") + MS.square("case_sphere", "persp") + MS.square("case_sphere", "top")
           + MS.pairs_and_corner("case_hmap", "persp"))
ENDS = [pt for case, cam in DM.VIEWS for pt in (P(case, cam), MS.corner(case, cam))]
VERTEX = [(pt, dm, 0.0) for dm in (1, 4) for pt in LATTICE] + [(pt, dm, 0.0) for dm in (2, 3) for pt in ENDS]


@pytest.mark.parametrize("pt,dm,radius", VERTEX, ids=_ids(VERTEX))
def test_debug_colours_under_the_frame_modes(renderer, pt, dm, radius):
    t, st, _ = _vertex_case(renderer, pt, dm)
    assert t["n_visible"] > 0 and t["n_pairs"] > 0


CLIPPED = [(pt, dm, 0.0) for dm in (1, 4) for case, cam in (("case_plane", "persp"), ("case_sphere", "top")) for pt in (P(case, cam), MS.corner(case, cam))]


@pytest.mark.parametrize("pt,dm,radius", CLIPPED, ids=_ids(CLIPPED))
def test_debug_colours_under_clip_volumes(renderer, pt, dm, radius):
    vols = CR.volume_sets(pt.case)["eight"]
    t, st, _ = _vertex_case(renderer, pt, dm, vols=vols)
    assert 0 < t["n_visible"] < DM.expected(pt, dm)["visible"].sum()


# ---- 2. point clouds ------------------------------------------------------------------------------------------------------------------------
CLOUDS = [(pt, dm, radius) for radius in (0.002, 0.02) for dm in (0, 3) for case, cam in DM.VIEWS
          for pt in (P(case, cam), P(case, cam, aa=True), MS.corner(case, cam))]


@pytest.mark.parametrize("pt,dm,radius", CLOUDS, ids=_ids(CLOUDS))
def test_point_clouds_under_the_frame_modes(renderer, pt, dm, radius):
    t, st, (cu, su, proj) = _vertex_case(renderer, pt, dm, radius)
    if (pt.case, pt.cam) != ("case_plane", "oblique"):
        assert t["n_visible"] > 0 and t["n_pairs"] > 0
        return
    # the known answer: every axis is NaN (tests/test_debug_modes_cpu.py), no splat is visible, the frame is its background
    assert not st["visible"].any() and (t["n_visible"], t["n_pairs"]) == (0, 0)
    bgc, bgd = DR.bg_images(W, Hh)
    img, z, pick = renderer.render(cu, su, W, Hh, projection=proj, order_mode=L.GSWT_ORDER_DEPTH, bg_rgba=bgc, bg_depth=bgd, depth=True, pick=True)
    tn = renderer.timings()
    assert (tn["n_visible"], tn["n_pairs"]) == (0, 0)
    assert FM.same(img, bgc) and FM.same(z, bgd) and not (pick["weight"] > 0).any()


# ---- 3. the float-colour compositor ---------------------------------------------------------------------------------------------------------
def _image_case(renderer, dm, cam, order_mode, bg, splat_scale=OR.SPLAT_SCALE, **kw):
    c = FM.image_case(renderer, cam, order_mode, bg, splat_scale, {}, f"draw_mode {dm}", scene=lambda su: DM.scene(su, dm), **kw)
    sp = c["sp"]
    vis = sp["visible"] == 1
    assert DM.off_grid(sp["rgba"][vis][:, :3]).any()                               # (float colours: no byte holds them)
    g, cu, su, proj, _ = FM.view("case_plane", cam, splat_scale)
    bgc, bgd = DR.bg_images(W, Hh) if bg else (None, None)
    assert not FM.same(c["img"], renderer.render(cu, su, W, Hh, projection=proj, order_mode=order_mode, bg_rgba=bgc, bg_depth=bgd))
    return c


@pytest.mark.parametrize("bg", [False, True], ids=["clear", "bg"])
@pytest.mark.parametrize("order_mode", [0, 1], ids=["reference", "depth"])
@pytest.mark.parametrize("dm", [1, 4])
def test_image_depth_and_pick_match_the_references(renderer, dm, order_mode, bg):
    _image_case(renderer, dm, "persp", order_mode, bg)


def test_image_depth_and_pick_with_several_segments_per_tile(renderer):
    """k_combine folds float-colour partials, with depth and pick."""
    renderer.set_option(L.GSWT_OPT_SEGMENT, 256)
    c = _image_case(renderer, 1, "oblique", L.GSWT_ORDER_DEPTH, True, OR.SPLAT_SCALE_DENSE)
    lens = renderer.read_ranges().astype(np.int64)
    assert ((lens[:, 1] - lens[:, 0]) > 256).sum() >= 1 and c["t"]["n_pairs"] > 256


def test_image_with_a_transmittance_threshold(renderer):
    eps = 1e-5
    _image_case(renderer, 4, "persp", L.GSWT_ORDER_DEPTH, True, transmittance_eps=eps, tol=FM.TOL + eps)


# ---- 4. the same bytes every way ------------------------------------------------------------------------------------------------------------
STATES = {"off": (0, 0.0), "tile_id": (1, 0.0), "view": (4, 0.0), "lod_points": (3, 0.02)}
DEBUG_STATES = ["tile_id", "view", "lod_points"]


def _mode(su):
    """The state lives in the scene block: nothing is set on the context."""
    return FM.Mode({name: (None, {}, DM.scene(su, dm, radius)) for name, (dm, radius) in STATES.items()}, lambda r, name: None, on="tile_id")


@pytest.fixture()
def plain(renderer):
    """The plane case bound under its perspective camera, depth order over a background, the mode and the plain synchronous frames
    (colour, depth, pick) of each of STATES."""
    g, cu, su, proj, _ = FM.view("case_plane", "persp")
    mode = _mode(su)
    s = FM.plain_frames(renderer, mode, g, su, cu)
    s["mode"] = mode
    assert len({bytes(np.ascontiguousarray(f[0])) for f in s["frames"].values()}) == len(STATES)
    assert s["pairs"]["off"] == s["pairs"]["tile_id"] == s["pairs"]["view"] != s["pairs"]["lod_points"] and s["pairs"]["lod_points"] > 0
    return s


def test_graph_replay_alternates_byte_and_float_colours(renderer, plain):
    seq1 = ["off", "tile_id", "off", "view", "lod_points", "off"]
    seq2 = ["tile_id", "off", "off", "lod_points", "view", "off"]
    _, rebuilds, _ = FM.check_graph_replay(renderer, plain, plain["mode"], seq1, seq2)
    assert rebuilds >= 4                                   # off <-> debug is another k_project and another k_composite: the slot's graph is rebuilt


def test_async_frames_in_flight_keep_their_state(renderer, plain):
    assert renderer.frame_slots() >= 4
    FM.check_in_flight(renderer, plain, plain["mode"], ["tile_id", "off", "lod_points", "view"], waves=4)
    FM.check_in_flight(renderer, plain, plain["mode"], ["off", "view", "off", "tile_id", "lod_points", "off", "off", "view"], waves=4, what="async, two waves")


def test_pair_buffer_overflow_rerun(renderer, plain):
    for name in ("tile_id", "lod_points"):
        FM.check_overflow_rerun(renderer, plain, plain["mode"], name, then="off")


def test_chunk_cull_off_changes_nothing(renderer, plain):
    FM.check_with_option_on(renderer, plain, plain["mode"], L.GSWT_OPT_NO_CHUNK_CULL, DEBUG_STATES)


def test_output_formats(renderer, plain):
    FM.check_output_formats(renderer, plain, plain["mode"], DEBUG_STATES, bgra=True)
    for name in DEBUG_STATES:
        y, cb, cr = FM.render_state(renderer, plain, plain["mode"], name, depth=False, pick=False, out_format=L.GSWT_VIDEO_I420)
        wy, wcb, wcr = YUV.i420(plain["frames"][name][0])
        assert np.array_equal(y, wy) and np.array_equal(cb, wcb) and np.array_equal(cr, wcr), name


@pytest.mark.parametrize("n", [2, 3])
def test_row_shards_tile_the_frame(renderer, plain, n):
    FM.check_row_shards(renderer, plain, plain["mode"], n, DEBUG_STATES)


@pytest.mark.parametrize("n", [2, 3, 5])
def test_column_bands_unite_to_the_frame(renderer, plain, n):
    FM.check_column_bands(renderer, plain, plain["mode"], n, DEBUG_STATES)


def test_plain_frames_are_untouched_by_debug_frames():
    """A fresh context: plain frames, then debug frames (the slot gets its float-colour buffer), then plain frames again -- colour, depth,
    pick and counts byte for byte."""
    g, cu, su, proj, unf = FM.view("case_plane", "persp")
    bgc, bgd = DR.bg_images(W, Hh)
    kws = [dict(order_mode=L.GSWT_ORDER_DEPTH, bg_rgba=bgc, bg_depth=bgd), dict(order_mode=L.GSWT_ORDER_REFERENCE)]
    r = GSWTRenderer(0)
    try:
        FM.bind(r, g)

        def plain_set():
            out = []
            for kw in kws:
                f = r.render(cu, su, W, Hh, projection=proj, depth=True, pick=True, **kw)
                t = r.timings()
                out.append((f, (t["n_visible"], t["n_pairs"])))
            return out

        before = plain_set()
        assert (before[0][0][2]["weight"] > 0).mean() > 0.3
        for dm, radius in list(STATES.values())[1:]:
            for k, kw in enumerate(kws):
                f = r.render(cu, DM.scene(su, dm, radius), W, Hh, projection=proj, depth=True, pick=True, **kw)
                assert not FM.same(f[0], before[k][0][0])
        for (fa, na), (fb, nb) in zip(before, plain_set()):
            assert na == nb
            for a, b in zip(fa, fb):
                assert FM.same(a, b)
        got, _ = FM.varyings(r, cu, su, projection=proj)
        vis = unf["visible"] == 1
        assert np.array_equal(got["visible"] == 1, vis)
        for fld in FM.FIELDS:
            assert FM.bits_equal(np.ascontiguousarray(got[fld][vis]), np.ascontiguousarray(unf[fld][vis])), fld
    finally:
        r.close()
