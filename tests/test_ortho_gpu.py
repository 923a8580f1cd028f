"""Orthographic frames (GSWT_OPT_PROJECTION = 1, include/gswt_hip.h) on the GPU.  Frames are 72 x 40: 5 x 3 screen tiles, partial on
the right and bottom edges.  The scenes are the golden cases with the draws of their own perspective sort event, seen by a top-down
and an oblique orthographic camera (tests/ortho_ref.py).

The vertex stage against the float32 restatement bit for bit; the surface mappings against the oracle on the outputs the Jacobian
does not touch; image, depth and pick against the CPU references over the GPU's own projected records; a known-answer height field;
the same bits through graphs, frames in flight, the chunk cull off, output formats and row shards; the refusals; and the
perspective path untouched by switching the option on and off."""
import numpy as np
import pytest

from gswt_renderer_amd import _lib as L
from gswt_renderer_amd import ortho
from gswt_renderer_amd.renderer import PICK_NONE, GSWTError
from oracle import gswt_oracle as orc
from tests import frame_modes as FM
from tests import ortho_ref as OR
from tests import special_splats as S

pytestmark = pytest.mark.gpu
W, Hh = OR.W, OR.H
ORTHO, PERSP = L.GSWT_PROJECTION_ORTHO, L.GSWT_PROJECTION_PERSPECTIVE


@pytest.fixture(autouse=True)
def _defaults(renderer):
    yield
    FM.restore_defaults(renderer)


def _varyings(renderer, cu, su, projection=ORTHO):
    return FM.varyings(renderer, cu, su, projection=projection)[0]


# ---- 1. the vertex stage, bit for bit ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", OR.CAMERAS)
def test_vertex_stage_is_bit_exact(renderer, which):
    g = OR.golden()
    FM.bind(renderer, g)
    cu, su, want = OR.plane_records(which)
    cam = FM.ortho_cam(which, g)
    assert bytes(cam.uniforms()) == bytes(cu)
    got = _varyings(renderer, cam.uniforms(), su)
    assert got.shape == want.shape
    assert np.array_equal(got["visible"], want["visible"])
    vis = want["visible"] == 1
    assert vis.sum() > 300
    for fld in ("ndc", "depth", "major", "minor", "rgba"):
        assert FM.bits_equal(got[fld][vis], want[fld][vis]), fld


# ---- 2. the surface mappings inside the FULL x ORTHO instantiations ------------------------------------------------------------------
@pytest.mark.parametrize("which", OR.CAMERAS)
@pytest.mark.parametrize("name", ["case_hmap", "case_sphere"])
def test_surfaces_agree_with_the_oracle_where_the_jacobian_plays_no_part(renderer, name, which):
    g = OR.golden(name)
    FM.bind(renderer, g)
    su = OR.scene_of(g)
    cu = FM.ortho_cam(which, g, name).uniforms()
    got = _varyings(renderer, cu, su)
    want = orc.project_draws(orc.Camera176.from_buffer_copy(bytes(cu)), su, g["pp"].tex, g["draws"], height_map=g["hm"])
    assert got.shape == want.shape
    both = (got["visible"] == 1) & (want["visible"] == 1)
    assert both.sum() > 150 and not ((got["visible"] == 1) & (want["visible"] == 0)).any()
    for fld in ("ndc", "depth", "rgba"):
        assert FM.bits_equal(got[fld][both], want[fld][both]), fld
    maj, mnr = got["major"][got["visible"] == 1].astype(np.float64), got["minor"][got["visible"] == 1].astype(np.float64)
    assert np.isfinite(maj).all() and np.isfinite(mnr).all()
    assert (np.hypot(maj[:, 0], maj[:, 1]) >= np.hypot(mnr[:, 0], mnr[:, 1])).all()


@pytest.mark.parametrize("which", OR.CAMERAS)
@pytest.mark.parametrize("name", ["case_hmap", "case_sphere"])
def test_surfaces_equal_the_oracle_bit_for_bit(renderer, name, which):
    """The same frames against the oracle's own orthographic stage (oracle.frame_mode(ortho=1); tests/test_pair_list_modes_cpu.py pins it to
    the float32 restatement on the plane): every output, the axes included, bit for bit, and the same `visible`."""
    g = OR.golden(name)
    FM.bind(renderer, g)
    su = OR.scene_of(g)
    cu = FM.ortho_cam(which, g, name).uniforms()
    got = _varyings(renderer, cu, su)
    block = orc.Camera176.from_buffer_copy(bytes(cu))
    with orc.frame_mode(ortho=1):
        want = orc.project_draws(block, su, g["pp"].tex, g["draws"], height_map=g["hm"])
        rects = orc.pair_rects(block, su, g["pp"].tex, g["draws"], W, Hh, height_map=g["hm"])
    assert got.shape == want.shape
    assert np.array_equal(got["visible"], rects["visible"])           # (the product's `visible`: the fragment setup passed too)
    vis = rects["visible"] == 1
    assert vis.sum() > 150
    for fld in ("ndc", "depth", "major", "minor", "rgba"):
        assert FM.bits_equal(got[fld][vis], want[fld][vis]), fld


# ---- 3. image, depth and pick against the CPU references over the GPU's own records --------------------------------------------------
def _image_case(renderer, which, order_mode, bg, splat_scale):
    return FM.image_case(renderer, which, order_mode, bg, splat_scale, {}, "ortho", min_cover=0.5)["t"]


@pytest.mark.parametrize("bg", [False, True], ids=["clear", "bg"])
@pytest.mark.parametrize("order_mode", [0, 1], ids=["reference", "depth"])
@pytest.mark.parametrize("which", OR.CAMERAS)
def test_image_depth_and_pick_match_the_references(renderer, which, order_mode, bg):
    _image_case(renderer, which, order_mode, bg, OR.SPLAT_SCALE)


def test_image_depth_and_pick_with_several_segments_per_tile(renderer):
    renderer.set_option(L.GSWT_OPT_SEGMENT, 256)
    t = _image_case(renderer, "oblique", L.GSWT_ORDER_DEPTH, True, OR.SPLAT_SCALE_DENSE)
    assert t["n_pairs"] > 256 * t["n_tiles"] / 4          # many tiles have several segments
    lens = renderer.read_ranges().astype(np.int64)
    assert ((lens[:, 1] - lens[:, 0]) > 256).sum() >= 2


# ---- 4. a known-answer height field --------------------------------------------------------------------------------------------------
def test_known_answer_height_field(renderer):
    """Five opaque splats at known heights under a top_down camera of 4 px per world unit: the pick image's depth at each splat's centre
    pixel, through height_from_depth, is the splat's height.

    The bound, from the binary32 chain of that depth (all other terms of the three expressions are products with exact zeros):
      view z   cv.z = fl(z - z_top)                      1 rounding  (V[10] = 1, V[14] = -z_top exactly: z_top is a binary32 number)
      clip z   q.z  = fl(GP[10] * cv.z),  GP[10] = 0.5 fl(-2 / range)    2 roundings  (GP[14] = fl(0.5 * -1 + 0.5) = 0, q.w = 1 exactly)
      depth    q.z / q.w = q.z                           exact
    so depth = d (1 + e)^3 with |e| <= u = 2^-24 and d = (z_top - z) / range <= 1 the largest intermediate: |depth - d| <= 3 u (1 + 2 u) d,
    and the height, z_top - depth * range in binary64, is within 3 u (1 + 2 u) d range of z (+ 2^-50 for the binary64 steps)."""
    # (The splats are longer in y than in x.  vs_main takes the major axis' direction from (cov01, lambda1 - cov00), gswt.wgsl:245-250, which is
    # 0 / 0 for an exactly diagonal cov2d with cov00 >= cov11: such a splat draws nothing, in the shader as here.  A perspective view meets that
    # case only on the view axis; a straight-down orthographic one meets it for every exactly axis-aligned covariance.)
    z_top, z_bottom = 3.0, -1.0
    cam = ortho.top_down((0.0, 0.0), 5.0, z_top, z_bottom, W, Hh)
    assert cam.focal() == (4.0, 4.0)
    px = [(8, 6, 0.5), (30, 10, 1.25), (60, 8, -0.75), (20, 30, 2.5), (50, 31, 0.0)]          # (pixel x, pixel y, height)
    rows = [((( x + 0.5) / 4.0 - 9.0, 5.0 - (y + 0.5) / 4.0, z), S.diag_halves((0.2, 0.3, 0.25)), (200, 100 + 20 * k, 50, 255))
            for k, (x, y, z) in enumerate(px)]
    scene = S.raw_scene(rows)
    _, pd = scene.draws(map_index=7)
    renderer.configure(None)
    scene.upload(renderer)
    renderer.set_draws(pd)
    su = orc.scene_uniforms(num_lod=1)
    for order_mode in (0, 1):
        img, z, pick = renderer.render(cam.uniforms(), su, W, Hh, projection=ORTHO, depth=True, pick=True, order_mode=order_mode)
        assert renderer.timings()["n_visible"] == len(px)
        rng = z_top - z_bottom
        for k, (x, y, h) in enumerate(px):
            p = pick[y, x]
            assert p["map_index"] == 7 and p["entry"] == k and 1.0 - FM.TOL <= p["weight"] <= 1.0
            d = (z_top - h) / rng
            bound = 3 * OR.U * (1 + 2 * OR.U) * d * rng + 2.0 ** -50
            got = float(ortho.height_from_depth(cam, p["depth"]))
            print(f"splat {k}: height {h} from depth {p['depth']!r} -> {got!r} (bound {bound:.3e})")
            assert abs(got - h) <= bound
            assert abs(float(z[y, x]) - float(p["depth"])) <= FM.ZTOL      # an opaque splat's centre: weight 1, the depth image holds the same value
        free = pick["weight"] == 0
        assert free.sum() > 0.9 * W * Hh and (~free).sum() >= len(px)
        assert (pick["depth"][free] == 1.0).all() and (z[free] == 1.0).all()
        assert (pick["map_index"][free] == PICK_NONE).all() and (pick["entry"][free] == PICK_NONE).all()
        assert (ortho.height_from_depth(cam, pick["depth"][free]) == z_bottom).all()


# ---- 5. the same bits every way ------------------------------------------------------------------------------------------------------
def _set_projection(renderer, name):
    renderer.set_option(L.GSWT_OPT_PROJECTION, PERSP if name == "persp" else ORTHO)


def _opposite(wave):
    """The state whose projection is not that of the wave's first frame: the option as it stands must not reach the frames submitted."""
    return "persp" if wave[0] != "persp" else "top"


@pytest.fixture()
def plain(renderer):
    """The plane case bound, and the plain synchronous frames (colour, depth, pick) of the two orthographic cameras and the case's
    perspective camera, depth order, over a background; under "mode" the three cameras as states."""
    g = OR.golden()
    mode = FM.Mode({"top": (FM.ortho_cam("top", g).uniforms(), dict(projection=ORTHO)), "oblique": (FM.ortho_cam("oblique", g).uniforms(), dict(projection=ORTHO)),
                    "persp": (FM.persp_cam(g), dict(projection=PERSP))}, _set_projection)
    s = FM.plain_frames(renderer, mode, g, OR.scene_of(g))
    renderer.set_option(L.GSWT_OPT_PROJECTION, PERSP)
    frames = s["frames"]
    assert not FM.same(frames["top"][0], frames["oblique"][0]) and not FM.same(frames["top"][0], frames["persp"][0])
    for f in frames.values():
        assert (f[2]["weight"] > 0).mean() > 0.3
    return dict(s, mode=mode)


def test_graph_replay_with_alternating_projections(renderer, plain):
    # one frame at a time: slot 0 alternates; then two in flight: slots 0 and 1 each alternate from wave to wave
    seq1 = ["top", "persp", "oblique", "persp", "top"]
    seq2 = ["top", "persp", "persp", "oblique", "top", "persp"]
    _, rebuilds, _ = FM.check_graph_replay(renderer, plain, plain["mode"], seq1, seq2, then=_opposite)
    assert rebuilds >= 4                                    # another k_project instantiation: the slot's graph is rebuilt


def test_async_frames_in_flight_keep_their_projection(renderer, plain):
    slots = renderer.frame_slots()
    seq = [("top", "persp", "oblique", "persp")[k % 4] for k in range(slots)]
    FM.check_in_flight(renderer, plain, plain["mode"], seq, waves=slots, then=_opposite)


@pytest.mark.parametrize("opt", [L.GSWT_OPT_NO_CHUNK_CULL], ids=["no_chunk_cull"])
def test_cull_and_compositor_variants(renderer, plain, opt):
    FM.check_with_option_on(renderer, plain, plain["mode"], opt, ("top", "oblique"))


def test_output_formats(renderer, plain):
    FM.check_output_formats(renderer, plain, plain["mode"], ("top", "oblique"), bgra=True)


def test_two_row_shards_tile_the_frame(renderer, plain):
    FM.check_row_shards(renderer, plain, plain["mode"], 2, ("top", "oblique"))


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals(renderer, plain):
    lib, h = renderer._lib, renderer._h
    su, mode = plain["su"], plain["mode"]
    good, persp = mode.states["top"][0], mode.states["persp"][0]

    def block(edit=None, base=good):
        cu = L.CameraUniforms.from_buffer_copy(bytes(base))
        if edit:
            edit(cu)
        return cu

    # option values
    for bad in (2, -1):
        assert lib.gswt_set_option(h, L.GSWT_OPT_PROJECTION, bad) == L.GSWT_ERR_BAD_ARG
        assert b"GSWT_OPT_PROJECTION" in lib.gswt_last_error(h)
    with pytest.raises(GSWTError):
        renderer.render(good, su, W, Hh, projection=2)

    def setfocal(k, v):
        def f(cu):
            cu.focal[k] = v
        return f

    cases = [("perspective matrix", block(base=persp), {}, None, b"affine"),
             ("focal 0", block(setfocal(0, 0.0)), {}, None, b"focal"),
             ("focal NaN", block(setfocal(1, float("nan"))), {}, None, b"focal"),
             ("focal inf", block(setfocal(0, float("inf"))), {}, None, b"focal"),
             ("sequence v2", block(), {}, dict(STRICT_VS=0), b"GSWT_OPT_STRICT_VS"),
             ("column shards", block(), dict(shard_index=1, shard_count=2, shard_mode=L.GSWT_SHARD_COLUMNS), None, b"column")]
    refused, _ = FM.refusal_probe(renderer)
    renderer.set_option(L.GSWT_OPT_PROJECTION, ORTHO)
    for what, cu, cfg_kw, opt, word in cases:
        FM.check_refused(renderer, refused, *FM.frame_blocks(cu, su, **cfg_kw), (word,), what, opt=opt)
        # the next valid frame renders
        FM.assert_frames([FM.render_state(renderer, plain, mode, "top")], ["top"], plain, "after " + what)
    # row shards are not refused, and the perspective path takes its usual matrix with the option off
    renderer.render(good, su, W, Hh, projection=ORTHO, shard=(0, 2))
    renderer.render(persp, su, W, Hh, projection=PERSP, shard=(1, 2, "cols"))


# ---- 7. perspective is untouched --------------------------------------------------------------------------------------------------------
def test_perspective_untouched_by_the_switch(renderer):
    g = OR.golden()
    FM.bind(renderer, g)
    su, cu = OR.scene_of(g), FM.persp_cam(g)
    before = renderer.render(cu, su, W, Hh, depth=True, pick=True)
    v_before = _varyings(renderer, cu, su, projection=PERSP)
    renderer.render(FM.ortho_cam("top", g).uniforms(), su, W, Hh, projection=ORTHO)
    renderer.set_option(L.GSWT_OPT_PROJECTION, PERSP)
    after = renderer.render(cu, su, W, Hh, depth=True, pick=True)           # (no projection argument: the context is left as it is)
    for a, b in zip(before, after):
        assert FM.same(a, b)
    assert FM.same(v_before, _varyings(renderer, cu, su, projection=PERSP))
    assert (before[2]["weight"] > 0).mean() > 0.1
    # the perspective vertex stage still equals the oracle's
    want = orc.project_draws(orc.Camera176.from_buffer_copy(bytes(cu)), su, g["pp"].tex, g["draws"])
    vis = want["visible"] == 1
    assert np.array_equal(v_before["visible"][vis], want["visible"][vis])
    for fld in ("ndc", "depth", "major", "minor", "rgba"):
        assert FM.bits_equal(v_before[fld][vis], want[fld][vis]), fld
