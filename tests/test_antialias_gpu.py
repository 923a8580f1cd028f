"""Anti-aliased splats (GSWT_OPT_ANTIALIAS, include/gswt_hip.h) on the GPU.  Frames are 72 x 40 (tests/ortho_ref.py): 5 x 3 screen tiles,
partial on the right and bottom edges; the scenes are the golden cases with the draws of their own perspective sort event.

The filtered vertex stage against tests/antialias_ref.py's float64 filter of the UNFILTERED references (the oracle's records in
perspective, tests/ortho_ref.py's under the orthographic cameras); image, depth and pick against the CPU references over the GPU's
own filtered records; a known-answer minification; the same bits through graphs, frames in flight, the chunk cull off, a
pair-buffer overflow, output formats and shards (column bands included: their cull must know the filter); the option off leaves
every output as it was; the refusals."""
import math

import numpy as np
import pytest

from gswt_renderer_amd import _lib as L
from gswt_renderer_amd import ortho
from gswt_renderer_amd.renderer import GSWTError
from oracle import gswt_oracle as orc
from tests import antialias_ref as AA
from tests import frame_modes as FM
from tests import ortho_ref as OR
from tests import special_splats as S

pytestmark = pytest.mark.gpu
W, Hh = OR.W, OR.H
ORTHO, PERSP = L.GSWT_PROJECTION_ORTHO, L.GSWT_PROJECTION_PERSPECTIVE
AA_OPT = L.GSWT_OPT_ANTIALIAS
VALUES = (102, 307, 2048)


@pytest.fixture(autouse=True)
def _defaults(renderer):
    yield
    FM.restore_defaults(renderer)


def _varyings(renderer, cu, su, projection, value):
    return FM.varyings(renderer, cu, su, projection=projection, antialias=value / 1024.0)[0]


def _check_filtered(got, unf, value, splat_scale, label):
    """The GPU's filtered records against filter_records of the unfiltered reference records; returns the number of common records."""
    want, masked, n_masked = AA.filter_records(unf, value, splat_scale)
    assert got.shape == unf.shape
    vis_u, vis_g = unf["visible"] == 1, got["visible"] == 1
    assert not (vis_u & ~vis_g).any(), label                              # the visible set can only grow
    assert n_masked <= 0.01 * vis_u.sum(), (label, n_masked)
    both = vis_u & vis_g
    assert FM.bits_equal(got["ndc"][both], unf["ndc"][both]) and FM.bits_equal(got["depth"][both], unf["depth"][both]), label
    assert FM.bits_equal(np.ascontiguousarray(got["rgba"][both][:, :3]), np.ascontiguousarray(unf["rgba"][both][:, :3])), label
    ok = both & ~masked
    gm, gn = got["major"][ok].astype(np.float64), got["minor"][ok].astype(np.float64)
    lm, ln = np.hypot(gm[:, 0], gm[:, 1]), np.hypot(gn[:, 0], gn[:, 1])
    rel = lambda g, w: float((np.abs(g - w) / w).max())
    e = (rel(lm, want["len_major"][ok]), rel(ln, want["len_minor"][ok]), rel(got["rgba"][ok][:, 3].astype(np.float64), want["alpha"][ok]))
    d = max(float(np.abs(gm / lm[:, None] - want["dir_major"][ok]).max()), float(np.abs(gn / ln[:, None] - want["dir_minor"][ok]).max()))
    print(f"{label}: common {int(ok.sum())} (+{int((vis_g & ~vis_u).sum())} new, {n_masked} masked) |major| {e[0] / AA.U:.2f} |minor| {e[1] / AA.U:.2f} "
          f"alpha {e[2] / AA.U:.2f} x 2^-24 (tolerance {AA.VARYINGS_RTOL / AA.U:.0f}), directions {d / AA.U:.2f} x 2^-24")
    assert max(e) <= AA.VARYINGS_RTOL, (label, e)
    assert d <= AA.DIRECTION_ATOL, (label, d)
    # the filter did something: every common splat grew and lost opacity
    assert (lm > np.hypot(*unf["major"][ok].astype(np.float64).T)).all() and (got["rgba"][ok][:, 3] < unf["rgba"][ok][:, 3]).all(), label
    return int(ok.sum())


# ---- 1. the filtered vertex stage ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("value", VALUES)
@pytest.mark.parametrize("name,cam", [("case_plane", "persp"), ("case_plane", "top"), ("case_plane", "oblique"), ("case_hmap", "persp"),
                                      ("case_sphere", "persp")])
def test_filtered_varyings(renderer, name, cam, value):
    g, cu, su, proj, unf = FM.view(name, cam)
    FM.bind(renderer, g)
    got = _varyings(renderer, cu, su, proj, value)
    assert _check_filtered(got, unf, value, OR.SPLAT_SCALE, f"{name} {cam} value {value}") > 100


def test_s_carries_the_square_of_splat_scale(renderer):
    """The same view at splat_scale 12 and 24: each against filter_records at its own scale, and the two axes sets differ (s is four
    times as large at 12), while the unfiltered axes do not depend on splat_scale at all."""
    recs = {}
    for scale in (12.0, 24.0):
        g, cu, su, proj, unf = FM.view("case_plane", "oblique", scale)
        FM.bind(renderer, g)
        recs[scale] = _varyings(renderer, cu, su, proj, 307)
        _check_filtered(recs[scale], unf, 307, scale, f"oblique scale {scale}")
        seen = unf["visible"] == 1
        assert FM.bits_equal(_varyings(renderer, cu, su, proj, 0)["major"][seen], unf["major"][seen])
    vis = (recs[12.0]["visible"] == 1) & (recs[24.0]["visible"] == 1)
    l12, l24 = (np.hypot(*recs[k]["minor"][vis].astype(np.float64).T) for k in (12.0, 24.0))
    assert (l12 > l24).all()
    unf = FM.view("case_plane", "oblique", 12.0)[4]
    s12, s24 = float(AA.aa_s(307, 12.0)), float(AA.aa_s(307, 24.0))
    assert s12 == 4.0 * s24
    # |minor|^2 / 2 - l2 is s: the ratio of the two increments is 4 to rounding of the small differences
    l2 = 0.5 * np.hypot(*unf["minor"][vis].astype(np.float64).T) ** 2
    inc = (0.5 * l12 * l12 - l2) / (0.5 * l24 * l24 - l2)
    assert np.abs(np.median(inc) - 4.0) < 1e-3


# ---- 2. image, depth and pick over the GPU's own filtered records ------------------------------------------------------------------------
def _image_case(renderer, cam, order_mode, bg, splat_scale, value=307):
    c = FM.image_case(renderer, cam, order_mode, bg, splat_scale, dict(antialias=value / 1024.0), f"antialias {value}", min_cover=0.5)
    # ... and it is not the unfiltered frame
    off = c["again"](antialias=0.0)
    assert not FM.same(c["img"], off) and renderer.timings()["n_pairs"] <= c["t"]["n_pairs"]
    return c["t"]


@pytest.mark.parametrize("bg", [False, True], ids=["clear", "bg"])
@pytest.mark.parametrize("order_mode", [0, 1], ids=["reference", "depth"])
@pytest.mark.parametrize("cam", ["persp", "oblique"])
def test_image_depth_and_pick_match_the_references(renderer, cam, order_mode, bg):
    _image_case(renderer, cam, order_mode, bg, OR.SPLAT_SCALE)


def test_image_depth_and_pick_with_several_segments_per_tile(renderer):
    renderer.set_option(L.GSWT_OPT_SEGMENT, 256)
    t = _image_case(renderer, "oblique", L.GSWT_ORDER_DEPTH, True, OR.SPLAT_SCALE_DENSE)
    assert t["n_pairs"] > 256 * t["n_tiles"] / 4
    lens = renderer.read_ranges().astype(np.int64)
    assert ((lens[:, 1] - lens[:, 0]) > 256).sum() >= 2


def test_image_depth_and_pick_at_another_splat_scale(renderer):
    _image_case(renderer, "persp", L.GSWT_ORDER_DEPTH, True, 12.0, value=2048)


# ---- 3. known-answer minification ---------------------------------------------------------------------------------------------------------
def test_known_answer_minification(renderer):
    """Five isolated opaque splats under a top_down camera of 4 px per world unit, world variances 0.002 (x) and 0.003 (y) -- on-screen
    0.032 and 0.048 px^2, a footprint of about one pixel --, clear background, splat_scale 1.  A splat's summed output alpha over its
    neighbourhood is its integrated opacity; the analytic value is antialias_ref.analytic_mass of cov2d's eigenvalues, 16 x the stored
    (binary16) covariance entries.  With value = 512 every sum is within antialias_ref.lattice_bound (4.3 % here) of it, plus FM.TOL per
    covered pixel; with value = 0 it depends on the sub-pixel position of the centre: 4.1 x at a pixel centre, nothing at a corner.
    (The splats are longer in y than in x: tests/test_ortho_gpu.py's height-field test explains why.)"""
    z_top, z_bottom = 3.0, -1.0
    cam = ortho.top_down((0.0, 0.0), 5.0, z_top, z_bottom, W, Hh)
    assert cam.focal() == (4.0, 4.0)
    sig = (math.sqrt(0.002), math.sqrt(0.003), 0.05)
    halves = S.diag_halves(sig)
    l2, l1 = (16.0 * orc.half_to_float(halves[0]), 16.0 * orc.half_to_float(halves[3]))          # cov2d = diag(fx^2 Kxx, fy^2 Kyy), f = 4
    assert l1 > l2 > 0
    # (pixel x, pixel y, sub-pixel x, sub-pixel y): eighths of a pixel, so that every world coordinate is a binary32 number
    px = [(8, 6, 0.5, 0.5), (30, 10, 0.0, 0.0), (60, 8, 0.5, 0.375), (20, 30, 0.25, 0.25), (50, 31, 0.125, 0.75)]
    rows = [(((x + fx) / 4.0 - 9.0, 5.0 - (y + fy) / 4.0, 0.5), halves, (200, 100 + 20 * k, 50, 255)) for k, (x, y, fx, fy) in enumerate(px)]
    scene = S.raw_scene(rows)
    _, pd = scene.draws(map_index=7)
    renderer.configure(None)
    scene.upload(renderer)
    renderer.set_draws(pd)
    su = orc.scene_uniforms(num_lod=1)
    want = AA.analytic_mass(l1, l2, 1.0)
    bound = AA.lattice_bound(l1, l2, 1.0, 512)
    # the float64 reference itself: filtered within the bound everywhere, unfiltered off by more than 2 x for at least two splats
    ref_on = [AA.lattice_mass(l1, l2, math.pi / 2, x + fx, y + fy, 1.0, 512, with_count=True) for x, y, fx, fy in px]
    ref_off = [AA.lattice_mass(l1, l2, math.pi / 2, x + fx, y + fy, 1.0, 0) for x, y, fx, fy in px]
    assert all(abs(m / want - 1.0) <= bound for m, _ in ref_on)
    assert sum(1 for m in ref_off if not 0.5 <= m / want <= 2.0) >= 2
    R = 5                                                                    # the filtered footprint reaches 2.2 px
    sums = {}
    for value in (512, 0):
        img = renderer.render(cam.uniforms(), su, W, Hh, projection=ORTHO, antialias=value / 1024.0)
        a = img[..., 3].astype(np.float64)
        got = []
        mask = np.zeros((Hh, W), bool)
        for x, y, _, _ in px:
            sl = (slice(max(0, y - R), y + R + 1), slice(max(0, x - R), x + R + 1))
            got.append((float(a[sl].sum()), int((a[sl] > 0).sum())))
            mask[sl] = True
        assert not a[~mask].any()                                            # isolated: nothing outside the five neighbourhoods
        sums[value] = got
    for k, ((m, n), (rm, rn)) in enumerate(zip(sums[512], ref_on)):
        print(f"splat {k}: filtered mass {m:.6f} over {n} px (float64 lattice {rm:.6f} over {rn}), analytic {want:.6f}, ratio {m / want:.4f} "
              f"(bound {bound:.4f}); unfiltered {sums[0][k][0]:.6f} (float64 {ref_off[k]:.6f}), ratio {sums[0][k][0] / want:.3f}")
        assert n > 0 and abs(m - want) <= bound * want + FM.TOL * n
        assert abs(m - rm) <= FM.TOL * max(n, rn)
    assert sum(1 for m, _ in sums[0] if not 0.5 <= m / want <= 2.0) >= 2
    assert renderer.timings()["n_visible"] == len(px)


# ---- 4. the same bits every way ---------------------------------------------------------------------------------------------------------
def _set_value(renderer, value):
    renderer.set_option(AA_OPT, value)


MODE = FM.Mode({value: (None, dict(antialias=value / 1024.0)) for value in (0, 102, 307, 2048)}, _set_value, on=307)


@pytest.fixture()
def plain(renderer):
    """The plane case bound under its perspective camera, depth order over a background, and the plain synchronous frames (colour,
    depth, pick) at each filter value."""
    g, cu, su, proj, _ = FM.view("case_plane", "persp")
    s = FM.plain_frames(renderer, MODE, g, su, cu)
    renderer.set_option(AA_OPT, 0)
    frames, pairs = s["frames"], s["pairs"]
    assert len({bytes(np.ascontiguousarray(f[0])) for f in frames.values()}) == 4
    assert pairs[0] <= pairs[102] <= pairs[307] <= pairs[2048] and pairs[2048] > pairs[0]
    return s


def test_graph_replay_with_alternating_values(renderer, plain):
    seq1 = [0, 307, 2048, 307, 0, 307]
    seq2 = [307, 0, 2048, 307, 0, 2048]
    _, _, updates = FM.check_graph_replay(renderer, plain, MODE, seq1, seq2)
    assert updates >= len(seq1) - 1                           # a changed aa_s reaches the kernel nodes that take the frame constants


def test_async_frames_in_flight_keep_their_value(renderer, plain):
    assert renderer.frame_slots() >= 4
    seq = [307, 0, 2048, 102]                                 # four frames in flight, each with a value of its own
    FM.check_in_flight(renderer, plain, MODE, seq, waves=4, then=4096)


@pytest.mark.parametrize("opt", [L.GSWT_OPT_NO_CHUNK_CULL], ids=["no_chunk_cull"])
def test_compositor_and_cull_variants(renderer, plain, opt):
    FM.check_with_option_on(renderer, plain, MODE, opt, [MODE.on])


def test_pair_buffer_overflow_rerun_keeps_the_value(renderer, plain):
    FM.check_overflow_rerun(renderer, plain, MODE, MODE.on, then=2048)


def test_output_formats(renderer, plain):
    FM.check_output_formats(renderer, plain, MODE, [MODE.on])


# ---- 5. shards -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [2, 3])
@pytest.mark.parametrize("cam", ["persp", "top"])
def test_row_shards_tile_the_frame(renderer, cam, n):
    g, cu, su, proj, _ = FM.view("case_plane", cam)
    mode = FM.Mode({307: (None, dict(projection=proj, antialias=307 / 1024.0))}, _set_value)
    FM.check_row_shards(renderer, FM.plain_frames(renderer, mode, g, su, cu), mode, n, [307])


BAND_SPLAT_SCALE = 0.15


@pytest.mark.parametrize("n", [2, 3, 5])
@pytest.mark.parametrize("value", [2048, 4096])
def test_column_bands_unite_to_the_frame(renderer, value, n):
    """splat_scale 0.15: the filter's reach, sqrt(8 v) px whatever the scale (4 px at value 2048, 5.7 px at 4096), dominates every
    footprint, while the unfiltered bound of the band cull, 1.25 * 2 splat_scale sqrt(trace bound of lambda) + 2 px, shrinks with the
    scale to about 2.4 px here.  A cull whose bound leaves out aa_s drops cells whose splats still reach into the band.  Measured once on
    a build without that term, this scene, scales 0.05 .. 0.25: at 4096 the union of two and of five bands differs from the unsharded
    frame in one to four pixels (summed n_visible 306 against 336 with the term at two bands); at 2048 its 2 px pad still covers the
    4 px, and at scales of 0.5 and more every case passes without the term.  The 4096 cases are what pins the term."""
    g, cu, su, proj, _ = FM.view("case_plane", "persp", BAND_SPLAT_SCALE)
    FM.bind(renderer, g)
    kw = dict(order_mode=L.GSWT_ORDER_DEPTH, projection=PERSP, antialias=value / 1024.0, depth=True, pick=True)
    full = renderer.render(cu, su, W, Hh, **kw)
    n_vis = renderer.timings()["n_visible"]
    assert n_vis > 150 and (full[0][..., 3] > 0).mean() > 0.2
    bw = renderer.shard_cols_padded(W, n)
    parts, total = [], 0
    for r in range(n):
        parts.append(renderer.render(cu, su, W, Hh, shard=(r, n, "cols"), **kw))
        total += renderer.timings()["n_visible"]
        assert parts[r][0].shape == (Hh, bw, 4)
    for a, b in zip(FM.assemble_column_bands(parts, W, bw), full):
        assert FM.same(a, b), (value, n)
    print(f"{n} column bands at value {value}: visible {total} summed over the bands, {n_vis} unsharded")
    assert total < n * n_vis                                  # the band cull did engage


# ---- 6. off is untouched ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cam", ["persp", "oblique"])
def test_off_is_untouched(cam):
    """A context on which the option was never set, then frames at 307, then 0 again: byte-identical colour, depth, pick and counts,
    and the unfiltered vertex stage is still the reference's, bit for bit."""
    FM.check_off_is_untouched(cam, dict(antialias=307 / 1024.0), [("0", lambda r: dict(antialias=0.0))])


# ---- 7. refusals --------------------------------------------------------------------------------------------------------------------------
def test_refusals(renderer, plain):
    lib, h = renderer._lib, renderer._h

    def scene(splat_scale=None):
        su = orc.Scene160.from_buffer_copy(bytes(plain["su"]))
        if splat_scale is not None:
            su.splat_scale = splat_scale
        return su

    # option values: refused, and the value in force stays
    renderer.set_option(AA_OPT, 307)
    for bad in (-1, 4097):
        assert lib.gswt_set_option(h, AA_OPT, bad) == L.GSWT_ERR_BAD_ARG
        assert b"GSWT_OPT_ANTIALIAS" in lib.gswt_last_error(h)
    with pytest.raises(GSWTError):
        renderer.render(plain["cu"], plain["su"], W, Hh, antialias=4.5)
    got = renderer.render(plain["cu"], plain["su"], W, Hh, depth=True, pick=True, **plain["kw"])
    FM.assert_frames([got], [307], plain, "after refused option values")
    for ok in (1, 4096):
        assert lib.gswt_set_option(h, AA_OPT, ok) == L.GSWT_OK
    renderer.set_option(AA_OPT, 307)

    cases = [("sequence v2", scene(), dict(STRICT_VS=0), b"GSWT_OPT_STRICT_VS"),
             ("splat_scale 0", scene(0.0), None, b"splat_scale"),
             ("splat_scale inf", scene(float("inf")), None, b"splat_scale"),
             ("splat_scale NaN", scene(float("nan")), None, b"splat_scale"),
             # finite, but s = 4 v / splat_scale^2 is not a finite positive binary32 number: the square overflows (s = 0) or underflows (s = inf)
             ("splat_scale 1e20", scene(1e20), None, b"splat_scale"),
             ("splat_scale 1e-20", scene(1e-20), None, b"splat_scale")]
    refused, rendered = FM.refusal_probe(renderer)
    for what, su, opt, word in cases:
        FM.check_refused(renderer, refused, *FM.frame_blocks(plain["cu"], su), (word,), what, opt=opt)
        # the next valid frame renders
        got = renderer.render(plain["cu"], plain["su"], W, Hh, depth=True, pick=True, **plain["kw"])
        FM.assert_frames([got], [307], plain, "after " + what)
    # with the filter off neither is refused: sequence v2 runs, and a zero splat_scale draws nothing
    renderer.set_option(AA_OPT, 0)
    renderer.set_option(L.GSWT_OPT_STRICT_VS, 0)
    renderer.render(plain["cu"], plain["su"], W, Hh)
    renderer.set_option(L.GSWT_OPT_STRICT_VS, 1)
    rendered(*FM.frame_blocks(plain["cu"], scene(0.0)))


# ---- 8. through the frame harness -----------------------------------------------------------------------------------------------------------
def test_pipeline_passes_antialias_through(renderer):
    """GSWTPipeline.render(antialias=...) is GSWTRenderer.render with the pipeline's scene block: the same bits as the direct call at
    that value, another frame than the unfiltered one, and 0.0 gives the unfiltered frame back."""
    from gswt_renderer_amd import host, synth
    from gswt_renderer_amd.pipeline import GSWTPipeline
    cfg = dict(tile_map_half_wh=(3, 3), surface_type=0, lod_max_dist=20.0, tile_sort_type=3, merge_type=2)
    pipe = GSWTPipeline(synth.make_tileset(n_lod=3, n_tile=16, lod0_count=800), host.user_data(**cfg), renderer=renderer)
    pos = (4.2, 1.0, 2.0)
    cu, vp = host.camera_uniforms(pos, (5.0, 3.0, 1.5), (0, 0, 1), 45.0, 0.1, 2400.0, W, Hh)
    pipe.update(pos, vp)
    off = pipe.render(cu, W, Hh)
    pairs_off = renderer.timings()["n_pairs"]
    on = pipe.render(cu, W, Hh, antialias=307 / 1024.0)
    assert renderer.timings()["n_pairs"] > pairs_off > 0 and not FM.same(on, off)
    renderer.set_option(AA_OPT, 0)
    assert FM.same(renderer.render(cu, pipe.wang.scene_uniforms(), W, Hh, antialias=307 / 1024.0), on)
    assert FM.same(pipe.render(cu, W, Hh), on)                  # (no argument: the context keeps 307)
    assert FM.same(pipe.render(cu, W, Hh, antialias=0.0), off)
