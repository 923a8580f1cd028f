"""The atmosphere (gswt_set_atmosphere, include/gswt_hip.h) on the GPU: per-splat far fade and distance fog, and the fogged proxy ground.
Frames are 72 x 40 (tests/ortho_ref.py): 5 x 3 screen tiles, partial on the right and bottom edges; the scenes are the golden cases with
the draws of their own perspective sort event.

The faded vertex stage bit for bit against tests/atmosphere_ref.py on the plain surface (perspective and orthographic, with and without
the pixel filter) and within the derived tolerance on the HeightMap and Sphere surfaces; the fogged colour bytes against the float64
reference; known answers; image, depth and pick against the CPU references over the GPU's own records; the same bits through graphs,
frames in flight, the chunk cull off, a pair-buffer overflow, output formats and shards; the block off leaves every output as
it was; the refusals; the proxy pass; the pipeline's keyword."""
import ctypes as C
import struct

import numpy as np
import pytest

from gswt_renderer_amd import _lib as L
from gswt_renderer_amd import atmosphere as A
from gswt_renderer_amd.renderer import GSWTError
from oracle import gswt_oracle as orc
from tests import atmosphere_ref as AR
from tests import frame_modes as FM
from tests import ortho_ref as OR
from tests import proxy_raster_ref as R
from tests import special_splats as S

pytestmark = pytest.mark.gpu
W, Hh = OR.W, OR.H
F32 = np.float32
ORTHO, PERSP = L.GSWT_PROJECTION_ORTHO, L.GSWT_PROJECTION_PERSPECTIVE
FADE = (4.0, 8.0)
FOG = (0.15, 2.0, 0.9, (0.62, 0.71, 0.80))
BLOCKS = {"off": A.OFF, "fade": A.Atmosphere(fade=FADE), "fog": A.Atmosphere(fog=FOG), "both": A.Atmosphere(fade=FADE, fog=FOG),
          "near": A.Atmosphere(fade=(2.0, 6.0), fog=(0.4, 0.0, 1.0, (0.9, 0.5, 0.1)))}
AA = 307 / 1024.0


@pytest.fixture(autouse=True)
def _defaults(renderer):
    yield
    FM.restore_defaults(renderer)


def _varyings(renderer, cu, su, projection, atm, antialias=0.0):
    return FM.varyings(renderer, cu, su, projection=projection, antialias=antialias, atmosphere=atm)


def _block(cu):
    return orc.Camera176.from_buffer_copy(bytes(cu))


def _unchanged(got, base, m, fields, label):
    for fld in fields:
        assert FM.bits_equal(np.ascontiguousarray(got[fld][m]), np.ascontiguousarray(base[fld][m])), (label, fld)


# ---- 1. the fade, bit for bit --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cam", ["persp", "top", "oblique"])
def test_fade_is_bit_exact_on_the_plain_surface(renderer, cam):
    g, cu, su, proj, unf = FM.view("case_plane", cam)
    FM.bind(renderer, g)
    p = AR.params(BLOCKS["fade"])
    dist = AR.dist_f32(_block(cu).cam_pos, su, g["pp"].tex, g["draws"])
    t, fs = AR.fade_f32(dist, p)
    assert dist.shape[0] == unf.shape[0] == 510
    assert (int((t == 0).sum()), int((t == 1).sum()), int(((t > 0) & (t < 1)).sum())) == (110, 92, 308)
    for label, aa in (("fade", 0.0), ("fade + antialias", AA)):
        # the records without the fade: the reference's, or (filtered) the GPU's own filtered-only records
        base = unf if aa == 0.0 else _varyings(renderer, cu, su, proj, A.OFF, aa)[0]
        got, tm = _varyings(renderer, cu, su, proj, BLOCKS["fade"], aa)
        want_vis = (base["visible"] == 1) & (t > 0)
        assert np.array_equal(got["visible"] == 1, want_vis), (cam, label)
        assert tm["n_visible"] == int(want_vis.sum()) and 0 < want_vis.sum() < (base["visible"] == 1).sum()
        _unchanged(got, base, want_vis, ("ndc", "depth", "major", "minor"), (cam, label))
        assert FM.bits_equal(np.ascontiguousarray(got["rgba"][want_vis][:, :3]), np.ascontiguousarray(base["rgba"][want_vis][:, :3])), (cam, label)
        alpha = (base["rgba"][:, 3].astype(F32) * fs).astype(F32)
        assert FM.bits_equal(got["rgba"][want_vis][:, 3].copy(), alpha[want_vis]), (cam, label)
        ramp = want_vis & (t < 1)
        assert ramp.sum() > 50 and (got["rgba"][ramp][:, 3] < base["rgba"][ramp][:, 3]).all()
        print(f"{cam} {label}: visible {int(want_vis.sum())} of {int((base['visible'] == 1).sum())}, {int(ramp.sum())} inside the ramp")


# ---- 2. the fade on the surfaces ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["case_hmap", "case_sphere"])
def test_fade_on_the_surfaces(renderer, name):
    g, cu, su, proj, unf = FM.view(name, "persp")
    FM.bind(renderer, g)
    cam = _block(cu)
    vis = unf["visible"] == 1
    dist, z = AR.dist_f64(cam, unf["ndc"][vis], unf["depth"][vis])
    start, end = AR.ramp_from_percentiles(dist)
    atm = A.Atmosphere(fade=(start, end))
    p = AR.params(atm)
    tol = AR.surface_t_tol(z, AR.near_of(cam), p)
    inside, at_one, at_zero, _ = AR.ramp_shares(dist, p)
    assert inside >= 0.25 and at_one >= 0.10 and at_zero >= 0.10
    t, fs = AR.fade_f64(dist, p)
    raw = (float(p["fade_end"]) - dist) * float(p["fade_inv"])
    masked = np.abs(raw) <= tol
    assert masked.mean() <= AR.MAX_MASKED
    got, tm = _varyings(renderer, cu, su, proj, atm)
    assert not (got["visible"][~vis] == 1).any()
    gv = got[vis]
    ok = ~masked
    assert np.array_equal(gv["visible"][ok] == 1, t[ok] > 0), name
    keep = ok & (t > 0)
    _unchanged(gv, unf[vis], keep, ("ndc", "depth", "major", "minor"), name)
    a0 = unf["rgba"][vis][:, 3].astype(np.float64)
    err = np.abs(gv["rgba"][:, 3].astype(np.float64) - a0 * fs)[keep]
    bound = (a0 * (1.5 * tol + 4.0 * AR.U) + AR.U)[keep]
    print(f"{name}: ramp {start:.4f} .. {end:.4f}, {int(keep.sum())} compared, {int(masked.sum())} masked, max |alpha error| / bound {np.max(err / bound):.3f}, "
          f"largest tolerance on t {tol.max():.3e}")
    assert (err <= bound).all(), name
    assert tm["n_visible"] == int((got["visible"] == 1).sum())
    assert abs(int(tm["n_visible"]) - int((t > 0).sum())) <= int(masked.sum())


# ---- 3. the fog's bytes ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["case_plane", "case_hmap", "case_sphere"])
def test_fog_bytes(renderer, name):
    g, cu, su, proj, unf = FM.view(name, "persp")
    FM.bind(renderer, g)
    cam = _block(cu)
    vis = unf["visible"] == 1
    if name == "case_plane":
        dist = AR.dist_f32(cam.cam_pos, su, g["pp"].tex, g["draws"]).astype(np.float64)[vis]
    else:
        dist, _ = AR.dist_f64(cam, unf["ndc"][vis], unf["depth"][vis])
    got, tm = _varyings(renderer, cu, su, proj, BLOCKS["fog"])
    assert np.array_equal(got["visible"] == 1, vis) and tm["n_visible"] == int(vis.sum())
    _unchanged(got, unf, vis, ("ndc", "depth", "major", "minor"), name)
    assert FM.bits_equal(got["rgba"][vis][:, 3].copy(), unf["rgba"][vis][:, 3].copy()), name
    want, near_half = AR.fog_bytes(AR.fog_codes_f64(unf["rgba"][vis][:, :3], dist, AR.params(BLOCKS["fog"])))
    codes = got["rgba"][vis][:, :3].astype(np.float64) * 255.0
    have = np.rint(codes)
    assert np.abs(codes - have).max() < 1e-4                                  # rgba[k] = (float)byte' / 255.0f
    changed = float((have != AR.bytes_of(unf["rgba"][vis])).mean())
    print(f"{name}: {int(vis.sum())} visible, {near_half.mean():.4%} of the channels inside the margin, {int((have != want).sum())} bytes off the float64 rint, "
          f"{changed:.2%} of the bytes changed")
    assert near_half.mean() <= AR.MAX_MASKED
    assert np.abs(have - want).max() <= 1.0, name
    assert np.array_equal(have[~near_half], want[~near_half]), name
    assert changed > 0.9


# ---- 4. known answers --------------------------------------------------------------------------------------------------------------------
def test_known_answers(renderer):
    """Five opaque splats under an eye at the origin at distances that are exact in binary32: 5, 7.5, 10, 2.5 and 15."""
    from gswt_renderer_amd import host
    pos = [(3.0, 4.0, 0.0), (4.5, 6.0, 0.0), (6.0, 8.0, 0.0), (0.0, 2.5, 0.0), (9.0, 12.0, 0.0)]
    # (taller than wide on screen: an isotropic splat on the screen's centre line has c01 = 0 and l1 = c00, a 0 / 0 direction in vs_main)
    halves = S.diag_halves((0.03, 0.03, 0.06))
    rows = [(p, halves, (200, 100 + 20 * k, 50, 255)) for k, p in enumerate(pos)]
    scene = S.raw_scene(rows)
    _, pd = scene.draws(map_index=7)
    renderer.configure(None)
    scene.upload(renderer)
    renderer.set_draws(pd)
    su = orc.scene_uniforms(num_lod=1)
    cu = host.camera_uniforms((0.0, 0.0, 0.0), (2.0, 4.0, 0.0), (0, 0, 1), 45.0, 0.1, 2400.0, W, Hh)[0]
    assert tuple(_block(cu).cam_pos)[:3] == (0.0, 0.0, 0.0)
    base, tm = _varyings(renderer, cu, su, PERSP, A.OFF)
    assert (base["visible"] == 1).all() and tm["n_visible"] == 5 and (base["rgba"][:, 3] == 1.0).all()
    base_bytes = AR.bytes_of(base["rgba"])
    assert np.array_equal(base_bytes, np.array([[200, 100 + 20 * k, 50] for k in range(5)], np.float64))
    got, tm = _varyings(renderer, cu, su, PERSP, A.Atmosphere(fade=(5.0, 10.0)))
    assert list(got["visible"]) == [1, 1, 0, 1, 0] and tm["n_visible"] == 3
    assert FM.bits_equal(got["rgba"][[0, 3]][:, 3].copy(), base["rgba"][[0, 3]][:, 3].copy())             # distances 5 and 2.5: t = 1
    assert got["rgba"][1, 3] == F32(0.5) * base["rgba"][1, 3]                                            # distance 7.5: exactly half
    assert np.array_equal(AR.bytes_of(got["rgba"][[0, 1, 3]]), base_bytes[[0, 1, 3]])                    # the fade leaves the colours alone
    # fog that begins behind every splat changes nothing; a saturated fog leaves the fog colour alone
    got, tm = _varyings(renderer, cu, su, PERSP, A.Atmosphere(fog=(0.15, 20.0, 0.9, FOG[3])))
    assert tm["n_visible"] == 5 and np.array_equal(AR.bytes_of(got["rgba"]), base_bytes)
    assert FM.bits_equal(got["rgba"].copy(), base["rgba"].copy())
    got, tm = _varyings(renderer, cu, su, PERSP, A.Atmosphere(fog=(1e6, 0.0, 1.0, FOG[3])))
    want = np.rint(255.0 * np.array(FOG[3], F32).astype(np.float64))
    assert tm["n_visible"] == 5 and (AR.bytes_of(got["rgba"]) == want[None, :]).all()
    assert FM.bits_equal(got["rgba"][:, 3].copy(), base["rgba"][:, 3].copy())


# ---- 5. image, depth and pick over the GPU's own records ----------------------------------------------------------------------------------
def _image_case(renderer, cam, order_mode, bg, splat_scale, atm=BLOCKS["both"]):
    c = FM.image_case(renderer, cam, order_mode, bg, splat_scale, dict(antialias=0.0, atmosphere=atm), "atmosphere")
    # ... it is not the frame without the atmosphere, and the fade did not add pairs
    off = c["again"](atmosphere=A.OFF)
    assert not FM.same(c["img"], off) and renderer.timings()["n_pairs"] >= c["t"]["n_pairs"] > 0
    return c["t"]


@pytest.mark.parametrize("bg", [False, True], ids=["clear", "bg"])
@pytest.mark.parametrize("order_mode", [0, 1], ids=["reference", "depth"])
@pytest.mark.parametrize("cam", ["persp", "oblique"])
def test_image_depth_and_pick_match_the_references(renderer, cam, order_mode, bg):
    _image_case(renderer, cam, order_mode, bg, OR.SPLAT_SCALE)


def test_image_depth_and_pick_with_several_segments_per_tile(renderer):
    renderer.set_option(L.GSWT_OPT_SEGMENT, 256)
    t = _image_case(renderer, "oblique", L.GSWT_ORDER_DEPTH, True, OR.SPLAT_SCALE_DENSE)
    lens = renderer.read_ranges().astype(np.int64)
    assert ((lens[:, 1] - lens[:, 0]) > 256).sum() >= 1 and t["n_pairs"] > 256


# ---- 6. the same bits every way ------------------------------------------------------------------------------------------------------------
def _set_block(renderer, name):
    renderer.set_atmosphere(BLOCKS[name])


MODE = FM.Mode({name: (None, dict(atmosphere=blk)) for name, blk in BLOCKS.items()}, _set_block, on="both")


@pytest.fixture()
def plain(renderer):
    """The plane case bound under its perspective camera, depth order over a background, and the plain synchronous frames (colour,
    depth, pick) under each block of BLOCKS."""
    g, cu, su, proj, _ = FM.view("case_plane", "persp")
    s = FM.plain_frames(renderer, MODE, g, su, cu)
    renderer.set_atmosphere(A.OFF)
    pairs = s["pairs"]
    assert len({bytes(np.ascontiguousarray(f[0])) for f in s["frames"].values()}) == len(BLOCKS)
    assert pairs["fog"] == pairs["off"] and pairs["both"] == pairs["fade"] < pairs["off"] and pairs["near"] < pairs["fade"]
    return s


def test_graph_replay_with_alternating_blocks(renderer, plain):
    seq1 = ["off", "both", "fade", "both", "off", "fog"]
    seq2 = ["both", "off", "near", "fog", "off", "fade"]
    FM.check_graph_replay(renderer, plain, MODE, seq1, seq2)


def test_async_frames_in_flight_keep_their_block(renderer, plain):
    assert renderer.frame_slots() >= 4
    seq = ["both", "off", "near", "fade"]                      # four frames in flight, each with a block of its own
    FM.check_in_flight(renderer, plain, MODE, seq, waves=4, then="fog")


@pytest.mark.parametrize("opt", [L.GSWT_OPT_NO_CHUNK_CULL], ids=["no_chunk_cull"])
def test_compositor_and_cull_variants(renderer, plain, opt):
    FM.check_with_option_on(renderer, plain, MODE, opt, [MODE.on])


def test_pair_buffer_overflow_rerun_keeps_the_block(renderer, plain):
    FM.check_overflow_rerun(renderer, plain, MODE, MODE.on, then="near")


def test_output_formats(renderer, plain):
    FM.check_output_formats(renderer, plain, MODE, [MODE.on])


@pytest.mark.parametrize("n", [2, 3])
def test_row_shards_tile_the_frame(renderer, plain, n):
    FM.check_row_shards(renderer, plain, MODE, n, [MODE.on])


@pytest.mark.parametrize("n", [2, 3, 5])
def test_column_bands_unite_to_the_frame(renderer, plain, n):
    FM.check_column_bands(renderer, plain, MODE, n, [MODE.on])


# ---- 7. off is untouched --------------------------------------------------------------------------------------------------------------------
def _null_block(r):
    r.set_atmosphere(None)
    return {}


@pytest.mark.parametrize("cam", ["persp", "oblique"])
def test_off_is_untouched(cam):
    """A context on which the block was never set, then frames with it, then NULL, then OFF: byte-identical colour, depth, pick and
    counts, and the vertex stage with the block off is still the reference's, bit for bit, the visible mask included."""
    FM.check_off_is_untouched(cam, dict(atmosphere=BLOCKS["both"]), [("NULL", _null_block), ("OFF", lambda r: dict(atmosphere=A.OFF))])


# ---- 8. refusals ----------------------------------------------------------------------------------------------------------------------------
def _raw_block(**kw):
    f = dict(fade_start=4.0, fade_end=8.0, fog_density=0.15, fog_start=2.0, fog_max=0.9, r=0.62, g=0.71, b=0.80)
    f.update(kw)
    return (C.c_char * 32).from_buffer_copy(struct.pack("<8f", *(f[k] for k in ("fade_start", "fade_end", "fog_density", "fog_start", "fog_max", "r", "g", "b"))))


def test_refused_blocks_leave_the_block_in_force(renderer, plain):
    lib, h = renderer._lib, renderer._h
    nan, inf = float("nan"), float("inf")
    assert lib.gswt_set_atmosphere(h, _raw_block()) == L.GSWT_OK          # = BLOCKS["both"]
    bad = [("fade_start", dict(fade_start=-1.0)), ("fade_start", dict(fade_start=nan)), ("fade_end", dict(fade_end=4.0)), ("fade_end", dict(fade_end=3.0)),
           ("fade_end", dict(fade_end=inf)), ("fade_end", dict(fade_end=nan)), ("fade_end", dict(fade_start=4.0, fade_end=0.0)),
           ("fade_end", dict(fade_start=0.0, fade_end=1e-45)),           # 1.0f / (fade_end - fade_start) is not finite
           ("fog_density", dict(fog_density=-0.1)), ("fog_density", dict(fog_density=nan)), ("fog_density", dict(fog_density=inf)),
           ("fog_start", dict(fog_start=-1.0)), ("fog_start", dict(fog_start=nan)),
           ("fog_max", dict(fog_max=0.0)), ("fog_max", dict(fog_max=1.5)), ("fog_max", dict(fog_max=-0.5)), ("fog_max", dict(fog_max=nan)),
           ("fog_color[0]", dict(r=1.5)), ("fog_color[1]", dict(g=-0.1)), ("fog_color[2]", dict(b=nan)), ("fog_color[2]", dict(b=inf))]
    for field, kw in bad:
        assert lib.gswt_set_atmosphere(h, _raw_block(**kw)) == L.GSWT_ERR_BAD_ARG, (field, kw)
        assert field.encode() in lib.gswt_last_error(h), (field, kw, lib.gswt_last_error(h))
    with pytest.raises(GSWTError):
        renderer.set_atmosphere(A.Atmosphere(fade=(8.0, 4.0)))
    got = renderer.render(plain["cu"], plain["su"], W, Hh, depth=True, pick=True, **plain["kw"])
    FM.assert_frames([got], ["both"], plain, "after refused blocks")
    # the edges of the ranges are accepted
    for kw in (dict(fade_start=0.0), dict(fog_max=1.0), dict(fog_start=0.0), dict(r=0.0, g=1.0), dict(fade_start=0.0, fade_end=0.0), dict(fog_density=0.0, fog_max=0.0)):
        assert lib.gswt_set_atmosphere(h, _raw_block(**kw)) == L.GSWT_OK, kw
    assert lib.gswt_set_atmosphere(h, None) == L.GSWT_OK
    got = renderer.render(plain["cu"], plain["su"], W, Hh, depth=True, pick=True, **plain["kw"])
    FM.assert_frames([got], ["off"], plain, "after NULL")


def test_sequence_v2_is_refused_at_submit(renderer, plain):
    FM.check_v2_refused_at_submit(renderer, plain, MODE, ("fade", "fog", "both"), (b"GSWT_OPT_STRICT_VS", b"gswt_set_atmosphere"))


# ---- 9. the proxy pass ------------------------------------------------------------------------------------------------------------------------
def _proxy(renderer, us, Wp, Hp, grid_dim, hm, mips, atm):
    import torch
    renderer.configure(hm)
    renderer.proxy_configure(mips, grid_dim=grid_dim)
    renderer.set_atmosphere(atm)
    rgba = torch.from_numpy(R.sky(Wp, Hp)).cuda()
    depth = torch.zeros((Hp, Wp), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    for k, u in enumerate(us):
        renderer.proxy_render(u, Wp, Hp, rgba.data_ptr(), depth.data_ptr(), clear_depth=(k == 0))
    renderer.synchronize()
    return depth.cpu().numpy(), rgba.cpu().numpy()


@pytest.mark.parametrize("name", ["oblique", "flat_two_draws", "clip_two_draws", "black_background"])
def test_proxy_is_fogged(renderer, name):
    cam_kw, draws, grid_dim, _ = R.SCENES[name]
    Wp, Hp = R.W0, R.H0
    cam = R.scene_camera(cam_kw, Wp, Hp)
    us = R.scene_uniforms(cam, draws)
    hm, mips = R.height_map(), R.mip_chain()
    atm = A.Atmosphere(fade=(1.0, 2.0), fog=FOG)                # (the fade does not apply to the proxy)
    d0, c0 = _proxy(renderer, us, Wp, Hp, grid_dim, hm, mips, A.OFF)
    d1, c1 = _proxy(renderer, us, Wp, Hp, grid_dim, hm, mips, atm)
    d2, c2 = _proxy(renderer, us, Wp, Hp, grid_dim, hm, mips, A.Atmosphere(fade=(1.0, 2.0)))
    assert FM.same(d0, d1) and FM.same(d0, d2) and FM.same(c0, c2)
    written = d0 < 1.0
    assert written.mean() > 0.05
    sky = R.sky(Wp, Hp)
    assert FM.same(c1[~written], sky[~written]) and FM.same(c0[~written], sky[~written])
    if name == "black_background":
        assert FM.same(c0, c1) and (c0[written] == np.array([0, 0, 0, 1], F32)).all()
        return
    # the hit distance from the float64 unprojection of the proxy's own depth
    cu = cam.uniforms()
    ys, xs = np.nonzero(written)
    ndc = np.stack([(xs + 0.5) / Wp * 2.0 - 1.0, 1.0 - (ys + 0.5) / Hp * 2.0], 1)
    dist, z = AR.dist_f64(cu, ndc, d0[written])
    p = AR.params(atm)
    near = AR.near_of(cu)
    F = AR.fog_amount_f64(dist, p)[:, None]
    want = c0[written][:, :3].astype(np.float64) * (1.0 - F) + p["fog_color"].astype(np.float64)[None] * F
    tol = 2e-6 + 4.0 * float(p["fog_max"]) * float(p["fog_density"]) * z * z / near * AR.U
    err = np.abs(c1[written][:, :3].astype(np.float64) - want).max(1)
    print(f"{name}: {int(written.sum())} proxy pixels, F {F.min():.3f} .. {F.max():.3f}, max |colour error| / tolerance {np.max(err / tol):.3f}, largest tolerance {tol.max():.2e}")
    assert (err <= tol).all()
    assert (c1[written][:, 3] == 1.0).all()
    assert F.max() > 0.3 and not FM.same(c0, c1)


# ---- 10. through the frame harness -----------------------------------------------------------------------------------------------------------
def test_pipeline_passes_atmosphere_through(renderer):
    """GSWTPipeline.render(atmosphere=...) is GSWTRenderer.render with the pipeline's scene block (merged draws: the single_draw offsets
    are under the fade): the same bits as the direct call, another frame than the one without, and OFF gives that one back."""
    from gswt_renderer_amd import host, synth
    from gswt_renderer_amd.pipeline import GSWTPipeline
    cfg = dict(tile_map_half_wh=(3, 3), surface_type=0, lod_max_dist=20.0, tile_sort_type=3, merge_type=2)
    pipe = GSWTPipeline(synth.make_tileset(n_lod=3, n_tile=16, lod0_count=800), host.user_data(**cfg), renderer=renderer)
    pos = (4.2, 1.0, 2.0)
    cu, vp = host.camera_uniforms(pos, (5.0, 3.0, 1.5), (0, 0, 1), 45.0, 0.1, 2400.0, W, Hh)
    pipe.update(pos, vp)
    off = pipe.render(cu, W, Hh)
    pairs_off = renderer.timings()["n_pairs"]
    atm = A.Atmosphere(fade=(3.0, 9.0), fog=FOG)
    on = pipe.render(cu, W, Hh, atmosphere=atm)
    assert 0 < renderer.timings()["n_pairs"] < pairs_off and not FM.same(on, off)
    renderer.set_atmosphere(A.OFF)
    assert FM.same(renderer.render(cu, pipe.wang.scene_uniforms(), W, Hh, atmosphere=atm), on)
    assert FM.same(pipe.render(cu, W, Hh), on)                   # (no argument: the context keeps the block)
    assert FM.same(pipe.render(cu, W, Hh, atmosphere=A.OFF), off)
