"""The atmosphere (gswt_set_atmosphere, include/gswt_hip.h) on the GPU: per-splat far fade and distance fog, and the fogged proxy ground.
Frames are 72 x 40 (tests/ortho_ref.py): 5 x 3 screen tiles, partial on the right and bottom edges; the scenes are the golden cases with
the draws of their own perspective sort event.

The faded vertex stage bit for bit against tests/atmosphere_ref.py on the plain surface (perspective and orthographic, with and without
the pixel filter) and within the derived tolerance on the HeightMap and Sphere surfaces; the fogged colour bytes against the float64
reference; known answers; image, depth and pick against the CPU references over the GPU's own records; the same bits through graphs,
frames in flight, compositor and cull variants, a pair-buffer overflow, output formats and shards; the block off leaves every output as
it was; the refusals; the proxy pass; the pipeline's keyword."""
import ctypes as C
import struct

import numpy as np
import pytest

from gswt_renderer_amd import _lib as L
from gswt_renderer_amd import atmosphere as A
from gswt_renderer_amd.renderer import PICK_DTYPE, GSWTError, GSWTRenderer
from oracle import gswt_oracle as orc
from tests import atmosphere_ref as AR
from tests import depth_ref as DR
from tests import ortho_ref as OR
from tests import pick_ref as PR
from tests import proxy_raster_ref as R
from tests import special_splats as S
from tests import unorm8_ref as U8
from tests import yuv_ref as YUV
from tests.test_depth_out_gpu import _check_against_ref
from tests.test_ortho_gpu import _bind, _bits_equal, _cam, _persp, _same

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
    """Every test leaves the shared context as it found it: no atmosphere, perspective, no filter, default options."""
    yield
    renderer.set_atmosphere(A.OFF)
    for key, value in ((L.GSWT_OPT_ANTIALIAS, 0), (L.GSWT_OPT_PROJECTION, PERSP), (L.GSWT_OPT_STRICT_VS, 1), (L.GSWT_OPT_GRAPH, 0), (L.GSWT_OPT_TIMING, 2),
                       (L.GSWT_OPT_SEGMENT, L.GSWT_DEFAULT_SEGMENT), (L.GSWT_OPT_COMPOSITE, 0), (L.GSWT_OPT_NO_CHUNK_CULL, 0),
                       (L.GSWT_OPT_ITEM_ORDER, 0), (L.GSWT_OPT_PAIR_CAP, 0), (L.GSWT_OPT_DEBUG_VARYINGS, 0), (L.GSWT_OPT_NO_LOD_PREFILTER, 0)):
        renderer.set_option(key, value)
    renderer.configure(None)


def _varyings(renderer, cu, su, projection, atm, antialias=0.0):
    renderer.set_option(L.GSWT_OPT_DEBUG_VARYINGS, 1)
    try:
        renderer.render(cu, su, W, Hh, projection=projection, antialias=antialias, atmosphere=atm)
        return renderer.read_projected().view(orc.SPLAT_DTYPE), renderer.timings()
    finally:
        renderer.set_option(L.GSWT_OPT_DEBUG_VARYINGS, 0)


_VIEWS = {}


def _view(name, cam, splat_scale=OR.SPLAT_SCALE):
    """(golden case, camera block, scene block, projection, reference records WITHOUT atmosphere) of case `name` under camera `cam`:
    "persp" (the oracle's vertex stage) or one of OR.CAMERAS (tests/ortho_ref.py's restatement, plane case only); computed once."""
    k = (name, cam, splat_scale)
    if k not in _VIEWS:
        g = OR.golden(name)
        if cam == "persp":
            cu, su = _persp(g), OR.scene_of(g, splat_scale)
            sp = orc.project_draws(orc.Camera176.from_buffer_copy(bytes(cu)), su, g["pp"].tex, g["draws"], height_map=g["hm"])
            _VIEWS[k] = (g, cu, su, PERSP, sp)
        else:
            assert name == "case_plane"
            _, su, sp = OR.plane_records(cam, splat_scale)
            _VIEWS[k] = (g, _cam(cam, g).uniforms(), su, ORTHO, sp)
    return _VIEWS[k]


def _block(cu):
    return orc.Camera176.from_buffer_copy(bytes(cu))


def _unchanged(got, base, m, fields, label):
    for fld in fields:
        assert _bits_equal(np.ascontiguousarray(got[fld][m]), np.ascontiguousarray(base[fld][m])), (label, fld)


# ---- 1. the fade, bit for bit --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cam", ["persp", "top", "oblique"])
def test_fade_is_bit_exact_on_the_plain_surface(renderer, cam):
    g, cu, su, proj, unf = _view("case_plane", cam)
    _bind(renderer, g)
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
        assert _bits_equal(np.ascontiguousarray(got["rgba"][want_vis][:, :3]), np.ascontiguousarray(base["rgba"][want_vis][:, :3])), (cam, label)
        alpha = (base["rgba"][:, 3].astype(F32) * fs).astype(F32)
        assert _bits_equal(got["rgba"][want_vis][:, 3].copy(), alpha[want_vis]), (cam, label)
        ramp = want_vis & (t < 1)
        assert ramp.sum() > 50 and (got["rgba"][ramp][:, 3] < base["rgba"][ramp][:, 3]).all()
        print(f"{cam} {label}: visible {int(want_vis.sum())} of {int((base['visible'] == 1).sum())}, {int(ramp.sum())} inside the ramp")


# ---- 2. the fade on the surfaces ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["case_hmap", "case_sphere"])
def test_fade_on_the_surfaces(renderer, name):
    g, cu, su, proj, unf = _view(name, "persp")
    _bind(renderer, g)
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
    g, cu, su, proj, unf = _view(name, "persp")
    _bind(renderer, g)
    cam = _block(cu)
    vis = unf["visible"] == 1
    if name == "case_plane":
        dist = AR.dist_f32(cam.cam_pos, su, g["pp"].tex, g["draws"]).astype(np.float64)[vis]
    else:
        dist, _ = AR.dist_f64(cam, unf["ndc"][vis], unf["depth"][vis])
    got, tm = _varyings(renderer, cu, su, proj, BLOCKS["fog"])
    assert np.array_equal(got["visible"] == 1, vis) and tm["n_visible"] == int(vis.sum())
    _unchanged(got, unf, vis, ("ndc", "depth", "major", "minor"), name)
    assert _bits_equal(got["rgba"][vis][:, 3].copy(), unf["rgba"][vis][:, 3].copy()), name
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
    assert _bits_equal(got["rgba"][[0, 3]][:, 3].copy(), base["rgba"][[0, 3]][:, 3].copy())             # distances 5 and 2.5: t = 1
    assert got["rgba"][1, 3] == F32(0.5) * base["rgba"][1, 3]                                            # distance 7.5: exactly half
    assert np.array_equal(AR.bytes_of(got["rgba"][[0, 1, 3]]), base_bytes[[0, 1, 3]])                    # the fade leaves the colours alone
    # fog that begins behind every splat changes nothing; a saturated fog leaves the fog colour alone
    got, tm = _varyings(renderer, cu, su, PERSP, A.Atmosphere(fog=(0.15, 20.0, 0.9, FOG[3])))
    assert tm["n_visible"] == 5 and np.array_equal(AR.bytes_of(got["rgba"]), base_bytes)
    assert _bits_equal(got["rgba"].copy(), base["rgba"].copy())
    got, tm = _varyings(renderer, cu, su, PERSP, A.Atmosphere(fog=(1e6, 0.0, 1.0, FOG[3])))
    want = np.rint(255.0 * np.array(FOG[3], F32).astype(np.float64))
    assert tm["n_visible"] == 5 and (AR.bytes_of(got["rgba"]) == want[None, :]).all()
    assert _bits_equal(got["rgba"][:, 3].copy(), base["rgba"][:, 3].copy())


# ---- 5. image, depth and pick over the GPU's own records ----------------------------------------------------------------------------------
def _image_case(renderer, cam, order_mode, bg, splat_scale, atm=BLOCKS["both"]):
    g, cu, su, proj, _ = _view("case_plane", cam, splat_scale)
    _bind(renderer, g)
    sp, _ = _varyings(renderer, cu, su, proj, atm)
    bgc, bgd = DR.bg_images(W, Hh) if bg else (None, None)
    kw = dict(order_mode=order_mode, bg_rgba=bgc, bg_depth=bgd)
    img, z, pick = renderer.render(cu, su, W, Hh, projection=proj, depth=True, pick=True, **kw)          # (the context keeps the block)
    t = renderer.timings()
    assert z.shape == (Hh, W) and pick.shape == (Hh, W) and pick.dtype == PICK_DTYPE
    ref_img, ref_z, n_cover = DR.composite(sp, W, Hh, splat_scale=splat_scale, with_cover=True, **kw)
    assert (n_cover > 0).mean() > 0.3 and ref_img[..., 3].max() > 0.5
    dz = _check_against_ref(img, z, ref_img, ref_z)
    ev = PR.composite(sp, W, Hh, splat_scale=splat_scale, **kw)
    mi, en = PR.identities(g["draws"])
    label = f"atmosphere {cam} order={order_mode} bg={bg} scale={splat_scale}"
    dw = PR.check_pick(pick, ev, sp, mi, en, label=label)
    print(f"{label}: visible {t['n_visible']} pairs {t['n_pairs']} max|dz| {dz:.3e} max|dw| {dw:.3e}")
    assert t["n_visible"] == int((sp["visible"] == 1).sum())
    assert _same(img, renderer.render(cu, su, W, Hh, projection=proj, **kw))
    # ... it is not the frame without the atmosphere, and the fade did not add pairs
    off = renderer.render(cu, su, W, Hh, projection=proj, atmosphere=A.OFF, **kw)
    assert not _same(img, off) and renderer.timings()["n_pairs"] >= t["n_pairs"] > 0
    return t


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
@pytest.fixture()
def plain(renderer):
    """The plane case bound under its perspective camera, depth order over a background, and the plain synchronous frames (colour,
    depth, pick) under each block of BLOCKS."""
    g, cu, su, proj, _ = _view("case_plane", "persp")
    _bind(renderer, g)
    bgc, bgd = DR.bg_images(W, Hh)
    kw = dict(order_mode=L.GSWT_ORDER_DEPTH, bg_rgba=bgc, bg_depth=bgd)
    frames, pairs = {}, {}
    for name, blk in BLOCKS.items():
        frames[name] = renderer.render(cu, su, W, Hh, projection=PERSP, atmosphere=blk, depth=True, pick=True, **kw)
        pairs[name] = renderer.timings()["n_pairs"]
    renderer.set_atmosphere(A.OFF)
    assert len({bytes(np.ascontiguousarray(f[0])) for f in frames.values()}) == len(BLOCKS)
    assert pairs["fog"] == pairs["off"] and pairs["both"] == pairs["fade"] < pairs["off"] and pairs["near"] < pairs["fade"]
    return dict(g=g, cu=cu, su=su, kw=kw, bgc=bgc, bgd=bgd, frames=frames, pairs=pairs)


def _device_frames(renderer, s, seq, *, waves, then=None):
    """Submits frames under the blocks named in `seq` with render_async, `waves` at a time in flight, into buffers of their own; sets
    the context's block to `then` before waiting; returns (colour, depth, pick) as numpy arrays."""
    import torch
    bgc, bgd = torch.from_numpy(s["bgc"]).cuda(), torch.from_numpy(s["bgd"]).cuda()
    outs = [(torch.zeros((Hh, W, 4), dtype=torch.float32, device="cuda"), torch.full((Hh, W), -1.0, dtype=torch.float32, device="cuda"),
             torch.full((Hh, W, 4), -1, dtype=torch.int32, device="cuda")) for _ in seq]
    torch.cuda.synchronize()
    for i in range(0, len(seq), waves):
        tickets = []
        for name, (o, z, p) in zip(seq[i:i + waves], outs[i:i + waves]):
            tickets.append(renderer.render_async(s["cu"], s["su"], W, Hh, o.data_ptr(), order_mode=L.GSWT_ORDER_DEPTH, bg_rgba_ptr=bgc.data_ptr(),
                                                 bg_depth_ptr=bgd.data_ptr(), out_depth_ptr=z.data_ptr(), out_pick_ptr=p.data_ptr(),
                                                 atmosphere=BLOCKS[name]))
        assert len(set(tickets)) == len(tickets)
        if then is not None:                                                 # must not reach the frames already submitted
            renderer.set_atmosphere(BLOCKS[then])
        for t in tickets:
            renderer.render_wait(t)
    torch.cuda.synchronize()
    return [(o.cpu().numpy(), z.cpu().numpy(), p.cpu().numpy()) for o, z, p in outs]


def _assert_frames(got, seq, s, what):
    for k, (name, f) in enumerate(zip(seq, got)):
        want = s["frames"][name]
        assert _same(f[0], want[0]) and _same(f[1], want[1]) and _same(f[2], want[2]), (what, k, name)


def test_graph_replay_with_alternating_blocks(renderer, plain):
    renderer.set_option(L.GSWT_OPT_TIMING, 0)
    renderer.set_option(L.GSWT_OPT_GRAPH, 1)
    launches0, _, _ = renderer.graph_stats()
    seq1 = ["off", "both", "fade", "both", "off", "fog"]
    _assert_frames(_device_frames(renderer, plain, seq1, waves=1), seq1, plain, "graph, one slot")
    seq2 = ["both", "off", "near", "fog", "off", "fade"]
    _assert_frames(_device_frames(renderer, plain, seq2, waves=2), seq2, plain, "graph, two slots")
    launches, _, _ = renderer.graph_stats()
    assert launches - launches0 == len(seq1) + len(seq2)


def test_async_frames_in_flight_keep_their_block(renderer, plain):
    assert renderer.frame_slots() >= 4
    seq = ["both", "off", "near", "fade"]                      # four frames in flight, each with a block of its own
    _assert_frames(_device_frames(renderer, plain, seq, waves=4, then="fog"), seq, plain, "async")


@pytest.mark.parametrize("opt", [L.GSWT_OPT_COMPOSITE, L.GSWT_OPT_ITEM_ORDER, L.GSWT_OPT_NO_CHUNK_CULL], ids=["composite_dw", "item_order", "no_chunk_cull"])
def test_compositor_and_cull_variants(renderer, plain, opt):
    renderer.set_option(opt, 1)
    got = renderer.render(plain["cu"], plain["su"], W, Hh, atmosphere=BLOCKS["both"], depth=True, pick=True, **plain["kw"])
    _assert_frames([got], ["both"], plain, opt)


def test_pair_buffer_overflow_rerun_keeps_the_block(renderer, plain):
    assert plain["pairs"]["both"] > 256
    renderer.set_option(L.GSWT_OPT_PAIR_CAP, 256)             # the next frame overflows and is re-run with grown buffers
    got = renderer.render(plain["cu"], plain["su"], W, Hh, atmosphere=BLOCKS["both"], depth=True, pick=True, **plain["kw"])
    assert renderer.timings()["n_pairs"] == plain["pairs"]["both"]
    _assert_frames([got], ["both"], plain, "overflow, synchronous")
    # ... and in flight, with the block changed between submit and the wait that re-runs the frame
    renderer.set_option(L.GSWT_OPT_PAIR_CAP, 256)
    _assert_frames(_device_frames(renderer, plain, ["both"], waves=1, then="near"), ["both"], plain, "overflow, in flight")
    assert renderer.timings()["n_pairs"] == plain["pairs"]["both"]


def test_output_formats(renderer, plain):
    f32 = plain["frames"]["both"][0]
    kw = dict(atmosphere=BLOCKS["both"], **plain["kw"])
    assert np.array_equal(renderer.render(plain["cu"], plain["su"], W, Hh, out_format=L.GSWT_OUT_RGBA8_UNORM, **kw), U8.rgba8(f32))
    y, cbcr = renderer.render(plain["cu"], plain["su"], W, Hh, out_format=L.GSWT_VIDEO_NV12, **kw)
    wy, wc = YUV.nv12(f32)
    assert np.array_equal(y, wy) and np.array_equal(cbcr, wc)


@pytest.mark.parametrize("n", [2, 3])
def test_row_shards_tile_the_frame(renderer, plain, n):
    kw = dict(atmosphere=BLOCKS["both"], depth=True, pick=True, **plain["kw"])
    full = plain["frames"]["both"]
    rows = renderer.shard_rows_padded(Hh, n)
    parts = [np.zeros((Hh, W, 4), np.float32), np.zeros((Hh, W), np.float32), np.zeros((Hh, W), PICK_DTYPE)]
    for r in range(n):
        got = renderer.render(plain["cu"], plain["su"], W, Hh, shard=(r, n), **kw)
        assert got[0].shape == (rows, W, 4)
        k = 0
        for ty in range(r, (Hh + 15) // 16, n):
            y0, y1 = ty * 16, min(Hh, ty * 16 + 16)
            for dst, src in zip(parts, got):
                dst[y0:y1] = src[k * 16:k * 16 + (y1 - y0)]
            k += 1
    for a, b in zip(parts, full):
        assert _same(a, b), n


@pytest.mark.parametrize("n", [2, 3, 5])
def test_column_bands_unite_to_the_frame(renderer, plain, n):
    kw = dict(atmosphere=BLOCKS["both"], depth=True, pick=True, **plain["kw"])
    full = plain["frames"]["both"]
    bw = renderer.shard_cols_padded(W, n)
    parts = [np.zeros((Hh, W, 4), np.float32), np.zeros((Hh, W), np.float32), np.zeros((Hh, W), PICK_DTYPE)]
    for r in range(n):
        got = renderer.render(plain["cu"], plain["su"], W, Hh, shard=(r, n, "cols"), **kw)
        x0, x1 = r * bw, min(W, (r + 1) * bw)
        assert got[0].shape == (Hh, bw, 4)
        for dst, src in zip(parts, got):
            dst[:, x0:x1] = src[:, :x1 - x0]
    for a, b in zip(parts, full):
        assert _same(a, b), n


# ---- 7. off is untouched --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cam", ["persp", "oblique"])
def test_off_is_untouched(cam):
    """A context on which the block was never set, then frames with it, then NULL: byte-identical colour, depth, pick and counts."""
    g, cu, su, proj, unf = _view("case_plane", cam)
    r = GSWTRenderer(0)
    try:
        _bind(r, g)
        bgc, bgd = DR.bg_images(W, Hh)
        kw = dict(order_mode=L.GSWT_ORDER_DEPTH, bg_rgba=bgc, bg_depth=bgd, projection=proj, depth=True, pick=True)
        before = r.render(cu, su, W, Hh, **kw)
        t0 = r.timings()
        on = r.render(cu, su, W, Hh, atmosphere=BLOCKS["both"], **kw)
        assert _same(r.render(cu, su, W, Hh, **kw)[0], on[0]) and not _same(on[0], before[0])     # (no argument: the context keeps the block)
        r.set_atmosphere(None)
        after = r.render(cu, su, W, Hh, **kw)
        t1 = r.timings()
        for a, b in zip(before, after):
            assert _same(a, b)
        assert (t0["n_visible"], t0["n_pairs"]) == (t1["n_visible"], t1["n_pairs"])
        assert _same(r.render(cu, su, W, Hh, atmosphere=A.OFF, **kw)[0], before[0])
        assert (before[2]["weight"] > 0).mean() > 0.3
        # ... and the vertex stage with the block off is still the reference's, bit for bit
        r.set_option(L.GSWT_OPT_DEBUG_VARYINGS, 1)
        r.render(cu, su, W, Hh, projection=proj)
        got = r.read_projected().view(orc.SPLAT_DTYPE)
        vis = unf["visible"] == 1
        assert np.array_equal(got["visible"] == 1, vis)
        for fld in ("ndc", "depth", "major", "minor", "rgba"):
            assert _bits_equal(got[fld][vis], unf[fld][vis]), fld
    finally:
        r.close()


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
    _assert_frames([got], ["both"], plain, "after refused blocks")
    # the edges of the ranges are accepted
    for kw in (dict(fade_start=0.0), dict(fog_max=1.0), dict(fog_start=0.0), dict(r=0.0, g=1.0), dict(fade_start=0.0, fade_end=0.0), dict(fog_density=0.0, fog_max=0.0)):
        assert lib.gswt_set_atmosphere(h, _raw_block(**kw)) == L.GSWT_OK, kw
    assert lib.gswt_set_atmosphere(h, None) == L.GSWT_OK
    got = renderer.render(plain["cu"], plain["su"], W, Hh, depth=True, pick=True, **plain["kw"])
    _assert_frames([got], ["off"], plain, "after NULL")


def test_sequence_v2_is_refused_at_submit(renderer, plain):
    import torch
    lib, h = renderer._lib, renderer._h
    cam = (C.c_char * 176).from_buffer_copy(bytes(plain["cu"]))
    sc = (C.c_char * 160).from_buffer_copy(bytes(plain["su"]))
    cfg = L.RenderConfig()
    cfg.culling_dist, cfg.lod_enable_mask, cfg.order_mode = 1.0, 0xFFFFFFFF, L.GSWT_ORDER_DEPTH
    out = np.full((Hh, W, 4), 7.0, np.float32)
    z = np.full((Hh, W), -1.0, np.float32)
    pk = np.full((Hh, W, 4), 0x55555555, np.uint32)
    o_d = torch.full((Hh, W, 4), 7.0, dtype=torch.float32, device="cuda")
    z_d = torch.full((Hh, W), -1.0, dtype=torch.float32, device="cuda")
    p_d = torch.full((Hh, W, 4), 0x55555555, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    for name in ("fade", "fog", "both"):
        renderer.set_atmosphere(BLOCKS[name])
        renderer.set_option(L.GSWT_OPT_STRICT_VS, 0)
        try:
            assert lib.gswt_render_pick(h, cam, sc, C.byref(cfg), W, Hh, None, None, 0, vp(out), vp(z), vp(pk), 0) == L.GSWT_ERR_BAD_ARG, name
            assert b"GSWT_OPT_STRICT_VS" in lib.gswt_last_error(h) and b"gswt_set_atmosphere" in lib.gswt_last_error(h)
            ticket = C.c_int(-7)
            assert lib.gswt_render_async_pick(h, cam, sc, C.byref(cfg), W, Hh, None, None, C.c_void_p(o_d.data_ptr()), C.c_void_p(z_d.data_ptr()),
                                              C.c_void_p(p_d.data_ptr()), C.byref(ticket)) == L.GSWT_ERR_BAD_ARG, name
            assert ticket.value == -7
        finally:
            renderer.set_option(L.GSWT_OPT_STRICT_VS, 1)
        torch.cuda.synchronize()
        assert (out == 7.0).all() and (z == -1.0).all() and (pk == 0x55555555).all(), name
        assert bool((o_d == 7.0).all()) and bool((z_d == -1.0).all()) and bool((p_d == 0x55555555).all()), name
        # the next valid frame renders, with the block still in force
        got = renderer.render(plain["cu"], plain["su"], W, Hh, depth=True, pick=True, **plain["kw"])
        _assert_frames([got], [name], plain, "after the refused v2 frame, " + name)
    # with the block off sequence v2 renders
    renderer.set_atmosphere(A.OFF)
    renderer.set_option(L.GSWT_OPT_STRICT_VS, 0)
    assert lib.gswt_render_pick(h, cam, sc, C.byref(cfg), W, Hh, None, None, 0, vp(out), vp(z), vp(pk), 0) == L.GSWT_OK
    assert not (out == 7.0).all()


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
    assert _same(d0, d1) and _same(d0, d2) and _same(c0, c2)
    written = d0 < 1.0
    assert written.mean() > 0.05
    sky = R.sky(Wp, Hp)
    assert _same(c1[~written], sky[~written]) and _same(c0[~written], sky[~written])
    if name == "black_background":
        assert _same(c0, c1) and (c0[written] == np.array([0, 0, 0, 1], F32)).all()
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
    assert F.max() > 0.3 and not _same(c0, c1)


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
    assert 0 < renderer.timings()["n_pairs"] < pairs_off and not _same(on, off)
    renderer.set_atmosphere(A.OFF)
    assert _same(renderer.render(cu, pipe.wang.scene_uniforms(), W, Hh, atmosphere=atm), on)
    assert _same(pipe.render(cu, W, Hh), on)                   # (no argument: the context keeps the block)
    assert _same(pipe.render(cu, W, Hh, atmosphere=A.OFF), off)
