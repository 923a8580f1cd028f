"""Frames rendered straight into the 4:2:0 video formats (GSWT_VIDEO_NV12 / GSWT_VIDEO_I420, include/gswt_hip.h), case by case as
tests/test_out_format_gpu.py does it for the 8-bit formats: every case renders the same inputs as RGBA f32 and in a video format and
requires the planes to EQUAL tests/yuv_ref.py of the f32 image byte for byte -- every compositor variant and order with and without
the early-out (multi-segment tiles: k_combine's store), screen tiles no splat reaches over a coloured background, a background with
values outside [0, 1] / NaN / inf and a proxy depth buffer, the depth image beside a video frame, an even size that is not a multiple
of the tile (guard bytes behind the last plane untouched), odd sizes refused, row and column shards with gswt_unshard_format, the
peer-copy group gather, asynchronous frames in flight through the graph path with the format changing from frame to frame, host
output, a pair-buffer overflow re-run, and NV12 against I420."""
import functools

import numpy as np
import pytest

from gswt_renderer_amd import _lib as L
from gswt_renderer_amd.renderer import GSWTError, GSWTRenderer, video_planes
from oracle import gswt_oracle as orc
from tests import helpers as H
from tests import yuv_ref
from tests.unorm8_ref import rgba8

pytestmark = pytest.mark.gpu

FORMATS = [(L.GSWT_VIDEO_NV12, yuv_ref.nv12), (L.GSWT_VIDEO_I420, yuv_ref.i420)]
FLAT = {L.GSWT_VIDEO_NV12: yuv_ref.nv12_bytes, L.GSWT_VIDEO_I420: yuv_ref.i420_bytes}
FMT_IDS = ["nv12", "i420"]


@functools.lru_cache(maxsize=1)
def _c3():
    import bench
    return bench.build_workload("c3")


def _load_c3(r):
    w, wang, cu, vp, sort = _c3()
    wang.upload_to(r)
    r.configure(None)
    r.set_draws(sort.draws, sort.merged_gs_index, sort.merged_map_id, sort.merged_lod_id)
    return w["width"], w["height"], cu, wang.scene_uniforms()


def _load_grid(r):
    pp = H.tileset()
    r.upload_scene(pp.tex, pp.gs_index, pp.gs_lod_id)
    r.configure(None)
    r.set_draws(H.grid_case(pp).draws)
    return pp


def _bg(W, Hh, seed=7):
    """A background colour with values outside [0, 1] (and a few NaN / inf) and a proxy depth buffer."""
    rng = np.random.default_rng(seed)
    bg = rng.uniform(-0.6, 1.6, size=(Hh, W, 4)).astype(np.float32)
    flat = bg.reshape(-1)
    idx = rng.choice(flat.size, size=64, replace=False)
    flat[idx[:16]] = np.nan
    flat[idx[16:32]] = np.inf
    flat[idx[32:48]] = -np.inf
    flat[idx[48:]] = 1.0 + 1e-7
    depth = rng.uniform(0.0, 1.0, size=(Hh, W)).astype(np.float32)
    return bg, depth


def _same(got, want):
    """Plane tuples equal in count, shape, type and every byte; on a mismatch the message says which plane and how many samples."""
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == np.uint8 and g.shape == w.shape, (k, g.dtype, g.shape, w.shape)
        assert np.array_equal(g, w), (k, int(np.count_nonzero(g != w)), g.size)
    return True


@pytest.mark.parametrize("order", [L.GSWT_ORDER_REFERENCE, L.GSWT_ORDER_DEPTH], ids=["ref_order", "depth_order"])
@pytest.mark.parametrize("composite", [0, 1, 2])
def test_c3_every_compositor_and_order(renderer, composite, order):
    W, Hh, cu, su = _load_c3(renderer)
    renderer.set_option(L.GSWT_OPT_COMPOSITE, composite)
    try:
        for eps in (0.0, 1e-5):
            kw = dict(transmittance_eps=eps, order_mode=order)
            f32 = renderer.render(cu, su, W, Hh, **kw)
            assert f32.dtype == np.float32 and f32[..., 3].max() > 0.5
            for fmt, ref in FORMATS:
                planes = renderer.render(cu, su, W, Hh, out_format=fmt, **kw)
                assert planes[0].shape == (Hh, W) and planes[1].shape[:2] == (Hh // 2, W // 2)
                assert _same(planes, ref(f32)), (fmt, eps)
    finally:
        renderer.set_option(L.GSWT_OPT_COMPOSITE, 0)


@pytest.mark.parametrize("composite", [0, 1, 2])
def test_tiles_without_any_splat_over_a_coloured_background(renderer, composite):
    """The camera looks above the horizon: the upper screen tiles hold no pair at all and are written by the path that stores
    background-only tiles, in the video format like every other tile."""
    from gswt_renderer_amd import host, workloads
    W, Hh, _, su = _load_c3(renderer)
    cam = workloads.camera_for("c3")
    tgt = (cam["target"][0], cam["target"][1], cam["target"][2] + 0.2)
    cu = host.camera_uniforms(cam["pos"], tgt, cam["up"], cam["fovy"], cam["near"], cam["far"], W, Hh)[0]
    rng = np.random.default_rng(11)
    bg = rng.uniform(0.0, 1.0, size=(Hh, W, 4)).astype(np.float32)
    renderer.set_option(L.GSWT_OPT_COMPOSITE, composite)
    try:
        f32 = renderer.render(cu, su, W, Hh, bg_rgba=bg, transmittance_eps=1e-5)
        untouched = np.all(f32 == bg, axis=-1)                      # pixels no splat changed
        tiles = untouched[: Hh // 16 * 16, : W // 16 * 16].reshape(Hh // 16, 16, W // 16, 16).all(axis=(1, 3))
        assert tiles.sum() >= 100 and (~tiles).sum() >= 100, (int(tiles.sum()), tiles.size)   # both kinds of tile are on screen
        for fmt, ref in FORMATS:
            assert _same(renderer.render(cu, su, W, Hh, bg_rgba=bg, transmittance_eps=1e-5, out_format=fmt), ref(f32)), fmt
    finally:
        renderer.set_option(L.GSWT_OPT_COMPOSITE, 0)


@pytest.mark.parametrize("composite", [0, 1, 2])
def test_background_outside_unit_range_depth_buffer_and_depth_image(renderer, composite):
    W, Hh, cu, su = _load_c3(renderer)
    bg, depth = _bg(W, Hh)
    renderer.set_option(L.GSWT_OPT_COMPOSITE, composite)
    try:
        f32, z32 = renderer.render(cu, su, W, Hh, bg_rgba=bg, bg_depth=depth, transmittance_eps=1e-5, depth=True)
        assert (f32 < 0).any() and (f32 > 1).any() and np.isnan(f32).any()        # the clamp and the NaN rule are exercised
        for fmt, ref in FORMATS:
            planes = renderer.render(cu, su, W, Hh, bg_rgba=bg, bg_depth=depth, transmittance_eps=1e-5, out_format=fmt)
            assert _same(planes, ref(f32)), fmt
            # depth=True: the depth image follows the planes and is the f32 call's
            got = renderer.render(cu, su, W, Hh, bg_rgba=bg, bg_depth=depth, transmittance_eps=1e-5, out_format=fmt, depth=True)
            assert _same(got[:-1], ref(f32)), fmt
            assert got[-1].dtype == np.float32 and got[-1].shape == (Hh, W) and np.array_equal(got[-1], z32), fmt
    finally:
        renderer.set_option(L.GSWT_OPT_COMPOSITE, 0)


@pytest.mark.parametrize("fmt", [L.GSWT_VIDEO_NV12, L.GSWT_VIDEO_I420], ids=FMT_IDS)
def test_even_size_off_the_tile_grid_into_a_guarded_device_buffer(renderer, fmt):
    import torch
    pp = _load_grid(renderer)
    W, Hh = 330, 250                       # even, neither a multiple of 16 (nor of 4)
    cam = orc.default_camera(W, Hh).uniforms()
    su = orc.scene_uniforms(num_lod=pp.n_lod)
    bg, _ = _bg(W, Hh, seed=3)
    f32 = renderer.render(cam, su, W, Hh, bg_rgba=bg)
    assert np.nanmax(f32[..., 3]) > 0.0 and np.count_nonzero(np.isfinite(bg) & (f32 != bg)) > 1000      # splats are on screen
    want = FLAT[fmt](f32)
    n = W * Hh * 3 // 2
    assert want.size == n == renderer._lib.gswt_out_image_bytes(fmt, Hh, W)
    guard = 4096
    buf = torch.full((n + guard,), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    for composite in (0, 1, 2):
        renderer.set_option(L.GSWT_OPT_COMPOSITE, composite)
        try:
            buf[:n].fill_(0x5A)
            torch.cuda.synchronize()
            renderer.render(cam, su, W, Hh, bg_rgba=bg, out_device_ptr=buf.data_ptr(), out_format=fmt)
            renderer.synchronize()
        finally:
            renderer.set_option(L.GSWT_OPT_COMPOSITE, 0)
        host = buf.cpu().numpy()
        assert np.array_equal(host[:n], want), (composite, int(np.count_nonzero(host[:n] != want)))
        assert (host[n:] == 0xA5).all(), composite                      # nothing written past the last plane


@pytest.mark.parametrize("size", [(333, 188), (332, 187), (333, 187)], ids=["odd_width", "odd_height", "odd_both"])
@pytest.mark.parametrize("fmt", [L.GSWT_VIDEO_NV12, L.GSWT_VIDEO_I420], ids=FMT_IDS)
def test_odd_size_is_refused_and_writes_nothing(renderer, fmt, size):
    import torch
    pp = _load_grid(renderer)
    W, Hh = size
    cam = orc.default_camera(W, Hh).uniforms()
    su = orc.scene_uniforms(num_lod=pp.n_lod)
    buf = torch.full((Hh * W * 16,), 0x3C, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    with pytest.raises(GSWTError) as e:
        renderer.render(cam, su, W, Hh, out_device_ptr=buf.data_ptr(), out_format=fmt)
    assert e.value.code == L.GSWT_ERR_BAD_ARG
    with pytest.raises(GSWTError) as e:
        renderer.render_async(cam, su, W, Hh, buf.data_ptr(), out_format=fmt)
    assert e.value.code == L.GSWT_ERR_BAD_ARG
    with pytest.raises(GSWTError) as e:
        renderer.render(cam, su, W, Hh, out_format=fmt)                      # host output
    assert e.value.code == L.GSWT_ERR_BAD_ARG
    with pytest.raises(GSWTError) as e:
        renderer.unshard_format(buf.data_ptr(), W, Hh, 2, "rows", fmt, buf.data_ptr())
    assert e.value.code == L.GSWT_ERR_BAD_ARG
    renderer.synchronize()
    assert (buf.cpu().numpy() == 0x3C).all()
    # the renderer still renders afterwards, the same size as f32 and an even size as video
    assert renderer.render(cam, su, W, Hh)[..., 3].max() > 0.0
    W2, H2 = W + (W & 1), Hh + (Hh & 1)
    cam2 = orc.default_camera(W2, H2).uniforms()
    assert _same(renderer.render(cam2, su, W2, H2, out_format=fmt), dict(FORMATS)[fmt](renderer.render(cam2, su, W2, H2)))


@pytest.mark.parametrize("n", [3, 8])
@pytest.mark.parametrize("mode", ["rows", "cols"])
@pytest.mark.parametrize("fmt,ref", FORMATS, ids=FMT_IDS)
def test_shards_and_unshard_format(renderer, fmt, ref, mode, n):
    import torch
    W, Hh, cu, su = _load_c3(renderer)
    f32 = renderer.render(cu, su, W, Hh, transmittance_eps=1e-5)
    full = renderer.render(cu, su, W, Hh, transmittance_eps=1e-5, out_format=fmt)
    assert _same(full, ref(f32))
    shards = []
    for k in range(n):
        shard = (k, n, "cols") if mode == "cols" else (k, n)
        s32 = renderer.render(cu, su, W, Hh, transmittance_eps=1e-5, shard=shard)
        sv = renderer.render(cu, su, W, Hh, transmittance_eps=1e-5, shard=shard, out_format=fmt)
        assert sv[0].shape == s32.shape[:2]
        # a shard is itself a complete small image: the pixels it owns (its first rows / columns) are the reference of the f32
        # shard, its padding rows / columns are zero BYTES in every plane (not the code of a black pixel)
        rows_real, cols_real = s32.shape[0], s32.shape[1]
        if mode == "cols":
            cols_real = min(max(W - k * s32.shape[1], 0), s32.shape[1])
        else:
            rows_real = renderer._lib.gswt_shard_rows(Hh, k, n)
        assert rows_real % 2 == 0 and cols_real % 2 == 0
        want = [p.copy() for p in ref(s32)]
        want[0][rows_real:] = 0
        want[0][:, cols_real:] = 0
        for p in want[1:]:
            p[rows_real // 2:] = 0
            p[:, cols_real // 2:] = 0
        assert _same(sv, want), k
        shards.append(np.concatenate([p.reshape(-1) for p in sv]))
    assert all(s.size == renderer._lib.gswt_out_image_bytes(fmt, *s32.shape[:2]) for s in shards)
    gathered = torch.from_numpy(np.ascontiguousarray(np.concatenate(shards))).cuda()
    nbytes = W * Hh * 3 // 2
    out = torch.full((nbytes + 256,), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    renderer.unshard_format(gathered.data_ptr(), W, Hh, n, mode, fmt, out.data_ptr())
    renderer.synchronize()
    host = out.cpu().numpy()
    assert _same(video_planes(host, fmt, Hh, W), full)
    assert (host[nbytes:] == 0xA5).all()


@pytest.mark.parametrize("mode", ["cols", "rows"])
def test_group_gather_three_ranks_video(mode):
    import torch
    n = 3
    rs = [GSWTRenderer(0) for _ in range(n)]
    try:
        pp = None
        for r in rs:
            pp = _load_grid(r)
        W, Hh = 200, 120
        cam = orc.default_camera(W, Hh).uniforms()
        su = orc.scene_uniforms(num_lod=pp.n_lod)
        want32 = rs[0].render(cam, su, W, Hh)
        GSWTRenderer.group_init(rs)
        shard_hw = (Hh, rs[0].shard_cols_padded(W, n)) if mode == "cols" else (rs[0].shard_rows_padded(Hh, n), W)
        shard = lambda k: (k, n, "cols") if mode == "cols" else (k, n)
        for fmt, ref in FORMATS:
            outs = [torch.zeros((shard_hw[0] * shard_hw[1] * 3 // 2,), dtype=torch.uint8, device="cuda") for _ in range(n)]
            frames = [torch.zeros((Hh * W * 3 // 2,), dtype=torch.uint8, device="cuda") for _ in range(n)]
            torch.cuda.synchronize()
            tickets = [r.render_async(cam, su, W, Hh, o.data_ptr(), shard=shard(k), out_format=fmt) for k, (r, o) in enumerate(zip(rs, outs))]
            GSWTRenderer.group_render_gather(rs, tickets, [f.data_ptr() for f in frames])
            for r, t in zip(rs, tickets):
                r.render_wait(t)
                r.synchronize()
            for f in frames:
                assert _same(video_planes(f.cpu().numpy(), fmt, Hh, W), ref(want32)), fmt
    finally:
        for r in rs:
            r.comm_destroy()
            r.close()


def test_async_frames_in_flight_through_the_graph_alternating_formats(renderer):
    """Every slot replays its graph with the format changing between its frames (f32, NV12, RGBA8, I420: another compositor /
    k_combine function, the slot's graph is rebuilt), neighbouring frames in flight differ in format, and each frame equals its
    own reference."""
    import torch
    from gswt_renderer_amd import host, workloads
    W, Hh, _, su = _load_c3(renderer)
    cam = workloads.camera_for("c3")
    slots = renderer.frame_slots()
    n_rounds = 4
    cams = [host.camera_uniforms((cam["pos"][0] + 0.15 * k, cam["pos"][1] + 0.2 * k, cam["pos"][2]),
                                 (cam["target"][0] + 0.15 * k, cam["target"][1] + 0.2 * k, cam["target"][2]),
                                 cam["up"], cam["fovy"], cam["near"], cam["far"], W, Hh)[0] for k in range(slots)]
    wants = [renderer.render(c, su, W, Hh, transmittance_eps=1e-5) for c in cams]
    cycle = [L.GSWT_OUT_RGBA32F, L.GSWT_VIDEO_NV12, L.GSWT_OUT_RGBA8_UNORM, L.GSWT_VIDEO_I420]
    flat = {L.GSWT_OUT_RGBA32F: lambda a: a.reshape(-1).view(np.uint8), L.GSWT_OUT_RGBA8_UNORM: lambda a: rgba8(a).reshape(-1), **FLAT}
    renderer.set_option(L.GSWT_OPT_TIMING, 0)
    renderer.set_option(L.GSWT_OPT_GRAPH, 1)
    try:
        stats0 = renderer.graph_stats()
        for rnd in range(n_rounds):
            fmts = [cycle[(k + rnd) % 4] for k in range(slots)]
            sizes = [int(renderer._lib.gswt_out_image_bytes(f, Hh, W)) for f in fmts]
            outs = [torch.full((s + 64,), 0x5A, dtype=torch.uint8, device="cuda") for s in sizes]
            torch.cuda.synchronize()
            tickets = [renderer.render_async(c, su, W, Hh, o.data_ptr(), transmittance_eps=1e-5, out_format=f) for c, o, f in zip(cams, outs, fmts)]
            for t in tickets:
                renderer.render_wait(t)
            renderer.synchronize()
            for k, (o, f, s) in enumerate(zip(outs, fmts, sizes)):
                got = o.cpu().numpy()
                assert np.array_equal(got[:s], flat[f](wants[k])), (rnd, k, f)
                assert (got[s:] == 0x5A).all(), (rnd, k, f)
        stats = renderer.graph_stats()
        assert stats[0] - stats0[0] >= n_rounds * slots          # every frame went through hipGraphLaunch (a re-run adds one)
    finally:
        renderer.set_option(L.GSWT_OPT_GRAPH, 0)
        renderer.set_option(L.GSWT_OPT_TIMING, 2)


@pytest.mark.parametrize("fmt,ref", FORMATS, ids=FMT_IDS)
def test_host_output(renderer, fmt, ref):
    """out_on_device = 0: the library's staging buffer and its device-to-host copy are sized from the format."""
    W, Hh, cu, su = _load_c3(renderer)
    f32 = renderer.render(cu, su, W, Hh)
    planes = renderer.render(cu, su, W, Hh, out_format=fmt)
    assert sum(p.nbytes for p in planes) == W * Hh * 3 // 2
    assert _same(planes, ref(f32))
    again = renderer.render(cu, su, W, Hh)                     # and back: the f32 frame after a video one is unchanged
    assert np.array_equal(again, f32)


@pytest.mark.parametrize("fmt,ref", FORMATS, ids=FMT_IDS)
def test_pair_buffer_overflow_rerun(renderer, fmt, ref):
    W, Hh, cu, su = _load_c3(renderer)
    f32 = renderer.render(cu, su, W, Hh, transmittance_eps=1e-5)
    renderer.set_option(L.GSWT_OPT_PAIR_CAP, 4096)
    try:
        planes = renderer.render(cu, su, W, Hh, transmittance_eps=1e-5, out_format=fmt)
        assert renderer.timings()["n_pairs"] > 4096                  # the frame overflowed the pinned capacity and was re-run
    finally:
        renderer.set_option(L.GSWT_OPT_PAIR_CAP, 0)
    assert _same(planes, ref(f32))                                   # the re-run rewrote every plane


def test_nv12_and_i420_hold_the_same_samples(renderer):
    W, Hh, cu, su = _load_c3(renderer)
    bg, _ = _bg(W, Hh, seed=5)
    y1, cbcr = renderer.render(cu, su, W, Hh, bg_rgba=bg, transmittance_eps=1e-5, out_format=L.GSWT_VIDEO_NV12)
    y2, cb, cr = renderer.render(cu, su, W, Hh, bg_rgba=bg, transmittance_eps=1e-5, out_format=L.GSWT_VIDEO_I420)
    assert np.array_equal(y1, y2) and np.array_equal(cbcr[..., 0], cb) and np.array_equal(cbcr[..., 1], cr)
    assert y1.min() >= 16 and y1.max() <= 235 and cbcr.min() >= 16 and cbcr.max() <= 240
    assert len(np.unique(cb)) > 8 and len(np.unique(cr)) > 8         # a picture, not a constant
