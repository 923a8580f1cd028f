"""Frames rendered straight into the 8-bit display formats (GSWT_OUT_RGBA8_UNORM / GSWT_OUT_BGRA8_UNORM, include/gswt_hip.h).
Every case renders the same inputs twice, once as RGBA f32 and once in 8 bits, and requires the 8-bit image to be q(f32 image)
EXACTLY (tests/unorm8_ref.py), BGRA as the channel swap of that: every compositor variant and order, the early-out, a background
colour with values outside [0, 1] and a depth buffer, a frame size that is not a multiple of the 16-px tile (guard bytes behind
the image stay untouched), row and column shards with gswt_unshard_format, the peer-copy group gather, asynchronous frames in
flight through the graph path with the format changing from frame to frame, host output, a pair-buffer overflow re-run, and
the refusal of unknown formats."""
import ctypes as C
import functools

import numpy as np
import pytest

from gswt_renderer_amd import _lib as L
from gswt_renderer_amd.renderer import GSWTError, GSWTRenderer
from oracle import gswt_oracle as orc
from tests import helpers as H
from tests.unorm8_ref import bgra8, rgba8

pytestmark = pytest.mark.gpu

FORMATS = [(L.GSWT_OUT_RGBA8_UNORM, rgba8), (L.GSWT_OUT_BGRA8_UNORM, bgra8)]
FMT_IDS = ["rgba8", "bgra8"]


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
                u8 = renderer.render(cu, su, W, Hh, out_format=fmt, **kw)
                assert u8.dtype == np.uint8 and u8.shape == (Hh, W, 4)
                assert np.array_equal(u8, ref(f32)), (fmt, eps, int(np.count_nonzero(u8 != ref(f32))))
    finally:
        renderer.set_option(L.GSWT_OPT_COMPOSITE, 0)


@pytest.mark.parametrize("composite", [0, 1, 2])
def test_background_outside_unit_range_and_depth_buffer(renderer, composite):
    W, Hh, cu, su = _load_c3(renderer)
    bg, depth = _bg(W, Hh)
    renderer.set_option(L.GSWT_OPT_COMPOSITE, composite)
    try:
        f32 = renderer.render(cu, su, W, Hh, bg_rgba=bg, bg_depth=depth, transmittance_eps=1e-5)
        assert (f32 < 0).any() and (f32 > 1).any() and np.isnan(f32).any()        # the clamp and the NaN rule are exercised
        for fmt, ref in FORMATS:
            u8 = renderer.render(cu, su, W, Hh, bg_rgba=bg, bg_depth=depth, transmittance_eps=1e-5, out_format=fmt)
            assert np.array_equal(u8, ref(f32)), fmt
    finally:
        renderer.set_option(L.GSWT_OPT_COMPOSITE, 0)


@pytest.mark.parametrize("fmt,ref", FORMATS, ids=FMT_IDS)
def test_odd_frame_size_into_a_guarded_device_buffer(renderer, fmt, ref):
    import torch
    pp = _load_grid(renderer)
    W, Hh = 333, 187
    cam = orc.default_camera(W, Hh).uniforms()
    su = orc.scene_uniforms(num_lod=pp.n_lod)
    bg, _ = _bg(W, Hh, seed=3)
    f32 = renderer.render(cam, su, W, Hh, bg_rgba=bg)
    guard = 4096
    buf = torch.full((Hh * W * 4 + guard,), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    for composite in (0, 1, 2):
        renderer.set_option(L.GSWT_OPT_COMPOSITE, composite)
        try:
            buf[: Hh * W * 4].fill_(0x5A)
            torch.cuda.synchronize()
            renderer.render(cam, su, W, Hh, bg_rgba=bg, out_device_ptr=buf.data_ptr(), out_format=fmt)
            renderer.synchronize()
        finally:
            renderer.set_option(L.GSWT_OPT_COMPOSITE, 0)
        host = buf.cpu().numpy()
        assert np.array_equal(host[: Hh * W * 4].reshape(Hh, W, 4), ref(f32)), composite
        assert (host[Hh * W * 4:] == 0xA5).all(), composite                     # nothing written past rows * W * 4 bytes


@pytest.mark.parametrize("mode", ["rows", "cols"])
@pytest.mark.parametrize("fmt,ref", FORMATS, ids=FMT_IDS)
def test_shards_and_unshard_format(renderer, fmt, ref, mode):
    import torch
    W, Hh, cu, su = _load_c3(renderer)
    n = 3
    full = renderer.render(cu, su, W, Hh, transmittance_eps=1e-5, out_format=fmt)
    assert np.array_equal(full, ref(renderer.render(cu, su, W, Hh, transmittance_eps=1e-5)))
    shards = []
    for k in range(n):
        shard = (k, n, "cols") if mode == "cols" else (k, n)
        s32 = renderer.render(cu, su, W, Hh, transmittance_eps=1e-5, shard=shard)
        s8 = renderer.render(cu, su, W, Hh, transmittance_eps=1e-5, shard=shard, out_format=fmt)
        assert s8.dtype == np.uint8 and s8.shape == s32.shape
        assert np.array_equal(s8, ref(s32)), k
        shards.append(s8)
    gathered = torch.from_numpy(np.ascontiguousarray(np.concatenate(shards, axis=0))).cuda()
    out = torch.zeros((Hh, W, 4), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    renderer.unshard_format(gathered.data_ptr(), W, Hh, n, mode, fmt, out.data_ptr())
    renderer.synchronize()
    assert np.array_equal(out.cpu().numpy(), full)


@pytest.mark.parametrize("mode", ["cols", "rows"])
def test_group_gather_three_ranks_8bit(mode):
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
            outs = [torch.zeros(shard_hw + (4,), dtype=torch.uint8, device="cuda") for _ in range(n)]
            frames = [torch.zeros((Hh, W, 4), dtype=torch.uint8, device="cuda") for _ in range(n)]
            torch.cuda.synchronize()
            tickets = [r.render_async(cam, su, W, Hh, o.data_ptr(), shard=shard(k), out_format=fmt) for k, (r, o) in enumerate(zip(rs, outs))]
            GSWTRenderer.group_render_gather(rs, tickets, [f.data_ptr() for f in frames])
            for r, t in zip(rs, tickets):
                r.render_wait(t)
                r.synchronize()
            for f in frames:
                assert np.array_equal(f.cpu().numpy(), ref(want32)), fmt
        # ranks whose frames differ in format: refused
        outs = [torch.zeros(shard_hw + (4,), dtype=torch.float32, device="cuda") for _ in range(n)]
        frames = [torch.zeros((Hh, W, 4), dtype=torch.float32, device="cuda") for _ in range(n)]
        torch.cuda.synchronize()
        fmts = [L.GSWT_OUT_RGBA32F, L.GSWT_OUT_RGBA8_UNORM, L.GSWT_OUT_RGBA32F]
        tickets = [r.render_async(cam, su, W, Hh, o.data_ptr(), shard=shard(k), out_format=f) for k, (r, o, f) in enumerate(zip(rs, outs, fmts))]
        arr = (C.c_void_p * n)(*[r._h for r in rs])
        rc = L.load().gswt_group_render_gather(arr, (C.c_int * n)(*tickets), (C.c_void_p * n)(*[f.data_ptr() for f in frames]), n)
        assert rc == L.GSWT_ERR_BAD_ARG
        assert "out_format" in rs[1]._lib.gswt_last_error(rs[1]._h).decode()
        for r, t in zip(rs, tickets):
            r.render_wait(t)
            r.synchronize()
    finally:
        for r in rs:
            r.comm_destroy()
            r.close()


def test_async_frames_in_flight_through_the_graph_alternating_formats(renderer):
    """Every slot replays its graph with the format changing between its frames (another compositor / k_combine function: the
    slot's graph is rebuilt), neighbouring frames in flight differ in format, and each frame equals its own reference."""
    import torch
    from gswt_renderer_amd import host, workloads
    W, Hh, _, su = _load_c3(renderer)
    cam = workloads.camera_for("c3")
    slots = renderer.frame_slots()
    n_rounds = 3
    cams = [host.camera_uniforms((cam["pos"][0] + 0.15 * k, cam["pos"][1] + 0.2 * k, cam["pos"][2]),
                                 (cam["target"][0] + 0.15 * k, cam["target"][1] + 0.2 * k, cam["target"][2]),
                                 cam["up"], cam["fovy"], cam["near"], cam["far"], W, Hh)[0] for k in range(slots)]
    wants = [renderer.render(c, su, W, Hh, transmittance_eps=1e-5) for c in cams]
    renderer.set_option(L.GSWT_OPT_TIMING, 0)
    renderer.set_option(L.GSWT_OPT_GRAPH, 1)
    try:
        stats0 = renderer.graph_stats()
        for rnd in range(n_rounds):
            fmts = [[L.GSWT_OUT_RGBA32F, L.GSWT_OUT_RGBA8_UNORM, L.GSWT_OUT_RGBA32F, L.GSWT_OUT_BGRA8_UNORM][(k + rnd) % 4] for k in range(slots)]
            outs = [torch.full((Hh, W, 4), -1.0, dtype=torch.float32, device="cuda") if f == L.GSWT_OUT_RGBA32F
                    else torch.full((Hh, W, 4), 0x5A, dtype=torch.uint8, device="cuda") for f in fmts]
            torch.cuda.synchronize()
            tickets = [renderer.render_async(c, su, W, Hh, o.data_ptr(), transmittance_eps=1e-5, out_format=f) for c, o, f in zip(cams, outs, fmts)]
            for t in tickets:
                renderer.render_wait(t)
            renderer.synchronize()
            for k, (o, f) in enumerate(zip(outs, fmts)):
                got = o.cpu().numpy()
                want = wants[k] if f == L.GSWT_OUT_RGBA32F else (rgba8 if f == L.GSWT_OUT_RGBA8_UNORM else bgra8)(wants[k])
                assert np.array_equal(got, want), (rnd, k, f)
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
    u8 = renderer.render(cu, su, W, Hh, out_format=fmt)
    assert u8.nbytes == W * Hh * 4
    assert np.array_equal(u8, ref(f32))
    again = renderer.render(cu, su, W, Hh)                     # and back: the f32 frame after an 8-bit one is unchanged
    assert np.array_equal(again, f32)


@pytest.mark.parametrize("fmt,ref", FORMATS, ids=FMT_IDS)
def test_pair_buffer_overflow_rerun(renderer, fmt, ref):
    W, Hh, cu, su = _load_c3(renderer)
    f32 = renderer.render(cu, su, W, Hh, transmittance_eps=1e-5)
    renderer.set_option(L.GSWT_OPT_PAIR_CAP, 4096)
    try:
        u8 = renderer.render(cu, su, W, Hh, transmittance_eps=1e-5, out_format=fmt)
        assert renderer.timings()["n_pairs"] > 4096                  # the frame overflowed the pinned capacity and was re-run
    finally:
        renderer.set_option(L.GSWT_OPT_PAIR_CAP, 0)
    assert np.array_equal(u8, ref(f32))


@pytest.mark.parametrize("bad", [3, 0xFFFFFFFF])
def test_unknown_format_is_refused_and_writes_nothing(renderer, bad):
    import torch
    pp = _load_grid(renderer)
    W, Hh = 64, 48
    cam = orc.default_camera(W, Hh).uniforms()
    su = orc.scene_uniforms(num_lod=pp.n_lod)
    buf = torch.full((Hh * W * 16,), 0x3C, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    with pytest.raises(GSWTError) as e:
        renderer.render(cam, su, W, Hh, out_device_ptr=buf.data_ptr(), out_format=bad)
    assert e.value.code == L.GSWT_ERR_BAD_ARG
    with pytest.raises(GSWTError) as e:
        renderer.render_async(cam, su, W, Hh, buf.data_ptr(), out_format=bad)
    assert e.value.code == L.GSWT_ERR_BAD_ARG
    with pytest.raises(GSWTError) as e:
        renderer.render(cam, su, W, Hh, out_format=bad)                      # host output
    assert e.value.code == L.GSWT_ERR_BAD_ARG
    renderer.synchronize()
    assert (buf.cpu().numpy() == 0x3C).all()
    with pytest.raises(GSWTError) as e:
        renderer.unshard_format(buf.data_ptr(), W, Hh, 1, "rows", bad, buf.data_ptr())
    # the renderer still renders afterwards
    assert renderer.render(cam, su, W, Hh)[..., 3].max() > 0.0
