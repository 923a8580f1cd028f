"""What the GPU tests of the frame's outputs share: the display formats (tests/test_out_format_gpu.py: RGBA8 / BGRA8,
tests/test_video_out_gpu.py: NV12 / I420) and the side images (tests/test_depth_out_gpu.py, tests/test_pick_gpu.py), on the bench
workloads (`workload`) and the grid case (`load_grid`).

A plain module in the style of tests/frame_modes.py: scenes and inputs once, one descriptor (`ColourFormat`: what differs between
display formats), one function per shared check.  A display-format frame has to EQUAL its reference of the f32 frame (`same_planes`);
a side image has to equal itself byte for byte however the frame was run (`frame_modes.same`)."""
import ctypes as C
import functools
from dataclasses import dataclass
from types import SimpleNamespace
from typing import Callable

import numpy as np
import pytest

from gswt_renderer_amd import _lib as L
from gswt_renderer_amd.renderer import GSWTError, GSWTRenderer, video_planes
from oracle import gswt_oracle as orc
from tests import frame_modes as FM
from tests import helpers as H
from tests import unorm8_ref as U8
from tests import yuv_ref as YUV


# ---- scenes and inputs ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=2)
def workload(name):
    """bench.build_workload(name), kept for the tests that follow: frame size, scene, camera block, view-projection, sort data, scene
    block and the height map of a HeightMap surface.  Shared: not to be changed."""
    import bench
    w, wang, cu, vp, sort = bench.build_workload(name)
    hm = wang.height_map() if int(wang.user.surface_type) == 1 else None
    return dict(name=name, W=w["width"], H=w["height"], wang=wang, cu=cu, vp=vp, sort=sort, su=wang.scene_uniforms(), hm=hm)


def bind_workload(renderer, s):
    """Uploads the workload's scene, surface and draw list; returns (W, H, camera block, scene block)."""
    s["wang"].upload_to(renderer)
    renderer.configure(s["hm"])
    renderer.set_draws(s["sort"].draws, s["sort"].merged_gs_index, s["sort"].merged_map_id, s["sort"].merged_lod_id)
    return s["W"], s["H"], s["cu"], s["su"]


def load_grid(renderer):
    pp = H.tileset()
    renderer.upload_scene(pp.tex, pp.gs_index, pp.gs_lod_id)
    renderer.configure(None)
    renderer.set_draws(H.grid_case(pp).draws)
    return pp


def grid_view(pp, W, Hh):
    return orc.default_camera(W, Hh).uniforms(), orc.scene_uniforms(num_lod=pp.n_lod)


def hostile_bg(W, Hh, seed=7):
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


def bg_depth(W, Hh):
    return np.random.default_rng(3).uniform(0.99, 1.0, size=(Hh, W)).astype(np.float32)


def path_cameras(name, n):
    """n camera blocks along a short walk from the workload's camera: frame k is moved by (0.15 k, 0.2 k, 0)."""
    from gswt_renderer_amd import host, workloads
    s, cam = workload(name), workloads.camera_for(name)
    return [host.camera_uniforms((cam["pos"][0] + 0.15 * k, cam["pos"][1] + 0.2 * k, cam["pos"][2]),
                                 (cam["target"][0] + 0.15 * k, cam["target"][1] + 0.2 * k, cam["target"][2]),
                                 cam["up"], cam["fovy"], cam["near"], cam["far"], s["W"], s["H"])[0] for k in range(n)]


# ---- comparison ----------------------------------------------------------------------------------------------------------------------------
def same_planes(got, want):
    """Plane tuples equal in count, shape, type and every byte; on a mismatch the message says which plane and how many samples."""
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == np.uint8 and g.shape == w.shape, (k, g.dtype, g.shape, w.shape)
        assert np.array_equal(g, w), (k, int(np.count_nonzero(g != w)), g.size)
    return True


def same_image(got, want):
    """same_planes for a frame that is one array of bytes."""
    return same_planes((got,), (want,))


def split_guard(buf, n):
    """(the first n bytes, what lies behind them) of a flat buffer that was allocated with guard bytes behind the image."""
    assert buf.ndim == 1 and buf.dtype == np.uint8 and 0 <= n <= buf.size
    return buf[:n], buf[n:]


# ---- a display format ------------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class ColourFormat:
    name: str
    fmt: int                    # GSWT_OUT_* / GSWT_VIDEO_*
    ref: Callable               # the f32 image -> the frame as GSWTRenderer.render returns it (an array, or a tuple of planes)
    flat: Callable              # the f32 image -> the frame's bytes as a device buffer holds them
    same: Callable              # same(got, want) of two returned frames
    nbytes: Callable            # (rows, cols) -> what gswt_out_image_bytes has to say
    unflat: Callable            # (bytes, rows, cols) -> the frame as render returns it
    check_shape: Callable       # (frame, rows, cols): the shape checks of a returned frame
    zero_pad: Callable          # (frame, rows, cols) -> a copy with everything beyond the first rows / cols zero BYTES

    def image_bytes(self, renderer, rows, cols):
        n = self.nbytes(rows, cols)
        assert n == renderer._lib.gswt_out_image_bytes(self.fmt, rows, cols)
        return n

    def bytes_of(self, frame):
        return np.concatenate([np.ascontiguousarray(p).reshape(-1).view(np.uint8) for p in (frame if isinstance(frame, (tuple, list)) else (frame,))])


def _array_shape(dtype):
    def check(frame, rows, cols):
        assert frame.dtype == dtype and frame.shape == (rows, cols, 4)
    return check


def _array_pad(frame, rows, cols):
    out = frame.copy()
    out[rows:] = 0
    out[:, cols:] = 0
    return out


def _plane_shape(planes, rows, cols):
    assert planes[0].shape == (rows, cols) and all(p.shape[:2] == (rows // 2, cols // 2) for p in planes[1:])


def _plane_pad(planes, rows, cols):
    assert rows % 2 == 0 and cols % 2 == 0
    out = [p.copy() for p in planes]
    out[0][rows:] = 0
    out[0][:, cols:] = 0
    for p in out[1:]:
        p[rows // 2:] = 0
        p[:, cols // 2:] = 0
    return out


def _u8(name, fmt, ref):
    return ColourFormat(name, fmt, ref, lambda a: ref(a).reshape(-1), same_image, lambda r, c: r * c * 4,
                        lambda b, r, c: b.reshape(r, c, 4), _array_shape(np.uint8), _array_pad)


def _video(name, fmt, ref, flat):
    return ColourFormat(name, fmt, ref, flat, same_planes, lambda r, c: r * c * 3 // 2, lambda b, r, c: video_planes(b, fmt, r, c), _plane_shape, _plane_pad)


F32 = ColourFormat("f32", L.GSWT_OUT_RGBA32F, lambda a: a, lambda a: a.reshape(-1).view(np.uint8), FM.same, lambda r, c: r * c * 16,
                   lambda b, r, c: b.view(np.float32).reshape(r, c, 4), _array_shape(np.float32), _array_pad)
RGBA8, BGRA8 = _u8("rgba8", L.GSWT_OUT_RGBA8_UNORM, U8.rgba8), _u8("bgra8", L.GSWT_OUT_BGRA8_UNORM, U8.bgra8)
NV12, I420 = _video("nv12", L.GSWT_VIDEO_NV12, YUV.nv12, YUV.nv12_bytes), _video("i420", L.GSWT_VIDEO_I420, YUV.i420, YUV.i420_bytes)
BY_ID = {cf.fmt: cf for cf in (F32, RGBA8, BGRA8, NV12, I420)}


# ---- the checks the display formats share --------------------------------------------------------------------------------------------------
def check_every_compositor_and_order(renderer, formats, composite, order):
    W, Hh, cu, su = bind_workload(renderer, workload("c3"))
    with renderer.options(COMPOSITE=composite):
        for eps in (0.0, 1e-5):
            kw = dict(transmittance_eps=eps, order_mode=order)
            f32 = renderer.render(cu, su, W, Hh, **kw)
            assert f32.dtype == np.float32 and f32[..., 3].max() > 0.5
            for cf in formats:
                got = renderer.render(cu, su, W, Hh, out_format=cf.fmt, **kw)
                cf.check_shape(got, Hh, W)
                assert cf.same(got, cf.ref(f32)), (cf.name, eps)


def check_hostile_background(renderer, formats, composite, tail=None):
    """A background with values outside [0, 1], NaN and inf, and a proxy depth buffer.  tail(cf, f32, render), when given, runs
    behind every format's check under the same compositor; render(**kw) is a frame over the same inputs."""
    W, Hh, cu, su = bind_workload(renderer, workload("c3"))
    bg, depth = hostile_bg(W, Hh)
    render = lambda **kw: renderer.render(cu, su, W, Hh, bg_rgba=bg, bg_depth=depth, transmittance_eps=1e-5, **kw)
    with renderer.options(COMPOSITE=composite):
        f32 = render()
        assert (f32 < 0).any() and (f32 > 1).any() and np.isnan(f32).any()        # the clamp and the NaN rule are exercised
        for cf in formats:
            assert cf.same(render(out_format=cf.fmt), cf.ref(f32)), cf.name
            if tail is not None:
                tail(cf, f32, render)


def check_guarded_device_buffer(renderer, cf, W, Hh):
    """A frame size off the 16-px tile grid into a device buffer with guard bytes behind it, under every compositor."""
    import torch
    pp = load_grid(renderer)
    cam, su = grid_view(pp, W, Hh)
    bg, _ = hostile_bg(W, Hh, seed=3)
    f32 = renderer.render(cam, su, W, Hh, bg_rgba=bg)
    assert np.nanmax(f32[..., 3]) > 0.0 and np.count_nonzero(np.isfinite(bg) & (f32 != bg)) > 1000      # splats are on screen
    want = cf.flat(f32)
    n = cf.image_bytes(renderer, Hh, W)
    assert want.size == n
    buf = torch.full((n + 4096,), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    for composite in (0, 1, 2):
        with renderer.options(COMPOSITE=composite):
            buf[:n].fill_(0x5A)
            torch.cuda.synchronize()
            renderer.render(cam, su, W, Hh, bg_rgba=bg, out_device_ptr=buf.data_ptr(), out_format=cf.fmt)
            renderer.synchronize()
        image, guard = split_guard(buf.cpu().numpy(), n)
        assert np.array_equal(image, want), (composite, int(np.count_nonzero(image != want)))
        assert (guard == 0xA5).all(), composite                          # nothing written past the image's last byte


def check_shards_and_unshard(renderer, cf, mode, n):
    import torch
    W, Hh, cu, su = bind_workload(renderer, workload("c3"))
    f32 = renderer.render(cu, su, W, Hh, transmittance_eps=1e-5)
    full = renderer.render(cu, su, W, Hh, transmittance_eps=1e-5, out_format=cf.fmt)
    assert cf.same(full, cf.ref(f32))
    shards = []
    for k in range(n):
        shard = (k, n, "cols") if mode == "cols" else (k, n)
        s32 = renderer.render(cu, su, W, Hh, transmittance_eps=1e-5, shard=shard)
        got = renderer.render(cu, su, W, Hh, transmittance_eps=1e-5, shard=shard, out_format=cf.fmt)
        rows, cols = s32.shape[:2]
        cf.check_shape(got, rows, cols)
        # a shard is itself a complete small image: the pixels it owns (its first rows / columns) are the reference of the f32
        # shard, its padding rows / columns are zero BYTES (in every plane; not the code of a black pixel)
        rows_real, cols_real = rows, cols
        if mode == "cols":
            cols_real = min(max(W - k * cols, 0), cols)
        else:
            rows_real = renderer._lib.gswt_shard_rows(Hh, k, n)
        assert cf.same(got, cf.zero_pad(cf.ref(s32), rows_real, cols_real)), k
        shards.append(cf.bytes_of(got))
    assert all(s.size == cf.image_bytes(renderer, rows, cols) for s in shards)
    gathered = torch.from_numpy(np.ascontiguousarray(np.concatenate(shards))).cuda()
    nbytes = cf.image_bytes(renderer, Hh, W)
    out = torch.full((nbytes + 256,), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    renderer.unshard_format(gathered.data_ptr(), W, Hh, n, mode, cf.fmt, out.data_ptr())
    renderer.synchronize()
    image, guard = split_guard(out.cpu().numpy(), nbytes)
    assert cf.same(cf.unflat(image, Hh, W), full)
    assert (guard == 0xA5).all()


def check_group_gather_three_ranks(formats, mode, tail=None):
    """Three contexts on one device render a shard each and gather the frame with peer copies: every rank's frame is the reference of
    the f32 frame.  tail(rs, submit, wait), when given, runs on the same group afterwards; submit(fmts) queues one shard per rank in
    the formats given, into buffers that would hold the largest of them, and returns (tickets, frame buffers); wait(tickets)."""
    import torch
    n = 3
    rs = [GSWTRenderer(0) for _ in range(n)]
    try:
        for r in rs:
            pp = load_grid(r)
        W, Hh = 200, 120
        cam, su = grid_view(pp, W, Hh)
        want32 = rs[0].render(cam, su, W, Hh)
        GSWTRenderer.group_init(rs)
        shard_hw = (Hh, rs[0].shard_cols_padded(W, n)) if mode == "cols" else (rs[0].shard_rows_padded(Hh, n), W)
        shard = lambda k: (k, n, "cols") if mode == "cols" else (k, n)

        def submit(fmts):
            size = lambda rows, cols: max(BY_ID[f].nbytes(rows, cols) for f in fmts)
            outs = [torch.zeros((size(*shard_hw),), dtype=torch.uint8, device="cuda") for _ in fmts]
            frames = [torch.zeros((size(Hh, W),), dtype=torch.uint8, device="cuda") for _ in fmts]
            torch.cuda.synchronize()
            return [r.render_async(cam, su, W, Hh, o.data_ptr(), shard=shard(k), out_format=f) for k, (r, o, f) in enumerate(zip(rs, outs, fmts))], frames

        def wait(tickets):
            for r, t in zip(rs, tickets):
                r.render_wait(t)
                r.synchronize()

        for cf in formats:
            tickets, frames = submit([cf.fmt] * n)
            GSWTRenderer.group_render_gather(rs, tickets, [f.data_ptr() for f in frames])
            wait(tickets)
            for f in frames:
                assert cf.same(cf.unflat(f.cpu().numpy(), Hh, W), cf.ref(want32)), cf.name
        if tail is not None:
            tail(rs, submit, wait)
    finally:
        for r in rs:
            r.comm_destroy()
            r.close()


def check_in_flight_alternating_formats(renderer, cycle, n_rounds):
    """Every slot replays its graph with the format changing between its frames along `cycle` (another compositor / k_combine
    function: the slot's graph is rebuilt), neighbouring frames in flight differ in format, each frame equals its own reference and
    leaves the guard bytes behind it alone."""
    import torch
    W, Hh, _, su = bind_workload(renderer, workload("c3"))
    slots = renderer.frame_slots()
    cams = path_cameras("c3", slots)
    wants = [renderer.render(c, su, W, Hh, transmittance_eps=1e-5) for c in cams]
    with renderer.options(TIMING=0, GRAPH=1):
        stats0 = renderer.graph_stats()
        for rnd in range(n_rounds):
            fmts = [BY_ID[cycle[(k + rnd) % len(cycle)]] for k in range(slots)]
            sizes = [cf.image_bytes(renderer, Hh, W) for cf in fmts]
            outs = [torch.full((s + 64,), 0x5A, dtype=torch.uint8, device="cuda") for s in sizes]
            torch.cuda.synchronize()
            tickets = [renderer.render_async(c, su, W, Hh, o.data_ptr(), transmittance_eps=1e-5, out_format=cf.fmt) for c, o, cf in zip(cams, outs, fmts)]
            for t in tickets:
                renderer.render_wait(t)
            renderer.synchronize()
            for k, (o, cf, s) in enumerate(zip(outs, fmts, sizes)):
                image, guard = split_guard(o.cpu().numpy(), s)
                assert np.array_equal(image, cf.flat(wants[k])), (rnd, k, cf.name)
                assert (guard == 0x5A).all(), (rnd, k, cf.name)
        stats = renderer.graph_stats()
        assert stats[0] - stats0[0] >= n_rounds * slots          # every frame went through hipGraphLaunch (a re-run adds one)


def check_host_output(renderer, cf):
    """out_on_device = 0: the library's staging buffer and its device-to-host copy are sized from the format."""
    W, Hh, cu, su = bind_workload(renderer, workload("c3"))
    f32 = renderer.render(cu, su, W, Hh)
    got = renderer.render(cu, su, W, Hh, out_format=cf.fmt)
    assert cf.bytes_of(got).size == cf.image_bytes(renderer, Hh, W)
    assert cf.same(got, cf.ref(f32))
    again = renderer.render(cu, su, W, Hh)                     # and back: the f32 frame after one in the format is unchanged
    assert np.array_equal(again, f32)


def check_overflow_rerun(renderer, cf):
    W, Hh, cu, su = bind_workload(renderer, workload("c3"))
    f32 = renderer.render(cu, su, W, Hh, transmittance_eps=1e-5)
    with renderer.options(PAIR_CAP=4096):
        got = renderer.render(cu, su, W, Hh, transmittance_eps=1e-5, out_format=cf.fmt)
        assert renderer.timings()["n_pairs"] > 4096                  # the frame overflowed the pinned capacity and was re-run
    assert cf.same(got, cf.ref(f32))                                 # the re-run rewrote the whole image


def check_refused_and_nothing_written(renderer, fmt, W, Hh, n_unshard):
    """A W x Hh frame in `fmt` is refused with GSWT_ERR_BAD_ARG on every path -- device output, asynchronous, host output,
    gswt_unshard_format -- no byte of the buffer changes, and the context still renders.  Returns (camera block, scene block)."""
    import torch
    pp = load_grid(renderer)
    cam, su = grid_view(pp, W, Hh)
    buf = torch.full((Hh * W * 16,), 0x3C, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    for call in (lambda: renderer.render(cam, su, W, Hh, out_device_ptr=buf.data_ptr(), out_format=fmt),
                 lambda: renderer.render_async(cam, su, W, Hh, buf.data_ptr(), out_format=fmt),
                 lambda: renderer.render(cam, su, W, Hh, out_format=fmt),                      # host output
                 lambda: renderer.unshard_format(buf.data_ptr(), W, Hh, n_unshard, "rows", fmt, buf.data_ptr())):
        with pytest.raises(GSWTError) as e:
            call()
        assert e.value.code == L.GSWT_ERR_BAD_ARG
    renderer.synchronize()
    assert (buf.cpu().numpy() == 0x3C).all()
    assert renderer.render(cam, su, W, Hh)[..., 3].max() > 0.0
    return cam, su


# ---- the checks the side images share (depth, pick) ------------------------------------------------------------------------------------------
# `side` is "depth" or "pick": the keyword of render, and in out_<side>_ptr of render_async.
def side_buffer(side, Hh, W):
    """A device buffer for the side image, filled with a value no frame writes everywhere."""
    import torch
    if side == "depth":
        return torch.full((Hh, W), -1.0, dtype=torch.float32, device="cuda")
    return torch.full((Hh, W, 4), -1, dtype=torch.int32, device="cuda")


def check_side_shards_tile(renderer, s, side, full, n, mode):
    """The side images of the n shards, put together by frame_modes' assemblers, are `full` byte for byte.  Returns the n parts for
    the caller's own padding checks."""
    W, Hh, cu, su = s["W"], s["H"], s["cu"], s["su"]
    parts = [renderer.render(cu, su, W, Hh, shard=(r, n, "cols") if mode == "cols" else (r, n), **{side: True}) for r in range(n)]
    if mode == "cols":
        bw = renderer.shard_cols_padded(W, n)
        assert all(p[1].shape == (Hh, bw) for p in parts)
        got = FM.assemble_column_bands(parts, W, bw)
    else:
        assert all(p[1].shape == (renderer.shard_rows_padded(Hh, n), W) for p in parts)
        got = FM.assemble_row_shards(parts, Hh, n)
    assert FM.same(got[1], full), (mode, n)
    return [p[1] for p in parts]


def check_side_overflow_rerun(renderer, s, side):
    """A frame re-run after a pair-buffer overflow rewrites its side image: into a host buffer, then into a device buffer.  Returns
    the (colour, side image) of the frame that did not overflow."""
    import torch
    W, Hh, cu, su = s["W"], s["H"], s["cu"], s["su"]
    img0, p0 = renderer.render(cu, su, W, Hh, **{side: True})
    n_pairs = renderer.timings()["n_pairs"]
    with renderer.options(PAIR_CAP=256):                          # the next frame overflows and is re-run with grown buffers
        img1, p1 = renderer.render(cu, su, W, Hh, **{side: True})
        assert renderer.timings()["n_pairs"] == n_pairs
        assert FM.same(img1, img0) and FM.same(p1, p0)
        renderer.set_option(L.GSWT_OPT_PAIR_CAP, 256)
        out = torch.zeros((Hh, W, 4), dtype=torch.float32, device="cuda")
        buf = side_buffer(side, Hh, W)
        torch.cuda.synchronize()
        renderer.render_wait(renderer.render_async(cu, su, W, Hh, out.data_ptr(), **{f"out_{side}_ptr": buf.data_ptr()}))
        torch.cuda.synchronize()
        assert FM.same(buf.cpu().numpy(), p0)
    return img0, p0


def frames_in_flight(renderer, s, sides, akws):
    """One frame per entry of `akws` (keywords of render_async), all in flight at once, each with a colour buffer and a buffer per
    side image of its own.  Returns per frame the tuple (colour, side images in the order of `sides`) as numpy arrays."""
    import torch
    W, Hh, cu, su = s["W"], s["H"], s["cu"], s["su"]
    bufs = [[torch.zeros((Hh, W, 4), dtype=torch.float32, device="cuda")] + [side_buffer(side, Hh, W) for side in sides] for _ in akws]
    torch.cuda.synchronize()
    tickets = [renderer.render_async(cu, su, W, Hh, b[0].data_ptr(), **{f"out_{side}_ptr": t.data_ptr() for side, t in zip(sides, b[1:])}, **akw)
               for b, akw in zip(bufs, akws)]
    assert len(set(tickets)) == len(akws)
    for t in tickets:
        renderer.render_wait(t)
    torch.cuda.synchronize()
    return [tuple(t.cpu().numpy() for t in b) for b in bufs]


def check_side_graph_sequence(renderer, s, side, want, **akw):
    """GSWT_OPT_GRAPH: replayed graphs pick up the side buffer like any other argument -- two device buffers in turn, a frame without
    the side image in between (another compositor instantiation: the graph is rebuilt), the first buffer again: four graph launches,
    both buffers hold `want`.  Returns the colour the last frame wrote."""
    import torch
    W, Hh, cu, su = s["W"], s["H"], s["cu"], s["su"]
    out = torch.zeros((Hh, W, 4), dtype=torch.float32, device="cuda")
    bufs = [side_buffer(side, Hh, W) for _ in range(2)]
    torch.cuda.synchronize()
    with renderer.options(TIMING=0, GRAPH=1):
        launches0 = renderer.graph_stats()[0]
        for b in (bufs[0], bufs[1], None, bufs[0]):
            if b is not None:
                b.fill_(-1)
                torch.cuda.synchronize()
            renderer.render_wait(renderer.render_async(cu, su, W, Hh, out.data_ptr(), **{f"out_{side}_ptr": b.data_ptr() if b is not None else 0}, **akw))
        torch.cuda.synchronize()
        assert renderer.graph_stats()[0] - launches0 == 4
        for b in bufs:
            assert FM.same(b.cpu().numpy(), want)
    return out.cpu().numpy()


def side_refusal_probe(s, side):
    """What the "argument errors are refused before anything is enqueued" cases call the C ABI with: the frame's blocks (cam, sc, cfg),
    a host side image `host` and a device one `dev` full of sentinels, a zeroed device colour `out`, a `ticket` of -7, and
    untouched(): no ticket was given and none of the three buffers has changed."""
    import torch
    W, Hh = s["W"], s["H"]
    cam, sc, cfg = FM.frame_blocks(s["cu"], s["su"], order_mode=L.GSWT_ORDER_REFERENCE)
    host = np.full((Hh, W), -1.0, np.float32) if side == "depth" else np.full((Hh, W, 4), 0x55555555, np.uint32)
    sentinel = host.copy()
    out = torch.zeros((Hh, W, 4), dtype=torch.float32, device="cuda")
    dev = side_buffer(side, Hh, W)
    torch.cuda.synchronize()
    ticket = C.c_int(-7)

    def untouched():
        assert ticket.value == -7
        torch.cuda.synchronize()
        assert FM.same(host, sentinel) and bool((dev == -1).all()) and not bool(out.any())

    return SimpleNamespace(cam=cam, sc=sc, cfg=cfg, host=host, host_ptr=host.ctypes.data_as(C.c_void_p), out=out, dev=dev,
                           out_ptr=C.c_void_p(out.data_ptr()), dev_ptr=C.c_void_p(dev.data_ptr()), ticket=ticket, untouched=untouched)
