"""Depth output (gswt_render_depth / gswt_render_async_depth, include/gswt_hip.h) on the GPU.

Against the CPU reference tests/depth_ref.py on the golden-size cases (plane, HeightMap, Sphere surfaces) and one mid-size frame, in
both order modes, with and without a proxy depth buffer; then full c3 frames against themselves: the colour is bit-identical with and
without depth output in every out_format, the compositor / graph / item-order variants agree bit for bit, multi-segment tiles fold
through k_combine, shards tile the frame, a frame re-run after a pair overflow rewrites its depth, frames in flight write their own
depth buffers, and argument errors are refused before anything is enqueued."""
import ctypes as C

import numpy as np
import pytest

from gswt_renderer_amd import _lib as L
from oracle import gswt_oracle as orc
from tests import depth_ref as DR
from tests import frame_modes as FM
from tests import helpers as H

pytestmark = pytest.mark.gpu
FORMATS = [L.GSWT_OUT_RGBA32F, L.GSWT_OUT_RGBA8_UNORM, L.GSWT_OUT_BGRA8_UNORM]


@pytest.mark.parametrize("bg", [False, True], ids=["clear", "bg_depth"])
@pytest.mark.parametrize("order_mode", [0, 1], ids=["reference", "depth"])
@pytest.mark.parametrize("name", ["case_plane", "case_hmap", "case_sphere"])
def test_depth_matches_reference_golden_cases(renderer, name, order_mode, bg):
    from gswt_renderer_amd import host
    from gswt_renderer_amd.pipeline import GSWTPipeline
    g = DR.golden_case(name)
    W, Hh = g["W"], g["H"]
    bgc, bgd = DR.bg_images(W, Hh) if bg else (None, None)
    ref_img, ref_z, n_cover = DR.composite(g["sp"], W, Hh, splat_scale=g["su"].splat_scale, order_mode=order_mode, bg_rgba=bgc,
                                           bg_depth=bgd, with_cover=True)
    cu, vp = host.camera_uniforms(g["pos"], g["tgt"], (0, 0, 1), 45.0, 0.1, 2400.0, W, Hh)
    pipe = GSWTPipeline(g["verts"], host.user_data(**g["cfg"]), renderer=renderer)
    pipe.update(g["pos"], vp)
    img, z = pipe.render(cu, W, Hh, bg_rgba=bgc, bg_depth=bgd, order_mode=order_mode, depth=True)
    assert z.shape == (Hh, W) and z.dtype == np.float32
    FM.check_against_ref(img, z, ref_img, ref_z)
    # colour and depth from the same frame: the colour is the image a frame without depth output writes
    assert np.array_equal(img, pipe.render(cu, W, Hh, bg_rgba=bgc, bg_depth=bgd, order_mode=order_mode))
    zbg = np.ones((Hh, W), np.float32) if bgd is None else bgd
    free = n_cover == 0
    assert free.any() and (~free).any()
    assert np.abs(z[free] - zbg[free]).max() <= FM.ZTOL


@pytest.mark.parametrize("order_mode,bg", [(0, False), (1, True)], ids=["reference-clear", "depth-bg_depth"])
def test_depth_matches_reference_mid_size(renderer, order_mode, bg):
    pp = H.tileset()
    W, Hh = 320, 240
    cam = orc.default_camera(W, Hh).uniforms()
    su = orc.scene_uniforms(num_lod=pp.n_lod, map_half_wh=(1, 2))
    case = H.grid_case(pp)
    case.upload(renderer)
    sp = orc.project_draws(cam, su, pp.tex, case.orc_draws)
    bgc, bgd = DR.bg_images(W, Hh, seed=11) if bg else (None, None)
    ref_img, ref_z = DR.composite(sp, W, Hh, splat_scale=su.splat_scale, order_mode=order_mode, bg_rgba=bgc, bg_depth=bgd)
    img, z = renderer.render(cam, su, W, Hh, order_mode=order_mode, bg_rgba=bgc, bg_depth=bgd, depth=True)
    assert ref_img[..., 3].max() > 0.5
    FM.check_against_ref(img, z, ref_img, ref_z)


# ---- full frames against themselves (c3) ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def c3():
    import bench
    w, wang, cu, vp, sort = bench.build_workload("c3")
    return dict(W=w["width"], H=w["height"], wang=wang, cu=cu, vp=vp, sort=sort, su=wang.scene_uniforms())


def _bind(renderer, s):
    s["wang"].upload_to(renderer)
    renderer.configure(None)
    renderer.set_draws(s["sort"].draws, s["sort"].merged_gs_index, s["sort"].merged_map_id, s["sort"].merged_lod_id)


def _bg_depth(W, Hh):
    return np.random.default_rng(3).uniform(0.99, 1.0, size=(Hh, W)).astype(np.float32)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def test_colour_untouched_by_depth_output(renderer, c3):
    _bind(renderer, c3)
    W, Hh, cu, su = c3["W"], c3["H"], c3["cu"], c3["su"]
    bgd = _bg_depth(W, Hh)
    z32 = {}
    for fmt in FORMATS:
        for i, kw in enumerate((dict(), dict(transmittance_eps=1e-5, bg_depth=bgd))):
            want = renderer.render(cu, su, W, Hh, out_format=fmt, **kw)
            img, z = renderer.render(cu, su, W, Hh, out_format=fmt, depth=True, **kw)
            assert np.array_equal(img, want), (fmt, kw.keys())
            assert z.dtype == np.float32 and z.shape == (Hh, W)
            assert (z < 1.0).mean() > 0.1           # the frame covers a good part of the screen
            # the depth image does not depend on the colour format
            if fmt == L.GSWT_OUT_RGBA32F:
                z32[i] = z
            else:
                assert np.array_equal(_bits(z), _bits(z32[i]))


@pytest.mark.parametrize("eps,bg", [(0.0, False), (1e-5, True)], ids=["plain", "early_bg_depth"])
def test_variants_agree_bit_for_bit(renderer, c3, eps, bg):
    _bind(renderer, c3)
    W, Hh, cu, su = c3["W"], c3["H"], c3["cu"], c3["su"]
    kw = dict(transmittance_eps=eps, bg_depth=_bg_depth(W, Hh) if bg else None)
    _, z0 = renderer.render(cu, su, W, Hh, depth=True, **kw)
    for opt in (L.GSWT_OPT_COMPOSITE, L.GSWT_OPT_ITEM_ORDER):
        renderer.set_option(opt, 1)
        try:
            _, z1 = renderer.render(cu, su, W, Hh, depth=True, **kw)
        finally:
            renderer.set_option(opt, 0)
        assert np.array_equal(_bits(z1), _bits(z0)), opt
    # GSWT_OPT_GRAPH: replayed graphs pick up the depth buffer like any other argument (two device buffers in turn, and a frame without
    # depth in between: another compositor instantiation, the graph is rebuilt)
    import torch
    renderer.set_option(L.GSWT_OPT_TIMING, 0)
    renderer.set_option(L.GSWT_OPT_GRAPH, 1)
    try:
        out = torch.zeros((Hh, W, 4), dtype=torch.float32, device="cuda")
        zs = [torch.full((Hh, W), -1.0, dtype=torch.float32, device="cuda") for _ in range(2)]
        bgd_dev = torch.from_numpy(kw["bg_depth"]).cuda() if bg else None
        torch.cuda.synchronize()
        launches0 = renderer.graph_stats()[0]
        for zt in (zs[0], zs[1], None, zs[0]):
            if zt is not None:
                zt.fill_(-1.0)
                torch.cuda.synchronize()
            t = renderer.render_async(cu, su, W, Hh, out.data_ptr(), transmittance_eps=eps, bg_depth_ptr=bgd_dev.data_ptr() if bg else 0,
                                      out_depth_ptr=zt.data_ptr() if zt is not None else 0)
            renderer.render_wait(t)
        torch.cuda.synchronize()
        assert renderer.graph_stats()[0] - launches0 == 4
        for zt in zs:
            assert np.array_equal(_bits(zt.cpu().numpy()), _bits(z0))
    finally:
        renderer.set_option(L.GSWT_OPT_GRAPH, 0)
        renderer.set_option(L.GSWT_OPT_TIMING, 2)


def test_multi_segment_tiles_fold_depth(renderer, c3):
    _bind(renderer, c3)
    W, Hh, cu, su = c3["W"], c3["H"], c3["cu"], c3["su"]
    bgd = _bg_depth(W, Hh)
    for kw in (dict(), dict(bg_depth=bgd, order_mode=L.GSWT_ORDER_DEPTH)):
        img0, z0 = renderer.render(cu, su, W, Hh, depth=True, **kw)
        renderer.set_option(L.GSWT_OPT_SEGMENT, 256)
        try:
            img1, z1 = renderer.render(cu, su, W, Hh, depth=True, **kw)
        finally:
            renderer.set_option(L.GSWT_OPT_SEGMENT, L.GSWT_DEFAULT_SEGMENT)
        assert renderer.timings()["n_pairs"] > 256 * renderer.timings()["n_tiles"] / 4      # many tiles have several segments
        assert np.abs(z1.astype(np.float64) - z0).max() <= 1e-6
        assert np.abs(img1.astype(np.float64) - img0).max() <= 1e-5


def test_shards_tile_the_depth_image(renderer, c3):
    _bind(renderer, c3)
    W, Hh, cu, su = c3["W"], c3["H"], c3["cu"], c3["su"]
    _, full = renderer.render(cu, su, W, Hh, depth=True)
    for n in (2, 3, 8):
        bw = renderer.shard_cols_padded(W, n)
        z = np.full((Hh, W), np.nan, np.float32)
        for r in range(n):
            _, part = renderer.render(cu, su, W, Hh, shard=(r, n, "cols"), depth=True)
            assert part.shape == (Hh, bw)
            x0, x1 = r * bw, min(W, (r + 1) * bw)
            if x1 > x0:
                z[:, x0:x1] = part[:, :x1 - x0]
            assert not part[:, max(0, x1 - x0):].any()            # padding columns are zero
        assert np.array_equal(_bits(z), _bits(full)), n
    for n in (2, 3):
        rows = renderer.shard_rows_padded(Hh, n)
        z = np.full((Hh, W), np.nan, np.float32)
        for r in range(n):
            _, part = renderer.render(cu, su, W, Hh, shard=(r, n), depth=True)
            assert part.shape == (rows, W)
            k = 0
            for ty in range(r, (Hh + 15) // 16, n):
                y0, y1 = ty * 16, min(Hh, ty * 16 + 16)
                z[y0:y1] = part[k * 16:k * 16 + (y1 - y0)]
                k += 1
            assert not part[k * 16:].any()                        # padding rows are zero
        assert np.array_equal(_bits(z), _bits(full)), n


def test_overflow_rerun_rewrites_depth(renderer, c3):
    import torch
    _bind(renderer, c3)
    W, Hh, cu, su = c3["W"], c3["H"], c3["cu"], c3["su"]
    img0, z0 = renderer.render(cu, su, W, Hh, depth=True)
    n_pairs = renderer.timings()["n_pairs"]
    try:
        renderer.set_option(L.GSWT_OPT_PAIR_CAP, 256)             # the next frame overflows and is re-run with grown buffers
        img1, z1 = renderer.render(cu, su, W, Hh, depth=True)
        assert renderer.timings()["n_pairs"] == n_pairs
        assert np.array_equal(img1, img0) and np.array_equal(_bits(z1), _bits(z0))
        renderer.set_option(L.GSWT_OPT_PAIR_CAP, 256)
        out = torch.zeros((Hh, W, 4), dtype=torch.float32, device="cuda")
        zt = torch.full((Hh, W), -1.0, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        renderer.render_wait(renderer.render_async(cu, su, W, Hh, out.data_ptr(), out_depth_ptr=zt.data_ptr()))
        torch.cuda.synchronize()
        assert np.array_equal(_bits(zt.cpu().numpy()), _bits(z0))
    finally:
        renderer.set_option(L.GSWT_OPT_PAIR_CAP, 0)


def test_async_frames_in_flight_write_their_own_depth(renderer, c3):
    import torch
    _bind(renderer, c3)
    W, Hh, cu, su = c3["W"], c3["H"], c3["cu"], c3["su"]
    slots = renderer.frame_slots()
    # every frame its own proxy depth buffer, so every frame's depth image differs
    bgds = [np.full((Hh, W), 1.0 - 0.001 * k, np.float32) for k in range(slots)]
    wants = [renderer.render(cu, su, W, Hh, bg_depth=b, depth=True)[1] for b in bgds]
    bg_dev = [torch.from_numpy(b).cuda() for b in bgds]
    outs = [torch.zeros((Hh, W, 4), dtype=torch.float32, device="cuda") for _ in range(slots)]
    zs = [torch.full((Hh, W), -1.0, dtype=torch.float32, device="cuda") for _ in range(slots)]
    torch.cuda.synchronize()
    tickets = [renderer.render_async(cu, su, W, Hh, o.data_ptr(), bg_depth_ptr=b.data_ptr(), out_depth_ptr=z.data_ptr())
               for o, b, z in zip(outs, bg_dev, zs)]
    assert len(set(tickets)) == slots
    for t in tickets:
        renderer.render_wait(t)
    torch.cuda.synchronize()
    for k in range(slots):
        assert np.array_equal(_bits(zs[k].cpu().numpy()), _bits(wants[k])), k
    assert not np.array_equal(wants[0], wants[-1])


def test_argument_errors_refused_before_enqueue(renderer, c3):
    import torch
    _bind(renderer, c3)
    W, Hh, cu, su = c3["W"], c3["H"], c3["cu"], c3["su"]
    lib, h = renderer._lib, renderer._h
    cam = (C.c_char * 176).from_buffer_copy(bytes(cu))
    sc = (C.c_char * 160).from_buffer_copy(bytes(su))
    cfg = L.RenderConfig()
    cfg.culling_dist, cfg.lod_enable_mask = 1.0, 0xFFFFFFFF
    z = np.full((Hh, W), -1.0, np.float32)
    zp = z.ctypes.data_as(C.c_void_p)
    # host path: out_depth without out_rgba; out_depth aliasing out_rgba
    assert lib.gswt_render_depth(h, cam, sc, C.byref(cfg), W, Hh, None, None, 0, None, zp, 0) == L.GSWT_ERR_BAD_ARG
    assert lib.gswt_render_depth(h, cam, sc, C.byref(cfg), W, Hh, None, None, 0, zp, zp, 0) == L.GSWT_ERR_BAD_ARG
    assert (z == -1.0).all()
    # device path: the same, plus a bad out_format -- nothing is written to the depth buffer
    out = torch.zeros((Hh, W, 4), dtype=torch.float32, device="cuda")
    zt = torch.full((Hh, W), -1.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    ticket = C.c_int(-7)
    zd, od = C.c_void_p(zt.data_ptr()), C.c_void_p(out.data_ptr())
    assert lib.gswt_render_async_depth(h, cam, sc, C.byref(cfg), W, Hh, None, None, None, zd, C.byref(ticket)) == L.GSWT_ERR_BAD_ARG
    assert lib.gswt_render_async_depth(h, cam, sc, C.byref(cfg), W, Hh, None, None, zd, zd, C.byref(ticket)) == L.GSWT_ERR_BAD_ARG
    cfg.out_format = 7
    assert lib.gswt_render_async_depth(h, cam, sc, C.byref(cfg), W, Hh, None, None, od, zd, C.byref(ticket)) == L.GSWT_ERR_BAD_ARG
    assert ticket.value == -7
    torch.cuda.synchronize()
    assert bool((zt == -1.0).all()) and not bool(out.any())
    # and the ctx still renders
    _, z_ok = renderer.render(cu, su, W, Hh, depth=True)
    assert (z_ok < 1.0).any()
