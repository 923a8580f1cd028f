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
from tests import frame_outputs as FO
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
    return FO.workload("c3")


def test_colour_untouched_by_depth_output(renderer, c3):
    W, Hh, cu, su = FO.bind_workload(renderer, c3)
    bgd = FO.bg_depth(W, Hh)
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
                assert FM.bits_equal(z, z32[i])


@pytest.mark.parametrize("eps,bg", [(0.0, False), (1e-5, True)], ids=["plain", "early_bg_depth"])
def test_variants_agree_bit_for_bit(renderer, c3, eps, bg):
    import torch
    W, Hh, cu, su = FO.bind_workload(renderer, c3)
    kw = dict(transmittance_eps=eps, bg_depth=FO.bg_depth(W, Hh) if bg else None)
    _, z0 = renderer.render(cu, su, W, Hh, depth=True, **kw)
    bgd_dev = torch.from_numpy(kw["bg_depth"]).cuda() if bg else None
    FO.check_side_graph_sequence(renderer, c3, "depth", z0, transmittance_eps=eps, bg_depth_ptr=bgd_dev.data_ptr() if bg else 0)


def test_multi_segment_tiles_fold_depth(renderer, c3):
    W, Hh, cu, su = FO.bind_workload(renderer, c3)
    bgd = FO.bg_depth(W, Hh)
    for kw in (dict(), dict(bg_depth=bgd, order_mode=L.GSWT_ORDER_DEPTH)):
        img0, z0 = renderer.render(cu, su, W, Hh, depth=True, **kw)
        with renderer.options(SEGMENT=256):
            img1, z1 = renderer.render(cu, su, W, Hh, depth=True, **kw)
        assert renderer.timings()["n_pairs"] > 256 * renderer.timings()["n_tiles"] / 4      # many tiles have several segments
        assert np.abs(z1.astype(np.float64) - z0).max() <= 1e-6
        assert np.abs(img1.astype(np.float64) - img0).max() <= 1e-5


def test_shards_tile_the_depth_image(renderer, c3):
    W, Hh, cu, su = FO.bind_workload(renderer, c3)
    _, full = renderer.render(cu, su, W, Hh, depth=True)
    for n in (2, 3, 8):
        bw = renderer.shard_cols_padded(W, n)
        for r, part in enumerate(FO.check_side_shards_tile(renderer, c3, "depth", full, n, "cols")):
            assert not part[:, max(0, min(W, (r + 1) * bw) - r * bw):].any()      # padding columns are zero
    for n in (2, 3):
        for r, part in enumerate(FO.check_side_shards_tile(renderer, c3, "depth", full, n, "rows")):
            assert not part[16 * len(range(r, (Hh + 15) // 16, n)):].any()        # padding rows are zero


def test_overflow_rerun_rewrites_depth(renderer, c3):
    FO.bind_workload(renderer, c3)
    FO.check_side_overflow_rerun(renderer, c3, "depth")


def test_async_frames_in_flight_write_their_own_depth(renderer, c3):
    import torch
    W, Hh, cu, su = FO.bind_workload(renderer, c3)
    slots = renderer.frame_slots()
    # every frame its own proxy depth buffer, so every frame's depth image differs
    bgds = [np.full((Hh, W), 1.0 - 0.001 * k, np.float32) for k in range(slots)]
    wants = [renderer.render(cu, su, W, Hh, bg_depth=b, depth=True)[1] for b in bgds]
    bg_dev = [torch.from_numpy(b).cuda() for b in bgds]
    got = FO.frames_in_flight(renderer, c3, ("depth",), [dict(bg_depth_ptr=b.data_ptr()) for b in bg_dev])
    for k in range(slots):
        assert FM.bits_equal(got[k][1], wants[k]), k
    assert not np.array_equal(wants[0], wants[-1])


def test_argument_errors_refused_before_enqueue(renderer, c3):
    W, Hh, cu, su = FO.bind_workload(renderer, c3)
    lib, h = renderer._lib, renderer._h
    p = FO.side_refusal_probe(c3, "depth")
    cam, sc, cfg, zp, zd, od, ticket = p.cam, p.sc, p.cfg, p.host_ptr, p.dev_ptr, p.out_ptr, C.byref(p.ticket)
    # host path: out_depth without out_rgba; out_depth aliasing out_rgba
    assert lib.gswt_render_depth(h, cam, sc, C.byref(cfg), W, Hh, None, None, 0, None, zp, 0) == L.GSWT_ERR_BAD_ARG
    assert lib.gswt_render_depth(h, cam, sc, C.byref(cfg), W, Hh, None, None, 0, zp, zp, 0) == L.GSWT_ERR_BAD_ARG
    p.untouched()
    # device path: the same, plus a bad out_format -- nothing is written to the depth buffer
    assert lib.gswt_render_async_depth(h, cam, sc, C.byref(cfg), W, Hh, None, None, None, zd, ticket) == L.GSWT_ERR_BAD_ARG
    assert lib.gswt_render_async_depth(h, cam, sc, C.byref(cfg), W, Hh, None, None, zd, zd, ticket) == L.GSWT_ERR_BAD_ARG
    cfg.out_format = 7
    assert lib.gswt_render_async_depth(h, cam, sc, C.byref(cfg), W, Hh, None, None, od, zd, ticket) == L.GSWT_ERR_BAD_ARG
    p.untouched()
    # and the ctx still renders
    _, z_ok = renderer.render(cu, su, W, Hh, depth=True)
    assert (z_ok < 1.0).any()
