"""Frames rendered straight into the 4:2:0 video formats (GSWT_VIDEO_NV12 / GSWT_VIDEO_I420, include/gswt_hip.h), case by case as
tests/test_out_format_gpu.py does it for the 8-bit formats (the shared checks are tests/frame_outputs.py's): every case renders the same
inputs as RGBA f32 and in a video format and requires the planes to EQUAL tests/yuv_ref.py of the f32 image byte for byte -- every
compositor variant and order with and without the early-out (multi-segment tiles: k_combine's store), screen tiles no splat reaches
over a coloured background, a background with values outside [0, 1] / NaN / inf and a proxy depth buffer, the depth image beside a
video frame, an even size that is not a multiple of the tile (guard bytes behind the last plane untouched), odd sizes refused, row and
column shards with gswt_unshard_format, the peer-copy group gather, asynchronous frames in flight through the graph path with the
format changing from frame to frame, host output, a pair-buffer overflow re-run, and NV12 against I420."""
import numpy as np
import pytest

from gswt_renderer_amd import _lib as L
from oracle import gswt_oracle as orc
from tests import frame_outputs as FO

pytestmark = pytest.mark.gpu

FORMATS = [FO.NV12, FO.I420]
FMT_IDS = [cf.name for cf in FORMATS]
per_format = pytest.mark.parametrize("cf", FORMATS, ids=FMT_IDS)


@pytest.mark.parametrize("order", [L.GSWT_ORDER_REFERENCE, L.GSWT_ORDER_DEPTH], ids=["ref_order", "depth_order"])
@pytest.mark.parametrize("composite", [0, 1, 2])
def test_c3_every_compositor_and_order(renderer, composite, order):
    FO.check_every_compositor_and_order(renderer, FORMATS, composite, order)


@pytest.mark.parametrize("composite", [0, 1, 2])
def test_tiles_without_any_splat_over_a_coloured_background(renderer, composite):
    """The camera looks above the horizon: the upper screen tiles hold no pair at all and are written by the path that stores
    background-only tiles, in the video format like every other tile."""
    from gswt_renderer_amd import host, workloads
    W, Hh, _, su = FO.bind_workload(renderer, FO.workload("c3"))
    cam = workloads.camera_for("c3")
    tgt = (cam["target"][0], cam["target"][1], cam["target"][2] + 0.2)
    cu = host.camera_uniforms(cam["pos"], tgt, cam["up"], cam["fovy"], cam["near"], cam["far"], W, Hh)[0]
    rng = np.random.default_rng(11)
    bg = rng.uniform(0.0, 1.0, size=(Hh, W, 4)).astype(np.float32)
    with renderer.options(COMPOSITE=composite):
        f32 = renderer.render(cu, su, W, Hh, bg_rgba=bg, transmittance_eps=1e-5)
        untouched = np.all(f32 == bg, axis=-1)                      # pixels no splat changed
        tiles = untouched[: Hh // 16 * 16, : W // 16 * 16].reshape(Hh // 16, 16, W // 16, 16).all(axis=(1, 3))
        assert tiles.sum() >= 100 and (~tiles).sum() >= 100, (int(tiles.sum()), tiles.size)   # both kinds of tile are on screen
        for cf in FORMATS:
            assert cf.same(renderer.render(cu, su, W, Hh, bg_rgba=bg, transmittance_eps=1e-5, out_format=cf.fmt), cf.ref(f32)), cf.name


@pytest.mark.parametrize("composite", [0, 1, 2])
def test_background_outside_unit_range_depth_buffer_and_depth_image(renderer, composite):
    def depth_image_beside_the_planes(cf, f32, render):
        """depth=True: the depth image follows the planes and is the f32 call's"""
        f32z, z32 = render(depth=True)
        assert cf.same(render(out_format=cf.fmt), cf.ref(f32z)), cf.name
        got = render(out_format=cf.fmt, depth=True)
        assert cf.same(got[:-1], cf.ref(f32z)) and cf.same(got[:-1], cf.ref(f32)), cf.name
        assert got[-1].dtype == np.float32 and got[-1].shape == z32.shape == f32.shape[:2] and np.array_equal(got[-1], z32), cf.name

    FO.check_hostile_background(renderer, FORMATS, composite, tail=depth_image_beside_the_planes)


@per_format
def test_even_size_off_the_tile_grid_into_a_guarded_device_buffer(renderer, cf):
    FO.check_guarded_device_buffer(renderer, cf, 330, 250)             # even, neither a multiple of 16 (nor of 4)


@pytest.mark.parametrize("size", [(333, 188), (332, 187), (333, 187)], ids=["odd_width", "odd_height", "odd_both"])
@per_format
def test_odd_size_is_refused_and_writes_nothing(renderer, cf, size):
    W, Hh = size
    _, su = FO.check_refused_and_nothing_written(renderer, cf.fmt, W, Hh, 2)
    # the renderer still renders afterwards, the same size as f32 (checked there) and an even size as video
    W2, H2 = W + (W & 1), Hh + (Hh & 1)
    cam2 = orc.default_camera(W2, H2).uniforms()
    assert cf.same(renderer.render(cam2, su, W2, H2, out_format=cf.fmt), cf.ref(renderer.render(cam2, su, W2, H2)))


@pytest.mark.parametrize("n", [3, 8])
@pytest.mark.parametrize("mode", ["rows", "cols"])
@per_format
def test_shards_and_unshard_format(renderer, cf, mode, n):
    FO.check_shards_and_unshard(renderer, cf, mode, n)


@pytest.mark.parametrize("mode", ["cols", "rows"])
def test_group_gather_three_ranks_video(mode):
    FO.check_group_gather_three_ranks(FORMATS, mode)


def test_async_frames_in_flight_through_the_graph_alternating_formats(renderer):
    FO.check_in_flight_alternating_formats(renderer, [L.GSWT_OUT_RGBA32F, L.GSWT_VIDEO_NV12, L.GSWT_OUT_RGBA8_UNORM, L.GSWT_VIDEO_I420], 4)


@per_format
def test_host_output(renderer, cf):
    FO.check_host_output(renderer, cf)


@per_format
def test_pair_buffer_overflow_rerun(renderer, cf):
    FO.check_overflow_rerun(renderer, cf)


def test_nv12_and_i420_hold_the_same_samples(renderer):
    W, Hh, cu, su = FO.bind_workload(renderer, FO.workload("c3"))
    bg, _ = FO.hostile_bg(W, Hh, seed=5)
    y1, cbcr = renderer.render(cu, su, W, Hh, bg_rgba=bg, transmittance_eps=1e-5, out_format=L.GSWT_VIDEO_NV12)
    y2, cb, cr = renderer.render(cu, su, W, Hh, bg_rgba=bg, transmittance_eps=1e-5, out_format=L.GSWT_VIDEO_I420)
    assert np.array_equal(y1, y2) and np.array_equal(cbcr[..., 0], cb) and np.array_equal(cbcr[..., 1], cr)
    assert y1.min() >= 16 and y1.max() <= 235 and cbcr.min() >= 16 and cbcr.max() <= 240
    assert len(np.unique(cb)) > 8 and len(np.unique(cr)) > 8         # a picture, not a constant
