"""Frames rendered straight into the 8-bit display formats (GSWT_OUT_RGBA8_UNORM / GSWT_OUT_BGRA8_UNORM, include/gswt_hip.h).
Every case renders the same inputs twice, once as RGBA f32 and once in 8 bits, and requires the 8-bit image to be q(f32 image)
EXACTLY (tests/unorm8_ref.py), BGRA as the channel swap of that: every compositor variant and order, the early-out, a background
colour with values outside [0, 1] and a depth buffer, a frame size that is not a multiple of the 16-px tile (guard bytes behind
the image stay untouched), row and column shards with gswt_unshard_format, the peer-copy group gather, asynchronous frames in
flight through the graph path with the format changing from frame to frame, host output, a pair-buffer overflow re-run, and
the refusal of unknown formats.  The checks themselves are tests/frame_outputs.py's, shared with tests/test_video_out_gpu.py."""
import ctypes as C

import pytest

from gswt_renderer_amd import _lib as L
from tests import frame_outputs as FO

pytestmark = pytest.mark.gpu

FORMATS = [FO.RGBA8, FO.BGRA8]
per_format = pytest.mark.parametrize("cf", FORMATS, ids=[cf.name for cf in FORMATS])


@pytest.mark.parametrize("order", [L.GSWT_ORDER_REFERENCE, L.GSWT_ORDER_DEPTH], ids=["ref_order", "depth_order"])
@pytest.mark.parametrize("composite", [0, 1, 2])
def test_c3_every_compositor_and_order(renderer, composite, order):
    FO.check_every_compositor_and_order(renderer, FORMATS, composite, order)


@pytest.mark.parametrize("composite", [0, 1, 2])
def test_background_outside_unit_range_and_depth_buffer(renderer, composite):
    FO.check_hostile_background(renderer, FORMATS, composite)


@per_format
def test_odd_frame_size_into_a_guarded_device_buffer(renderer, cf):
    FO.check_guarded_device_buffer(renderer, cf, 333, 187)


@pytest.mark.parametrize("mode", ["rows", "cols"])
@per_format
def test_shards_and_unshard_format(renderer, cf, mode):
    for n in (3, 8):
        FO.check_shards_and_unshard(renderer, cf, mode, n)


@pytest.mark.parametrize("mode", ["cols", "rows"])
def test_group_gather_three_ranks_8bit(mode):
    def mixed_formats_are_refused(rs, submit, wait):
        tickets, frames = submit([L.GSWT_OUT_RGBA32F, L.GSWT_OUT_RGBA8_UNORM, L.GSWT_OUT_RGBA32F])
        n = len(rs)
        arr = (C.c_void_p * n)(*[r._h for r in rs])
        rc = L.load().gswt_group_render_gather(arr, (C.c_int * n)(*tickets), (C.c_void_p * n)(*[f.data_ptr() for f in frames]), n)
        assert rc == L.GSWT_ERR_BAD_ARG
        assert "out_format" in rs[1]._lib.gswt_last_error(rs[1]._h).decode()
        wait(tickets)

    FO.check_group_gather_three_ranks(FORMATS, mode, tail=mixed_formats_are_refused)


def test_async_frames_in_flight_through_the_graph_alternating_formats(renderer):
    FO.check_in_flight_alternating_formats(renderer, [L.GSWT_OUT_RGBA32F, L.GSWT_OUT_RGBA8_UNORM, L.GSWT_OUT_RGBA32F, L.GSWT_OUT_BGRA8_UNORM], 3)


@per_format
def test_host_output(renderer, cf):
    FO.check_host_output(renderer, cf)


@per_format
def test_pair_buffer_overflow_rerun(renderer, cf):
    FO.check_overflow_rerun(renderer, cf)


@pytest.mark.parametrize("bad", [3, 0xFFFFFFFF])
def test_unknown_format_is_refused_and_writes_nothing(renderer, bad):
    FO.check_refused_and_nothing_written(renderer, bad, 64, 48, 1)
