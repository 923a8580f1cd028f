"""The 4:2:0 video output formats at the C ABI (include/gswt_hip.h: GSWT_VIDEO_NV12 / GSWT_VIDEO_I420, gswt_out_image_bytes) and the
test-side definition the GPU tests compare against (tests/yuv_ref.py): the constants in the header, the Python table and the generated
Rust file; the size call for all five formats, odd sizes and unknown formats; the BT.709 colour bars as known answers; the float32
definition against an independent float64 evaluation within one code.  No GPU needed."""
import ctypes as C
import os
import re

import numpy as np

from tests import yuv_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_video_format_constants_in_header_python_and_rust():
    from gswt_renderer_amd import _lib as L
    assert (L.GSWT_VIDEO_NV12, L.GSWT_VIDEO_I420) == (16, 17)
    src = open(os.path.join(ROOT, "include", "gswt_hip.h")).read()
    declared = dict((k, int(v)) for k, v in re.findall(r"\b(GSWT_VIDEO_\w+)\s*=\s*(\d+)", src))
    assert declared == {"GSWT_VIDEO_NV12": 16, "GSWT_VIDEO_I420": 17}
    rs = open(os.path.join(ROOT, "rust", "src", "gswt_hip_sys.rs")).read()
    assert re.search(r"pub const GSWT_VIDEO_NV12: c_int = 16;", rs)
    assert re.search(r"pub const GSWT_VIDEO_I420: c_int = 17;", rs)


def test_out_image_bytes_is_exported_and_bound():
    from gswt_renderer_amd import _lib as L
    lib = C.CDLL(os.path.join(ROOT, "gswt_renderer_amd", "lib", "libgswt_hip.so"))
    assert hasattr(lib, "gswt_out_image_bytes")
    assert L.SYMBOLS["gswt_out_image_bytes"] == (C.c_size_t, [C.c_int, C.c_int, C.c_int])
    rs = open(os.path.join(ROOT, "rust", "src", "gswt_hip_sys.rs")).read()
    sig = re.search(r"pub fn gswt_out_image_bytes\((.*?)\) -> usize;", rs, flags=re.S)
    assert sig, "gswt_out_image_bytes missing from rust/src/gswt_hip_sys.rs"
    assert re.findall(r"(\w+): ", sig.group(1)) == ["out_format", "rows", "out_w"]


def test_out_image_bytes_values():
    from gswt_renderer_amd import _lib as L
    size = L.load().gswt_out_image_bytes
    for rows, w in ((1080, 1920), (2160, 3840), (250, 330), (16, 16), (2, 2)):
        assert size(L.GSWT_OUT_RGBA32F, rows, w) == rows * w * 16
        assert size(L.GSWT_OUT_RGBA8_UNORM, rows, w) == rows * w * 4
        assert size(L.GSWT_OUT_BGRA8_UNORM, rows, w) == rows * w * 4
        assert size(L.GSWT_VIDEO_NV12, rows, w) == rows * w * 3 // 2
        assert size(L.GSWT_VIDEO_I420, rows, w) == rows * w + 2 * (rows // 2) * (w // 2)
    assert size(L.GSWT_VIDEO_NV12, 1080, 1920) == 3110400               # 3.1 MB at 1080p
    # odd sizes: fine for the pixel formats, no plane layout for the video ones
    for rows, w in ((187, 333), (187, 332), (188, 333)):
        assert size(L.GSWT_OUT_RGBA32F, rows, w) == rows * w * 16 and size(L.GSWT_OUT_RGBA8_UNORM, rows, w) == rows * w * 4
        assert size(L.GSWT_VIDEO_NV12, rows, w) == 0 and size(L.GSWT_VIDEO_I420, rows, w) == 0
    for bad in (3, 7, 15, 18, -1, 0x7FFFFFFF):
        assert size(bad, 64, 64) == 0, bad
    for fmt in (L.GSWT_OUT_RGBA32F, L.GSWT_OUT_RGBA8_UNORM, L.GSWT_VIDEO_NV12, L.GSWT_VIDEO_I420):
        assert size(fmt, 0, 64) == 0 and size(fmt, -2, 64) == 0 and size(fmt, 64, -2) == 0
    # no 32-bit overflow: 65535 tiles of 16 px in both directions is the largest target gswt_render accepts
    assert size(L.GSWT_OUT_RGBA32F, 1048560, 1048560) == 1048560 * 1048560 * 16
    assert size(L.GSWT_VIDEO_I420, 1048560, 1048560) == 1048560 * 1048560 * 3 // 2


BARS = {    # BT.709 limited-range codes of the 100 % colour bars
    "white": ((1, 1, 1), (235, 128, 128)), "black": ((0, 0, 0), (16, 128, 128)), "red": ((1, 0, 0), (63, 102, 240)),
    "green": ((0, 1, 0), (173, 42, 26)), "blue": ((0, 0, 1), (32, 240, 118)), "yellow": ((1, 1, 0), (219, 16, 138)),
    "cyan": ((0, 1, 1), (188, 154, 16)), "magenta": ((1, 0, 1), (78, 214, 230)),
}


def test_colour_bars_known_answers():
    for name, (rgb, (y, cb, cr)) in BARS.items():
        img = np.empty((2, 2, 4), np.float32)
        img[..., :3] = rgb
        img[..., 3] = 0.25                                           # alpha is dropped
        py, pcb, pcr = yuv_ref.i420(img)
        assert py.tolist() == [[y, y], [y, y]] and pcb.tolist() == [[cb]] and pcr.tolist() == [[cr]], name
        ny, ncbcr = yuv_ref.nv12(img)
        assert ny.tolist() == py.tolist() and ncbcr.tolist() == [[[cb, cr]]], name
    # out of range and non-finite values clamp like the 8-bit formats' q(): NaN -> 0
    odd = np.array([[[np.nan, -3.0, -np.inf, 0], [np.inf, 7.0, 1.5, 0]], [[np.nan, np.nan, np.nan, np.nan], [2.0, np.inf, 1.0, 9]]], np.float32)
    py, pcb, pcr = yuv_ref.i420(odd)
    assert py.tolist() == [[16, 235], [16, 235]] and pcb.tolist() == [[128]] and pcr.tolist() == [[128]]


def test_layouts_and_block_mean():
    rng = np.random.default_rng(5)
    img = rng.uniform(0.0, 1.0, size=(6, 8, 4)).astype(np.float32)
    y, cb, cr = yuv_ref.i420(img)
    ny, cbcr = yuv_ref.nv12(img)
    assert y.shape == (6, 8) and cb.shape == cr.shape == (3, 4) and cbcr.shape == (3, 4, 2)
    assert all(a.dtype == np.uint8 for a in (y, cb, cr, ny, cbcr))
    assert np.array_equal(ny, y) and np.array_equal(cbcr[..., 0], cb) and np.array_equal(cbcr[..., 1], cr)
    assert yuv_ref.nv12_bytes(img).size == yuv_ref.i420_bytes(img).size == 6 * 8 * 3 // 2
    assert np.array_equal(yuv_ref.nv12_bytes(img)[48:].reshape(-1, 2).T.reshape(-1), yuv_ref.i420_bytes(img)[48:])
    # a block whose left column is red and right column blue: chroma is the plain mean of the four samples (centre sited)
    blk = np.zeros((2, 2, 4), np.float32)
    blk[:, 0, 0] = 1.0
    blk[:, 1, 2] = 1.0
    _, b_cb, b_cr = yuv_ref.i420(blk)
    assert b_cb.tolist() == [[171]] and b_cr.tolist() == [[179]]     # (102 + 240) / 2, (240 + 118) / 2


def test_float32_definition_within_one_code_of_float64():
    rng = np.random.default_rng(20260)
    img = rng.uniform(-0.2, 1.2, size=(512, 1024, 4)).astype(np.float32)
    flat = img.reshape(-1)
    idx = rng.choice(flat.size, size=3000, replace=False)
    flat[idx[:1000]] = np.nan
    flat[idx[1000:2000]] = np.inf
    flat[idx[2000:]] = -np.inf
    y, cb, cr = yuv_ref.i420(img)
    y64, cb64, cr64 = yuv_ref.yuv_f64(img)
    n_diff = 0
    for got, want, lo, hi in ((y, y64, 16, 235), (cb, cb64, 16, 240), (cr, cr64, 16, 240)):
        assert got.min() >= lo and got.max() <= hi
        nearest = np.rint(want)
        d = np.abs(got.astype(np.float64) - nearest)
        assert d.max() <= 1.0, d.max()
        assert np.abs(got.astype(np.float64) - want).max() <= 0.5 + 1e-3          # a different code only at a rounding tie
        n_diff += int(np.count_nonzero(d))
    print(f"codes that differ from the float64 evaluation's: {n_diff} of {y.size + cb.size + cr.size}")
    assert n_diff <= (y.size + cb.size + cr.size) // 1000
