"""Test-side statement of the 8-bit output contract (include/gswt_hip.h, GSWT_OUT_*): each channel byte is
q(x) = round_half_even(min(max(x, 0), 1) * 255) of the float the same frame writes as RGBA f32, with one correctly rounded
binary32 product; NaN -> 0.  Shared by tests/test_out_format_cpu.py and tests/test_out_format_gpu.py."""
import numpy as np


def q(x):
    """RGBA f32 values -> uint8, as the compositor's 8-bit store computes them."""
    x = np.asarray(x, dtype=np.float32)
    return np.rint(np.fmin(np.fmax(x, np.float32(0)), np.float32(1)).astype(np.float32) * np.float32(255)).astype(np.uint8)


def rgba8(img_f32):
    """The GSWT_OUT_RGBA8_UNORM image of an RGBA f32 frame: bytes R, G, B, A."""
    return q(img_f32)


def bgra8(img_f32):
    """The GSWT_OUT_BGRA8_UNORM image of an RGBA f32 frame: bytes B, G, R, A."""
    return np.ascontiguousarray(q(img_f32)[..., [2, 1, 0, 3]])
