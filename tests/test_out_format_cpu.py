"""The 8-bit output formats at the C ABI (include/gswt_hip.h: GSWT_OUT_*, gswt_render_config.out_format, gswt_unshard_format) and
the test-side quantiser the GPU tests compare against (tests/unorm8_ref.py).  No GPU needed."""
import ctypes as C
import os
import re

import numpy as np

from tests.unorm8_ref import bgra8, q, rgba8

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_output_format_constants_match_the_header():
    from gswt_renderer_amd import _lib as L
    assert (L.GSWT_OUT_RGBA32F, L.GSWT_OUT_RGBA8_UNORM, L.GSWT_OUT_BGRA8_UNORM) == (0, 1, 2)
    src = open(os.path.join(ROOT, "include", "gswt_hip.h")).read()
    declared = dict((k, int(v)) for k, v in re.findall(r"\b(GSWT_OUT_\w+)\s*=\s*(\d+)", src))
    assert declared == {"GSWT_OUT_RGBA32F": 0, "GSWT_OUT_RGBA8_UNORM": 1, "GSWT_OUT_BGRA8_UNORM": 2}


def test_render_config_out_format_field():
    from gswt_renderer_amd import _lib as L
    assert C.sizeof(L.RenderConfig) == 32
    assert L.RenderConfig.out_format.offset == 28 and L.RenderConfig.out_format.size == 4
    # every other offset as before the field had a name
    assert [getattr(L.RenderConfig, f).offset for f in ("culling_dist", "lod_enable_mask", "order_mode", "transmittance_eps",
                                                        "shard_index", "shard_count", "shard_mode")] == [0, 4, 8, 12, 16, 20, 24]
    assert L.RenderConfig().out_format == L.GSWT_OUT_RGBA32F            # a zero-initialised config renders as before


def test_unshard_format_is_exported_and_bound():
    from gswt_renderer_amd import _lib as L
    lib = C.CDLL(os.path.join(ROOT, "gswt_renderer_amd", "lib", "libgswt_hip.so"))
    assert hasattr(lib, "gswt_unshard_format")
    assert "gswt_unshard_format" in L.SYMBOLS
    rs = open(os.path.join(ROOT, "rust", "src", "gswt_hip_sys.rs")).read()
    sig = re.search(r"pub fn gswt_unshard_format\((.*?)\) -> c_int;", rs, flags=re.S)
    assert sig, "gswt_unshard_format missing from rust/src/gswt_hip_sys.rs"
    assert re.findall(r"(\w+): ", sig.group(1)) == ["ctx", "gathered", "width", "height", "shard_count", "shard_mode", "out_format", "out"]
    assert re.search(r"pub const GSWT_OUT_BGRA8_UNORM: c_int = 2;", rs)
    assert re.search(r"pub out_format: u32,", rs)


def test_quantiser_known_answers():
    # 0.5 / 255 and 1.5 / 255 round to binary32 values whose product with 255 is EXACTLY 0.5 / 1.5 in binary32: ties, to even
    # (the exact products, 0.50000003 and 1.50000003, would round up -- the contract is the binary32 product)
    x = np.array([-1.0, 0.0, 0.5 / 255, 1.5 / 255, 127.5 / 255, 1.0, 1.5, np.inf, np.nan], dtype=np.float32)
    assert q(x).tolist() == [0, 0, 0, 2, 128, 255, 255, 255, 0]
    assert q(np.array([-np.inf, -0.0, 1.0 / 255, 254.5 / 255, np.nextafter(np.float32(1), np.float32(0))], dtype=np.float32)).tolist() == \
        [0, 0, 1, 254, 255]


def test_quantiser_channel_orders():
    img = np.array([[[0.0, 0.5, 1.0, 0.25]]], dtype=np.float32)
    assert rgba8(img).tolist() == [[[0, 128, 255, 64]]]
    assert bgra8(img).tolist() == [[[255, 128, 0, 64]]]
    assert rgba8(img).dtype == np.uint8 and bgra8(img).dtype == np.uint8
