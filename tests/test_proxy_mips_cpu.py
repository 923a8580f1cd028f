"""The proxy mip restatement (tests/proxy_mips_ref.py) against Pillow's Lanczos resize and known answers, the default texture
size, and the mip build's entry points in the C ABI and the Python wrapper (no GPU needed)."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import proxy_mips_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# (w, h, n): down- and up-sampling, 1 -> n, n -> 1 and ratio 1 on one axis
PIL_CASES = [(100, 80, 64), (257, 129, 128), (300, 300, 1), (64, 100, 64), (33, 500, 16), (8, 8, 4), (1, 37, 1), (37, 1, 32),
             (1, 1, 8), (20, 300, 16), (300, 20, 256), (64, 13, 64)]


@pytest.mark.parametrize("w,h,n", PIL_CASES)
def test_restatement_matches_pillow_lanczos(w, h, n):
    """Pillow's float-mode ("F") LANCZOS resize is an independent implementation of the same separable Lanczos3 with clipped,
    renormalised windows; it stores f32, so the two agree to f32 rounding of values up to 255 (~3e-5 seen)."""
    Image = pytest.importorskip("PIL.Image")
    img = np.random.default_rng(w * 1000 + h + n).integers(0, 256, (h, w, 4)).astype(np.uint8)
    if (n, n) == (w, h):
        pytest.skip("copy case")
    _, _, t = R.resize_level(img, n)
    lanczos = getattr(Image, "Resampling", Image).LANCZOS
    for k in range(4):
        p = np.asarray(Image.fromarray(img[..., k].astype(np.float32), mode="F").resize((n, n), lanczos), np.float64)
        np.testing.assert_allclose(t[..., k], p, rtol=0, atol=2e-4)


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
def test_constant_image_stays_constant_at_every_level(dtype):
    v = 200 if dtype == np.uint8 else 51234
    img = np.full((37, 53, 4), v, dtype)
    img[..., 3] = np.iinfo(dtype).max
    for n in (64, 32, 8, 1):
        lvl, q, t = R.resize_level(img, n)
        np.testing.assert_allclose(t[..., :3], v, rtol=0, atol=1e-9 * v)
        assert np.all(q[..., :3] == v) and np.all(q[..., 3] == np.iinfo(dtype).max)
        assert np.all(lvl[..., :3] == np.float32(v) / np.float32(np.iinfo(dtype).max))


def test_copy_level_is_x_over_255():
    img = np.random.default_rng(1).integers(0, 256, (64, 64, 4)).astype(np.uint8)
    lvl, q, _ = R.resize_level(img, 64)
    assert np.array_equal(q, img)
    assert np.array_equal(lvl, img.astype(np.float32) / np.float32(255.0))
    img16 = np.random.default_rng(2).integers(0, 65536, (8, 8, 4)).astype(np.uint16)
    assert np.array_equal(R.resize_level(img16, 8)[0], img16.astype(np.float32) / np.float32(65535.0))


@pytest.mark.parametrize("n_in,n_out", [(64, 8), (4096, 64), (48, 16), (30, 10), (16, 16)])
def test_centred_output_weights_sum_to_one_and_are_symmetric(n_in, n_out):
    """An output whose window lies inside the image, at an integer ratio (its centre c - 0.5 falls on a source texel or half-way
    between two): the weights sum to 1 and are symmetric about the centre."""
    left, count, w = R.axis_taps(n_in, n_out)
    o = n_out // 2
    ws = w[o, :count[o]]
    assert left[o] > 0 and left[o] + count[o] < n_in
    assert abs(ws.sum() - 1.0) < 1e-12
    nz = np.nonzero(np.abs(ws) > 1e-15)[0]
    core = ws[nz[0]:nz[-1] + 1]
    np.testing.assert_allclose(core, core[::-1], rtol=0, atol=1e-12)


def test_window_is_clipped_at_the_edges_not_replicated():
    """Output 0 of 64 -> 8 (ratio 8): the window would start at floor(4 - 24) = -20; it starts at 0, and the weights are the
    kernel's values there renormalised over the taps that exist.  An edge-replicating resampler would weight texel 0 by the
    sum of the dropped taps; a wrapping one would read the last columns."""
    left, count, w = R.axis_taps(64, 8)
    assert left[0] == 0 and count[0] == 28                   # ceil(4 + 24) = 28
    x = (np.arange(28) - 3.5) / 8.0
    raw = R.lanczos3(x)
    np.testing.assert_allclose(w[0, :28], raw / raw.sum(), rtol=0, atol=1e-15)
    # through a resize: a bright last column never reaches output column 0, while an edge-replicating filter would give 0 a
    # share of column 0's brightness beyond what the renormalised window gives
    img = np.zeros((64, 64, 4), np.uint8)
    img[:, 63, 0] = 255
    _, _, t = R.resize_level(img, 8)
    assert np.all(t[:, 0, 0] == 0.0)
    img = np.zeros((64, 64, 4), np.uint8)
    img[:, 0, 0] = 255
    _, _, t = R.resize_level(img, 8)
    np.testing.assert_allclose(t[:, 0, 0], 255.0 * w[0, 0], rtol=1e-12)


def test_default_tex_size_and_the_reference_f32_expression():
    """The wrapper's default is the largest power of two <= width.  For every width 1..16384 except 8192, the reference's f32
    expression 2^floor(ln(w) / ln(2)) gives the same with a correctly rounded logf (float64 log rounded to f32) and with
    numpy's float32 log.  At 8192 the two roundings differ (4096 vs 8192): that is why tex_size is an argument."""
    f64 = lambda x: np.log(np.float64(x))                     # noqa: E731
    f32 = lambda x: np.log(np.float32(x))                     # noqa: E731
    for w in range(1, 16385):
        want = R.default_tex_size(w)
        assert want <= w < 2 * want and want & (want - 1) == 0
        if w != 8192:
            assert R.reference_max_size(w, f64) == want == R.reference_max_size(w, f32), w
    assert R.reference_max_size(8192, f64) == 4096 and R.reference_max_size(8192, f32) == 8192


def test_wrapper_default_tex_size():
    from gswt_renderer_amd.renderer import GSWTRenderer
    calls = []

    class FakeLib:
        def gswt_proxy_configure_image(self, h, p, w, hh, fmt, n, g):
            calls.append((w, hh, fmt, n, g))
            return 0

    r = GSWTRenderer.__new__(GSWTRenderer)
    r._lib, r._h = FakeLib(), None
    for w in (1, 5, 64, 100, 8192, 8191):
        r.proxy_configure_image(np.zeros((3, w), np.uint8))
        assert calls[-1][3] == R.default_tex_size(w) and calls[-1][:3] == (w, 3, 0)
    r.proxy_configure_image(np.zeros((2, 9, 3), np.uint16), tex_size=32, grid_dim=7)
    assert calls[-1] == (9, 2, 1, 32, 7)
    with pytest.raises(TypeError):
        r.proxy_configure_image(np.zeros((4, 4, 4), np.float32))


def test_library_exports_the_mip_build_and_the_download():
    from gswt_renderer_amd import _lib as L
    lib = C.CDLL(os.path.join(ROOT, "gswt_renderer_amd", "lib", "libgswt_hip.so"))
    for name in ("gswt_proxy_configure_image", "gswt_proxy_download"):
        assert hasattr(lib, name) and name in L.SYMBOLS
    assert (L.GSWT_PROXY_SRC_RGBA8, L.GSWT_PROXY_SRC_RGBA16) == (0, 1)


def test_null_context_is_a_bad_argument():
    from gswt_renderer_amd import _lib as L
    lib = L.load()
    buf = np.zeros((4, 4, 4), np.uint8)
    assert lib.gswt_proxy_configure_image(None, buf.ctypes.data_as(C.c_void_p), 4, 4, 0, 4, 2048) == L.GSWT_ERR_BAD_ARG
    out = np.zeros(16, np.float32)
    assert lib.gswt_proxy_download(None, out.ctypes.data_as(C.c_void_p)) == L.GSWT_ERR_BAD_ARG


def test_renderer_has_the_mip_build_and_the_download():
    from gswt_renderer_amd.renderer import GSWTRenderer
    assert callable(getattr(GSWTRenderer, "proxy_configure_image", None))
    assert callable(getattr(GSWTRenderer, "proxy_download", None))
