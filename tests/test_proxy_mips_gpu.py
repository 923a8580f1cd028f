"""The proxy mip build on the device (gswt_proxy_configure_image) against the float64 restatement of the reference's Lanczos3
chain (tests/proxy_mips_ref.py), the built chain through k_proxy, and the proxy state transitions."""
import ctypes as C

import numpy as np
import pytest

from gswt_renderer_amd import _lib as L
from oracle import gswt_oracle as orc
from tests import helpers as H
from tests import proxy_mips_ref as R

pytestmark = pytest.mark.gpu

# delta: how far the restatement's t (float64, source units) may lie from the kernel's f32 value.  With u = 2^-24, N taps and
# A = sum |w| (the L1 norm of an output's normalised weights, ~1.0-1.3 for Lanczos3) on each axis:
#  * a raw weight L(x) in f32 carries an absolute error of a few u (x rounded once, sinf within 2 ulp, two divisions; |L| <= 1,
#    |L'| < 2), so <= 16u; their f32 sum, in any order, adds at most N u sum|r|.  Since sum r ~ sratio and N < 6 sratio + 4,
#    the normalised weights move by at most u (128 + N A) in total weight mass (sum_i |dw_i| / A);
#  * the f32 accumulation of N products of values <= MAX' (any order: each partial sum rounds once) adds N u A MAX';
#  so one pass is off by at most u MAX' A (2 N A + 128).  The vertical pass sees MAX' = MAX, the horizontal MAX' = MAX A_v (the
#  intermediate rings past MAX) and carries the vertical error times A_h; the intermediate's f32 store is one more u.
#      delta = u MAX A_v A_h (2 N_v A_v + 2 N_h A_h + 256)
# e.g. RGBA8 100 x 80 -> 64: 0.009 codes; RGBA8 4096 -> 1: 0.25 codes; RGBA16 at thousands of taps the bound exceeds half a code
# and only the one-code check remains.  The bound is order independent, so it holds for the kernels' split sums.
U = 2.0 ** -24


def delta(w, h, n, mx):
    if (n, n) == (w, h):
        return 0.0
    _, cv, wv = R.axis_taps(h, n)
    _, ch, wh = R.axis_taps(w, n)
    av, ah = float(np.abs(wv).sum(1).max()), float(np.abs(wh).sum(1).max())
    return U * mx * av * ah * (2 * int(cv.max()) * av + 2 * int(ch.max()) * ah + 256)


def make_image(kind, w, h, dtype, seed=0):
    mx = np.iinfo(dtype).max
    if kind == "constant":
        img = np.empty((h, w, 4), dtype)
        img[...] = (int(0.3 * mx), int(0.7 * mx), mx, int(0.55 * mx))
        return img
    if kind == "noise":        # full-range noise: Lanczos ringing drives t past 0 and MAX (the clamp)
        return np.random.default_rng(seed).integers(0, mx + 1, (h, w, 4), dtype=np.int64).astype(dtype)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    y, x = (y + 0.5) / h, (x + 0.5) / w
    f = np.stack([0.5 + 0.45 * np.sin(2.1 * x + 3.3 * y + k) * np.cos(1.7 * x - 0.9 * y + 0.5 * k) for k in range(4)], -1)
    return np.rint(f * mx).astype(dtype)


def check_level(got, img, n, rows=None):
    """got: the device level [n, n, 4] f32.  Every texel within one code of the restatement, equal where the restatement's t is
    farther than delta from a rounding boundary, and exactly q / MAX in f32."""
    h, w = img.shape[:2]
    mx = R.maxval(img.dtype)
    _, q, t = R.resize_level(img, n, rows)
    g = got if rows is None else got[rows]
    gq = np.rint(g.astype(np.float64) * mx).astype(np.int64)
    assert np.array_equal(g, (gq.astype(np.float32) / np.float32(mx))), "level value is not code / MAX"
    d = np.abs(gq - q)
    assert d.max() <= 1, (n, int(d.max()))
    b = np.clip(np.round(t - 0.5) + 0.5, 0.5, mx - 0.5)        # the nearest rounding boundary inside [0, MAX]
    far = np.abs(t - b) > delta(w, h, n, mx)
    assert np.array_equal(gq[far], q[far]), (n, int((gq[far] != q[far]).sum()), far.sum())
    return far.mean()


def build(renderer, img, tex_size):
    renderer.proxy_configure_image(img, tex_size)
    chain = renderer.proxy_download()
    assert [c.shape for c in chain] == [(tex_size >> l, tex_size >> l, 4) for l in range(tex_size.bit_length())]
    return chain


def check_chain(renderer, img, tex_size, sample_above=1 << 20):
    chain = build(renderer, img, tex_size)
    for l, got in enumerate(chain):
        n = tex_size >> l
        if (n, n) == img.shape[1::-1]:
            assert np.array_equal(got, img.astype(np.float32) / np.float32(R.maxval(img.dtype)))
        elif n * n > sample_above:                            # >= 1 M texels: whole rows, seeded
            rows = np.sort(np.random.default_rng(n).choice(n, max(1, (1 << 20) // n), replace=False))
            check_level(got, img, n, rows)
        else:
            check_level(got, img, n)
    return chain


SMALL = [(1, 1, 1), (1, 37, 1), (37, 1, 32), (64, 64, 64), (100, 80, 64), (257, 129, 128), (300, 20, 256), (20, 300, 16)]


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
@pytest.mark.parametrize("w,h,n", SMALL)
def test_chain_matches_restatement(renderer, w, h, n, dtype):
    for k, kind in enumerate(("smooth", "noise", "constant")):
        check_chain(renderer, make_image(kind, w, h, dtype, seed=w * 7 + h + k), n)


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
def test_chain_3000x1700(renderer, dtype):
    for k, kind in enumerate(("smooth", "noise")):
        check_chain(renderer, make_image(kind, 3000, 1700, dtype, seed=11 + k), 2048)


@pytest.mark.parametrize("dtype,kind", [(np.uint8, "smooth"), (np.uint8, "noise"), (np.uint16, "noise")])
def test_chain_4096_thirteen_levels(renderer, dtype, kind):
    """The reference-size case: 4096^2 -> 13 levels; level 0 is the copy (bit-exact), 2048 is checked on 1 M texels in whole
    rows, 1024 and below in full."""
    img = make_image(kind, 4096, 4096, dtype, seed=5)
    chain = check_chain(renderer, img, 4096)
    assert len(chain) == 13


def test_copy_level_is_bit_exact(renderer):
    for dtype in (np.uint8, np.uint16):
        img = make_image("noise", 64, 64, dtype, seed=3)
        got = build(renderer, img, 64)[0]
        assert np.array_equal(got, img.astype(np.float32) / np.float32(np.iinfo(dtype).max))


def test_two_builds_are_bit_identical(renderer):
    img = make_image("noise", 4096, 4096, np.uint8, seed=9)
    a = build(renderer, img, 4096)
    b = build(renderer, img, 4096)
    for x, y in zip(a, b):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))


def test_grey_and_rgb_inputs_expand_like_to_rgba(renderer):
    g = make_image("smooth", 50, 40, np.uint8)[..., 0]
    rgba = np.stack([g, g, g, np.full_like(g, 255)], -1)
    want = build(renderer, rgba, 32)
    for x, y in zip(build(renderer, g, 32), want):
        assert np.array_equal(x, y)
    rgb = make_image("noise", 50, 40, np.uint16, seed=2)[..., :3]
    want = build(renderer, np.concatenate([rgb, np.full(rgb.shape[:2] + (1,), 65535, np.uint16)], -1), 32)
    for x, y in zip(build(renderer, rgb, 32), want):
        assert np.array_equal(x, y)


def _proxy_frames(renderer, surface, mips, grid_dim):
    """proxy_full then proxy_map into one colour / depth target (as tests/test_passes_gpu.py), device vs the oracle."""
    import torch
    W, Hh = 320, 208
    hm = np.random.default_rng(0).uniform(-1, 1, (8, 8)).astype(np.float32)
    renderer.configure(hm if surface == 1 else None)
    sky = np.random.default_rng(1).uniform(0, 1, (Hh, W, 4)).astype(np.float32)
    try:
        for pos, tgt in (((0.5, 0.3, 5.0), (1.0, 6.0, 2.5)), ((-3.0, 2.0, 1.2), (4.0, 9.0, 0.2))):
            cam = orc.Camera(W, Hh, pos, tgt, [0, 0, 1])
            rgba = torch.from_numpy(sky.copy()).cuda()
            depth = torch.zeros((Hh, W), dtype=torch.float32, device="cuda")
            torch.cuda.synchronize()
            ref_rgba, ref_depth = sky.copy(), np.ones((Hh, W), np.float32)
            common = dict(surface_type=surface, map_half_wh=(3, 4), center_coord=(1, -1), height_map_scale=(1.0, 1.0, 0.6))
            for k, u in enumerate((orc.proxy_uniforms(cam, map_proxy=0, height_offset=-0.5, width_scale=4.0, **common),
                                   orc.proxy_uniforms(cam, map_proxy=1, height_offset=-0.45, **common))):
                renderer.proxy_render(u, W, Hh, rgba.data_ptr(), depth.data_ptr(), clear_depth=(k == 0))
                orc.proxy_render(u, W, Hh, ref_rgba, ref_depth, mips, height_map=hm if surface == 1 else None, grid_dim=grid_dim)
            renderer.synchronize()
            got_d, got_c = depth.cpu().numpy(), rgba.cpu().numpy()
            assert 0.2 < (ref_depth < 1.0).mean() <= 1.0
            assert np.array_equal(got_d.view(np.uint32), ref_depth.view(np.uint32))
            assert H.max_abs_diff(got_c, ref_rgba) <= 1e-4
            yield got_c
    finally:
        renderer.configure(None)


@pytest.mark.parametrize("surface", [0, 1])
def test_built_chain_renders_like_the_oracle(renderer, surface):
    img = make_image("smooth", 100, 80, np.uint8)
    img[::9, :, 0] = 255                                      # some texture the proxy shows
    renderer.proxy_configure_image(img, 64, grid_dim=48)
    mips = renderer.proxy_download()
    for got in _proxy_frames(renderer, surface, mips, 48):
        assert got[..., :3].std() > 0.01


def _render_once(renderer):
    import torch
    W, Hh = 96, 64
    cam = orc.Camera(W, Hh, (0.5, 0.3, 5.0), (1.0, 6.0, 2.5), [0, 0, 1])
    u = orc.proxy_uniforms(cam, map_proxy=0, height_offset=-0.5, width_scale=4.0, surface_type=0, map_half_wh=(3, 4),
                           center_coord=(1, -1), height_map_scale=(1.0, 1.0, 0.6))
    rgba = torch.zeros((Hh, W, 4), dtype=torch.float32, device="cuda")
    depth = torch.zeros((Hh, W), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    renderer.proxy_render(u, W, Hh, rgba.data_ptr(), depth.data_ptr(), clear_depth=True)
    renderer.synchronize()
    return rgba.cpu().numpy(), depth.cpu().numpy()


def test_bad_arguments_keep_the_previous_proxy(renderer):
    img = make_image("noise", 40, 30, np.uint8, seed=4)
    renderer.proxy_configure_image(img, 32, grid_dim=48)
    before, chain = _render_once(renderer), renderer.proxy_download()
    lib, h = renderer._lib, renderer._h
    p = img.ctypes.data_as(C.c_void_p)
    for args in ((None, 40, 30, 0, 32, 48), (p, 0, 30, 0, 32, 48), (p, 16385, 30, 0, 32, 48), (p, 40, 0, 0, 32, 48),
                 (p, 40, -3, 0, 32, 48), (p, 40, 16385, 0, 32, 48), (p, 40, 30, 2, 32, 48), (p, 40, 30, -1, 32, 48),
                 (p, 40, 30, 0, 0, 48), (p, 40, 30, 0, 24, 48), (p, 40, 30, 0, 32768, 48), (p, 40, 30, 0, -32, 48),
                 (p, 40, 30, 0, 32, 0), (p, 40, 30, 0, 32, 32769)):
        assert lib.gswt_proxy_configure_image(h, *args) == L.GSWT_ERR_BAD_ARG, args
        assert b"gswt_proxy_configure_image" in lib.gswt_last_error(h)
    assert lib.gswt_proxy_download(h, None) == L.GSWT_ERR_BAD_ARG
    after = _render_once(renderer)
    np.testing.assert_array_equal(after[0], before[0])
    np.testing.assert_array_equal(after[1], before[1])
    for x, y in zip(renderer.proxy_download(), chain):
        assert np.array_equal(x, y)


def _synthetic_mips(ts):
    rng = np.random.default_rng(ts)
    return [rng.uniform(0, 1, (ts >> l, ts >> l, 4)).astype(np.float32) for l in range(ts.bit_length())]


def test_chain_configure_and_image_configure_replace_each_other(renderer):
    img = make_image("smooth", 90, 70, np.uint16)
    renderer.proxy_configure_image(img, 64, grid_dim=48)
    built = renderer.proxy_download()
    frame_built = _render_once(renderer)
    given = _synthetic_mips(16)
    renderer.proxy_configure(given, grid_dim=48)              # a finished chain after a build
    got = renderer.proxy_download()
    assert len(got) == len(given) and all(np.array_equal(x, y) for x, y in zip(got, given))
    frame_given = _render_once(renderer)
    assert not np.array_equal(frame_given[0], frame_built[0])
    renderer.proxy_configure_image(img, 64, grid_dim=48)      # a build after a finished chain
    got = renderer.proxy_download()
    assert len(got) == len(built) and all(np.array_equal(x, y) for x, y in zip(got, built))
    np.testing.assert_array_equal(_render_once(renderer)[0], frame_built[0])


def test_download_before_any_configure():
    from gswt_renderer_amd.renderer import GSWTRenderer, GSWTError
    r = GSWTRenderer(0)
    try:
        with pytest.raises(GSWTError) as e:
            r.proxy_download()
        assert e.value.code == L.GSWT_ERR_STATE
    finally:
        r.close()
