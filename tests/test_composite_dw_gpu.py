"""The retired values of GSWT_OPT_COMPOSITE and GSWT_OPT_ITEM_ORDER.  COMPOSITE = 1 was the decoupled-waves compositor, COMPOSITE = 2
k_composite<FOLD>, ITEM_ORDER = 1 the heaviest-first work-item table (all measured and removed: DESIGN.md sections 6 and 10).  gswt_set_option
still accepts them, and every frame under them has to be the default chain's -- k_composite + k_combine over a tile-order item table -- bit
for bit, counts included.  Per-pixel math: the reference's src/gswt.wgsl:425-435; blend state renderer.rs:118-129."""
import numpy as np
import pytest

from gswt_renderer_amd import _lib as L
from gswt_renderer_amd import host, synth
from gswt_renderer_amd.pipeline import GSWTPipeline
from tests import frame_outputs as FO
from tests.test_end_to_end_gpu import _run_case

pytestmark = pytest.mark.gpu


# ---- GSWT_OPT_COMPOSITE = 2: once k_composite<FOLD> (no k_combine launch; removed), now an alias of the default k_composite + k_combine
# chain.  It stays accepted, and its images and counts must stay bit-identical to option 0's.
def _variant(renderer, v, fn):
    with renderer.options(COMPOSITE=v):
        return fn()


@pytest.mark.parametrize("name,seg", [("c3", 1536), ("c3", 256), ("c3d", 512), ("c5", 512)])
def test_folded_combine_bit_identical_at_baseline_size(renderer, name, seg):
    import torch
    W, Hh, cu, su = FO.bind_workload(renderer, FO.workload(name))
    out = torch.empty((Hh, W, 4), dtype=torch.float32, device="cuda")
    with renderer.options(SEGMENT=seg):
        for eps in (0.0, 1e-5):
            def frame():
                out.fill_(-1.0)
                torch.cuda.synchronize()           # (torch's stream: nothing orders its fill against the frame slot's stream)
                renderer.render_wait(renderer.render_async(cu, su, W, Hh, out.data_ptr(), transmittance_eps=eps))
                return out.cpu().numpy().copy(), renderer.timings()
            (a, ta) = _variant(renderer, 0, frame)
            assert a[..., 3].max() > 0.5 and a.min() >= 0.0
            for rep in range(6):                         # the finishing order of the segments differs from launch to launch
                (b, tb) = _variant(renderer, 2, frame)
                assert np.array_equal(a, b), (name, seg, eps, rep, float(np.abs(a - b).max()))
                assert (tb["n_visible"], tb["n_pairs"]) == (ta["n_visible"], ta["n_pairs"])


@pytest.mark.parametrize("kw", [dict(bg=True), dict(bg=True, t_eps=1e-4), dict(render_config=dict(draw_mode=1)), dict(shard=3), dict(shard=2, shard_cols=True),
                                dict(order_mode=1, t_eps=1e-5)])
def test_folded_combine_variants(renderer, kw):
    cfg = dict(tile_map_half_wh=(3, 3), surface_type=0, lod_max_dist=20.0, tile_sort_type=3, merge_type=2)
    cam = ((4.2, 1.0, 1.2), (5.0, 3.0, 0.9))
    a, ref, _, _ = _variant(renderer, 0, lambda: _run_case(renderer, cfg, cam, 320, 240, lod0=2500, **kw))
    with renderer.options(SEGMENT=256):                  # many multi-segment tiles
        b, _, _, _ = _variant(renderer, 2, lambda: _run_case(renderer, cfg, cam, 320, 240, lod0=2500, **kw))
        c, _, _, _ = _variant(renderer, 0, lambda: _run_case(renderer, cfg, cam, 320, 240, lod0=2500, **kw))
    assert np.array_equal(b, c)                          # same segment length: bit-identical with and without k_combine
    assert np.abs(b.astype(np.float64) - ref).max() <= 1e-4 + kw.get("t_eps", 0.0)
    assert np.abs(a.astype(np.float64) - b).max() <= 2e-6 + kw.get("t_eps", 0.0)      # another segment length regroups the fold


@pytest.mark.parametrize("lod0", [2500, 10000])
@pytest.mark.parametrize("t_eps", [0.0, 1e-5])
def test_retired_options_leave_every_frame_as_the_defaults_do(renderer, t_eps, lod0):
    """_run_case's 320 x 240 scene through a pipeline of its own (one scene upload for all its frames) under the shortest segments: each
    retired value, alone and together, in both orders of the pairs, with and without the early-out.  At lod0 = 2500, the density of the
    tests above, the longest tile list has 142 pairs: every tile is one work item.  At lod0 = 10000 lists reach 568 pairs and 69 of the 300
    tiles have two or three segments (counted with the oracle's pair_rects), so k_combine runs on partials."""
    cfg = dict(tile_map_half_wh=(3, 3), surface_type=0, lod_max_dist=20.0, tile_sort_type=3, merge_type=2)
    cam = ((4.2, 1.0, 1.2), (5.0, 3.0, 0.9))
    W, Hh = 320, 240
    cu, vp = host.camera_uniforms(cam[0], cam[1], (0, 0, 1), 45.0, 0.1, 2400.0, W, Hh)
    pipe = GSWTPipeline(synth.make_tileset(n_lod=3, n_tile=16, lod0_count=lod0), host.user_data(**cfg), renderer=renderer)
    pipe.update(cam[0], vp)

    def frame(order_mode):
        img = pipe.render(cu, W, Hh, transmittance_eps=t_eps, order_mode=order_mode)
        t = renderer.timings()
        return img, (t["n_visible"], t["n_pairs"])

    with renderer.options(SEGMENT=256):
        for order_mode in (0, L.GSWT_ORDER_DEPTH):
            a, na = frame(order_mode)
            assert a[..., 3].max() > 0.5
            ranges = renderer.read_ranges().astype(np.int64)
            assert ((ranges[:, 1] - ranges[:, 0] > 256).sum() >= 50) == (lod0 == 10000)
            for opts in (dict(COMPOSITE=1), dict(COMPOSITE=2), dict(ITEM_ORDER=1), dict(COMPOSITE=1, ITEM_ORDER=1), dict(COMPOSITE=2, ITEM_ORDER=1)):
                with renderer.options(**opts):
                    b, nb = frame(order_mode)
                assert np.array_equal(a, b), (order_mode, opts, float(np.abs(a - b).max()))
                assert nb == na, (order_mode, opts)
