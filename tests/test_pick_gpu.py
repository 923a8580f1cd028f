"""Pick output (gswt_render_pick / gswt_render_async_pick, include/gswt_hip.h) on the GPU.

Against the CPU reference tests/pick_ref.py on the golden cases (plane, HeightMap, Sphere surfaces, debug draw mode 1) and the reduced
c3-style grid, in both order modes, through gswt_set_draws and gswt_set_draws_merge_groups, with and without bg_rgba / bg_depth: at every
pixel the returned identity names an instance that covers the pixel in the reference, that instance's reference weight is within tol of
the pixel's maximum, the returned weight within tol of the instance's, the depth is the instance's vertex-stage depth bit for bit, the
identity is the reference's arg-max on every decisive pixel, and uncovered pixels carry the no-hit record (tests/pick_ref.py check_pick).
tol = 1e-4, the image contract (+ transmittance_eps with the early-out on).

Then full c3 frames (1920 x 1080) against themselves: colour and depth untouched by the pick output in every out_format, sync = async
(also replayed as a graph), short against long segments, shards, the weight bound against the colour's alpha, a re-run after a pair
overflow, and argument errors refused before anything is enqueued."""
import ctypes as C

import numpy as np
import pytest

from gswt_renderer_amd import _lib as L
from gswt_renderer_amd.renderer import PICK_DTYPE, PICK_NONE
from tests import frame_modes as FM
from tests import frame_outputs as FO
from tests import pick_ref as PR
from tests import test_pick_cpu as TC

pytestmark = pytest.mark.gpu
TOL = PR.TOL
FORMATS = [L.GSWT_OUT_RGBA32F, L.GSWT_OUT_RGBA8_UNORM, L.GSWT_OUT_BGRA8_UNORM, L.GSWT_VIDEO_NV12, L.GSWT_VIDEO_I420]


@pytest.mark.parametrize("merge", ["set_draws", "merge_groups"])
@pytest.mark.parametrize("bg", [False, True], ids=["clear", "bg"])
@pytest.mark.parametrize("order_mode", [0, 1], ids=["reference", "depth"])
@pytest.mark.parametrize("name", TC.GOLDEN)
def test_pick_matches_reference_golden_cases(renderer, name, order_mode, bg, merge):
    from gswt_renderer_amd import host
    from gswt_renderer_amd.pipeline import GSWTPipeline
    g, ev = TC.case(name), TC.events(name, order_mode, bg)
    W, Hh = g["W"], g["H"]
    bgc, bgd = TC.bg_of(name, bg)
    cu, vp = host.camera_uniforms(g["pos"], g["tgt"], (0, 0, 1), 45.0, 0.1, 2400.0, W, Hh)
    pipe = GSWTPipeline(g["verts"], host.user_data(**g["cfg"]), renderer=renderer, device_merge=merge == "merge_groups")
    pipe.update(g["pos"], vp)
    kw = dict(bg_rgba=bgc, bg_depth=bgd, order_mode=order_mode, draw_mode=int(g["su"].draw_mode))
    img, z, pick = pipe.render(cu, W, Hh, depth=True, pick=True, **kw)
    assert pick.shape == (Hh, W) and pick.dtype == PICK_DTYPE
    mi, en = PR.identities(g["draws"], merged_lod="single" if merge == "merge_groups" else "zero")
    PR.check_pick(pick, ev, g["sp"], mi, en, label=f"{name} order={order_mode} bg={bg} {merge}")
    # colour and depth of the same frame are what a frame without pick output writes
    img0, z0 = pipe.render(cu, W, Hh, depth=True, **kw)
    assert np.array_equal(img, img0) and np.array_equal(z.view(np.uint32), z0.view(np.uint32))
    # the early-out: the same checks at tol + eps
    eps = 1e-5
    _, pick_e = pipe.render(cu, W, Hh, pick=True, transmittance_eps=eps, **kw)
    PR.check_pick(pick_e, ev, g["sp"], mi, en, tol=TOL + eps, label=f"{name} order={order_mode} bg={bg} {merge} eps")


@pytest.mark.parametrize("bg", [False, True], ids=["clear", "bg"])
@pytest.mark.parametrize("order_mode", [0, 1], ids=["reference", "depth"])
@pytest.mark.parametrize("name", ["grid", "grid_dense"])
def test_pick_matches_reference_grid(renderer, name, order_mode, bg):
    """grid_dense: screen tiles of more than 256 pairs, so with GSWT_OPT_SEGMENT 256 k_combine's fold is what the reference checks."""
    g, ev = TC.case(name), TC.events(name, order_mode, bg)
    W, Hh = g["W"], g["H"]
    g["case"].upload(renderer)
    bgc, bgd = TC.bg_of(name, bg)
    cam = g["cam"].uniforms()
    img, pick = renderer.render(cam, g["su"], W, Hh, order_mode=order_mode, bg_rgba=bgc, bg_depth=bgd, pick=True)
    mi, en = PR.identities(g["draws"])
    assert len(np.unique(mi)) == 15                        # every draw of the grid is its own tile instance
    PR.check_pick(pick, ev, g["sp"], mi, en, label=f"{name} order={order_mode} bg={bg}")
    assert np.array_equal(img, renderer.render(cam, g["su"], W, Hh, order_mode=order_mode, bg_rgba=bgc, bg_depth=bgd))
    with renderer.options(SEGMENT=256):
        _, pick_s = renderer.render(cam, g["su"], W, Hh, order_mode=order_mode, bg_rgba=bgc, bg_depth=bgd, pick=True)
        lens = renderer.read_ranges().astype(np.int64)
        n_long = int(((lens[:, 1] - lens[:, 0]) > 256).sum())
        print(f"{name} order={order_mode} bg={bg}: longest tile list {int((lens[:, 1] - lens[:, 0]).max())} pairs, {n_long} tiles of several segments")
        assert n_long >= 4 or name == "grid"                  # grid_dense: k_combine's fold ran on several tiles
    PR.check_pick(pick_s, ev, g["sp"], mi, en, label=f"{name} order={order_mode} bg={bg} segment 256")


# ---- full frames against themselves (c3, 1920 x 1080) ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def c3():
    return FO.workload("c3")


def _sane(pick, Hh, W):
    assert pick.shape == (Hh, W) and pick.dtype == PICK_DTYPE
    hit = pick["weight"] > 0
    assert hit.mean() > 0.1                                    # the frame covers a good part of the screen
    assert (pick["weight"][hit] <= 1.0).all() and (pick["map_index"][hit] != PICK_NONE).all()
    assert (pick["map_index"][~hit] == PICK_NONE).all() and (pick["entry"][~hit] == PICK_NONE).all() and (pick["weight"][~hit] == 0).all()
    assert ((pick["depth"][hit] >= 0) & (pick["depth"][hit] < 1)).all()


def test_colour_and_depth_untouched_by_pick_output(renderer, c3):
    W, Hh, cu, su = FO.bind_workload(renderer, c3)
    bgd = FO.bg_depth(W, Hh)
    first = {}
    for fmt in FORMATS:
        for i, kw in enumerate((dict(), dict(transmittance_eps=1e-5, bg_depth=bgd), dict(order_mode=L.GSWT_ORDER_DEPTH))):
            want = renderer.render(cu, su, W, Hh, out_format=fmt, depth=True, **kw)
            got = renderer.render(cu, su, W, Hh, out_format=fmt, depth=True, pick=True, **kw)
            assert len(got) == len(want) + 1
            for a, b in zip(got, want):                        # the image (or its planes) and the depth image
                assert FM.same(a, b), (fmt, i)
            only = renderer.render(cu, su, W, Hh, out_format=fmt, pick=True, **kw)      # without the depth output
            assert FM.same(only[-1], got[-1]) and all(FM.same(a, b) for a, b in zip(only[:-1], want[:-1]))
            _sane(got[-1], Hh, W)
            if i == 1:                                         # no hit behind the proxy depth: z_bg exactly
                miss = got[-1]["weight"] == 0
                assert miss.any() and np.array_equal(got[-1]["depth"][miss].view(np.uint32), bgd[miss].view(np.uint32))
            # the pick image does not depend on the colour format
            if fmt == FORMATS[0]:
                first[i] = got[-1]
            else:
                assert FM.same(got[-1], first[i]), (fmt, i)
    # debug draw mode (float colours)
    su1 = c3["wang"].scene_uniforms()
    su1.draw_mode = 1
    want = renderer.render(cu, su1, W, Hh)
    img, pick = renderer.render(cu, su1, W, Hh, pick=True)
    assert FM.same(img, want) and FM.same(pick, first[0])


def test_weight_bounded_by_the_colours_alpha(renderer, c3):
    W, Hh, cu, su = FO.bind_workload(renderer, c3)
    for eps in (0.0, 1e-5):
        img, pick = renderer.render(cu, su, W, Hh, pick=True, transmittance_eps=eps)
        over = pick["weight"].astype(np.float64) - img[..., 3].astype(np.float64)       # alpha = 1 - T_final without a bg_rgba
        print(f"c3 eps={eps}: max(weight - alpha) = {over.max():.3e}, hit share = {(pick['weight'] > 0).mean():.3f}")
        assert over.max() <= TOL + eps
        # a covered pixel has a hit and an uncovered one has none
        assert np.array_equal(pick["weight"] > 0, img[..., 3] > 0)


def test_sync_async_and_graph_picks_are_identical(renderer, c3):
    import torch
    W, Hh, cu, su = FO.bind_workload(renderer, c3)
    bgd = FO.bg_depth(W, Hh)
    bgd_dev = torch.from_numpy(bgd).cuda()
    for kw, akw in ((dict(), dict()), (dict(transmittance_eps=1e-5, bg_depth=bgd), dict(transmittance_eps=1e-5, bg_depth_ptr=bgd_dev.data_ptr()))):
        img0, z0, p0 = renderer.render(cu, su, W, Hh, depth=True, pick=True, **kw)
        # frames in flight write their own pick buffers
        for o, z, p in FO.frames_in_flight(renderer, c3, ("depth", "pick"), [akw] * renderer.frame_slots()):
            assert FM.same(o, img0) and FM.same(z, z0) and FM.same(p, p0)
        # GSWT_OPT_GRAPH: pick frames replay as graphs like depth-output frames (two pick buffers in turn, a frame without pick between)
        assert FM.same(FO.check_side_graph_sequence(renderer, c3, "pick", p0, **akw), img0)


def test_short_against_long_segments(renderer, c3):
    """GSWT_OPT_SEGMENT 256 against 4096: weights within tol, and identities equal wherever the two runs' weights differ by less than tol
    and the winner is decisive in either run.  Decisive is shown from a run's own outputs: the weights of a pixel sum to its alpha (the f32
    colour's, 1 - T_final without a bg_rgba), so every other splat weighs at most alpha - weight, and weight > alpha / 2 + tol puts the
    winner more than 2 tol in front of any runner-up."""
    W, Hh, cu, su = FO.bind_workload(renderer, c3)
    bgd = FO.bg_depth(W, Hh)
    for kw in (dict(), dict(bg_depth=bgd, order_mode=L.GSWT_ORDER_DEPTH)):
        runs = []
        for seg in (256, 4096):
            with renderer.options(SEGMENT=seg):
                runs.append(renderer.render(cu, su, W, Hh, pick=True, **kw))
                if seg == 256:
                    assert renderer.timings()["n_pairs"] > 256 * renderer.timings()["n_tiles"] / 4      # many tiles have several segments
                    lens = renderer.read_ranges().astype(np.int64)
                    assert ((lens[:, 1] - lens[:, 0]) > 256).mean() > 0.1
        (img_a, a), (img_b, b) = runs
        dw = np.abs(a["weight"].astype(np.float64) - b["weight"])
        same = (a["map_index"] == b["map_index"]) & (a["entry"] == b["entry"])
        decisive = np.zeros(same.shape, bool)
        for img, p in runs:
            decisive |= p["weight"].astype(np.float64) > 0.5 * img[..., 3].astype(np.float64) + TOL
        must = decisive & (dw < TOL)
        print(f"c3 segments 256 / 4096: max|dw| = {dw.max():.3e}, decisive pixels {int(must.sum())} of {int((a['weight'] > 0).sum())} hit, "
              f"identities differ at {int((~same).sum())} pixels ({int((~same & must).sum())} decisive), largest |dw| among them "
              f"{dw[~same].max() if (~same).any() else 0.0:.3e}")
        assert dw.max() <= TOL
        assert must.mean() > 0.05                                 # the check covers a good part of the frame
        assert same[must].all()
        assert np.array_equal(a["depth"][same].view(np.uint32), b["depth"][same].view(np.uint32))
        _sane(a, Hh, W)


def test_shards_tile_the_pick_image(renderer, c3):
    W, Hh, cu, su = FO.bind_workload(renderer, c3)
    _, full = renderer.render(cu, su, W, Hh, pick=True)
    n = 8
    bw = renderer.shard_cols_padded(W, n)
    for r, part in enumerate(FO.check_side_shards_tile(renderer, c3, "pick", full, n, "cols")):
        assert not FM._raw(part[:, max(0, min(W, (r + 1) * bw) - r * bw):]).any()          # padding columns are zero bytes
    n = 3
    for r, part in enumerate(FO.check_side_shards_tile(renderer, c3, "pick", full, n, "rows")):
        assert not FM._raw(part[16 * len(range(r, (Hh + 15) // 16, n)):]).any()            # padding rows are zero bytes


def test_overflow_rerun_leaves_the_same_pick(renderer, c3):
    W, Hh, cu, su = FO.bind_workload(renderer, c3)
    img0, p0 = FO.check_side_overflow_rerun(renderer, c3, "pick")
    # the frames behind the re-run, with the depth image beside the pick and without the pick
    img2, z2, p2 = renderer.render(cu, su, W, Hh, depth=True, pick=True)
    img3, z3 = renderer.render(cu, su, W, Hh, depth=True)
    assert FM.same(p2, p0) and FM.same(img2, img0) and FM.same(img3, img0) and FM.same(z2, z3)


def test_argument_errors_refused_before_enqueue(renderer, c3):
    W, Hh, cu, su = FO.bind_workload(renderer, c3)
    lib, h = renderer._lib, renderer._h
    p = FO.side_refusal_probe(c3, "pick")
    cam, sc, cfg, pp, pd, od, ticket = p.cam, p.sc, p.cfg, p.host_ptr, p.dev_ptr, p.out_ptr, C.byref(p.ticket)
    # host path: a pick without out_rgba; a pick aliasing out_rgba; a pick aliasing out_depth
    assert lib.gswt_render_pick(h, cam, sc, C.byref(cfg), W, Hh, None, None, 0, None, None, pp, 0) == L.GSWT_ERR_BAD_ARG
    assert lib.gswt_render_pick(h, cam, sc, C.byref(cfg), W, Hh, None, None, 0, pp, None, pp, 0) == L.GSWT_ERR_BAD_ARG
    img = np.zeros((Hh, W, 4), np.float32)
    assert lib.gswt_render_pick(h, cam, sc, C.byref(cfg), W, Hh, None, None, 0, img.ctypes.data_as(C.c_void_p), pp, pp, 0) == L.GSWT_ERR_BAD_ARG
    p.untouched()
    assert not img.any()
    # device path: the same, plus a bad out_format -- nothing is written
    assert lib.gswt_render_async_pick(h, cam, sc, C.byref(cfg), W, Hh, None, None, None, None, pd, ticket) == L.GSWT_ERR_BAD_ARG
    assert lib.gswt_render_async_pick(h, cam, sc, C.byref(cfg), W, Hh, None, None, pd, None, pd, ticket) == L.GSWT_ERR_BAD_ARG
    assert lib.gswt_render_async_pick(h, cam, sc, C.byref(cfg), W, Hh, None, None, od, pd, pd, ticket) == L.GSWT_ERR_BAD_ARG
    cfg.out_format = 7
    assert lib.gswt_render_async_pick(h, cam, sc, C.byref(cfg), W, Hh, None, None, od, None, pd, ticket) == L.GSWT_ERR_BAD_ARG
    p.untouched()
    # and the ctx still renders
    _, p_ok = renderer.render(cu, su, W, Hh, pick=True)
    _sane(p_ok, Hh, W)
