"""Pick output (gswt_render_pick / gswt_render_async_pick, include/gswt_hip.h) on the GPU.

Against the CPU reference tests/pick_ref.py on the golden cases (plane, HeightMap, Sphere surfaces, debug draw mode 1) and the reduced
c3-style grid, in both order modes, through gswt_set_draws and gswt_set_draws_merge_groups, with and without bg_rgba / bg_depth: at every
pixel the returned identity names an instance that covers the pixel in the reference, that instance's reference weight is within tol of
the pixel's maximum, the returned weight within tol of the instance's, the depth is the instance's vertex-stage depth bit for bit, the
identity is the reference's arg-max on every decisive pixel, and uncovered pixels carry the no-hit record (tests/pick_ref.py check_pick).
tol = 1e-4, the image contract (+ transmittance_eps with the early-out on).

Then full c3 frames (1920 x 1080) against themselves: colour and depth untouched by the pick output in every out_format, sync = async
(also replayed as a graph), short against long segments, shards, the weight bound against the colour's alpha, a re-run after a pair
overflow, GSWT_OPT_COMPOSITE = 1, and argument errors refused before anything is enqueued."""
import ctypes as C

import numpy as np
import pytest

from gswt_renderer_amd import _lib as L
from gswt_renderer_amd.renderer import PICK_DTYPE, PICK_NONE
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
    renderer.set_option(L.GSWT_OPT_SEGMENT, 256)
    try:
        _, pick_s = renderer.render(cam, g["su"], W, Hh, order_mode=order_mode, bg_rgba=bgc, bg_depth=bgd, pick=True)
        lens = renderer.read_ranges().astype(np.int64)
        n_long = int(((lens[:, 1] - lens[:, 0]) > 256).sum())
        print(f"{name} order={order_mode} bg={bg}: longest tile list {int((lens[:, 1] - lens[:, 0]).max())} pairs, {n_long} tiles of several segments")
        assert n_long >= 4 or name == "grid"                  # grid_dense: k_combine's fold ran on several tiles
    finally:
        renderer.set_option(L.GSWT_OPT_SEGMENT, L.GSWT_DEFAULT_SEGMENT)
    PR.check_pick(pick_s, ev, g["sp"], mi, en, label=f"{name} order={order_mode} bg={bg} segment 256")


# ---- full frames against themselves (c3, 1920 x 1080) ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def c3():
    import bench
    w, wang, cu, vp, sort = bench.build_workload("c3")
    return dict(W=w["width"], H=w["height"], wang=wang, cu=cu, vp=vp, sort=sort, su=wang.scene_uniforms())


def _bind(renderer, s):
    s["wang"].upload_to(renderer)
    renderer.configure(None)
    renderer.set_draws(s["sort"].draws, s["sort"].merged_gs_index, s["sort"].merged_map_id, s["sort"].merged_lod_id)


def _bg_depth(W, Hh):
    return np.random.default_rng(3).uniform(0.99, 1.0, size=(Hh, W)).astype(np.float32)


def _raw(a):
    return np.ascontiguousarray(a).reshape(-1).view(np.uint8)


def _same(a, b):
    return np.array_equal(_raw(a), _raw(b))


def _sane(pick, Hh, W):
    assert pick.shape == (Hh, W) and pick.dtype == PICK_DTYPE
    hit = pick["weight"] > 0
    assert hit.mean() > 0.1                                    # the frame covers a good part of the screen
    assert (pick["weight"][hit] <= 1.0).all() and (pick["map_index"][hit] != PICK_NONE).all()
    assert (pick["map_index"][~hit] == PICK_NONE).all() and (pick["entry"][~hit] == PICK_NONE).all() and (pick["weight"][~hit] == 0).all()
    assert ((pick["depth"][hit] >= 0) & (pick["depth"][hit] < 1)).all()


def test_colour_and_depth_untouched_by_pick_output(renderer, c3):
    _bind(renderer, c3)
    W, Hh, cu, su = c3["W"], c3["H"], c3["cu"], c3["su"]
    bgd = _bg_depth(W, Hh)
    first = {}
    for fmt in FORMATS:
        for i, kw in enumerate((dict(), dict(transmittance_eps=1e-5, bg_depth=bgd), dict(order_mode=L.GSWT_ORDER_DEPTH))):
            want = renderer.render(cu, su, W, Hh, out_format=fmt, depth=True, **kw)
            got = renderer.render(cu, su, W, Hh, out_format=fmt, depth=True, pick=True, **kw)
            assert len(got) == len(want) + 1
            for a, b in zip(got, want):                        # the image (or its planes) and the depth image
                assert _same(a, b), (fmt, i)
            only = renderer.render(cu, su, W, Hh, out_format=fmt, pick=True, **kw)      # without the depth output
            assert _same(only[-1], got[-1]) and all(_same(a, b) for a, b in zip(only[:-1], want[:-1]))
            _sane(got[-1], Hh, W)
            if i == 1:                                         # no hit behind the proxy depth: z_bg exactly
                miss = got[-1]["weight"] == 0
                assert miss.any() and np.array_equal(got[-1]["depth"][miss].view(np.uint32), bgd[miss].view(np.uint32))
            # the pick image does not depend on the colour format
            if fmt == FORMATS[0]:
                first[i] = got[-1]
            else:
                assert _same(got[-1], first[i]), (fmt, i)
    # debug draw mode (float colours)
    su1 = c3["wang"].scene_uniforms()
    su1.draw_mode = 1
    want = renderer.render(cu, su1, W, Hh)
    img, pick = renderer.render(cu, su1, W, Hh, pick=True)
    assert _same(img, want) and _same(pick, first[0])


def test_weight_bounded_by_the_colours_alpha(renderer, c3):
    _bind(renderer, c3)
    W, Hh, cu, su = c3["W"], c3["H"], c3["cu"], c3["su"]
    for eps in (0.0, 1e-5):
        img, pick = renderer.render(cu, su, W, Hh, pick=True, transmittance_eps=eps)
        over = pick["weight"].astype(np.float64) - img[..., 3].astype(np.float64)       # alpha = 1 - T_final without a bg_rgba
        print(f"c3 eps={eps}: max(weight - alpha) = {over.max():.3e}, hit share = {(pick['weight'] > 0).mean():.3f}")
        assert over.max() <= TOL + eps
        # a covered pixel has a hit and an uncovered one has none
        assert np.array_equal(pick["weight"] > 0, img[..., 3] > 0)


def test_sync_async_and_graph_picks_are_identical(renderer, c3):
    import torch
    _bind(renderer, c3)
    W, Hh, cu, su = c3["W"], c3["H"], c3["cu"], c3["su"]
    bgd = _bg_depth(W, Hh)
    bgd_dev = torch.from_numpy(bgd).cuda()
    for kw, akw in ((dict(), dict()), (dict(transmittance_eps=1e-5, bg_depth=bgd), dict(transmittance_eps=1e-5, bg_depth_ptr=bgd_dev.data_ptr()))):
        img0, z0, p0 = renderer.render(cu, su, W, Hh, depth=True, pick=True, **kw)
        slots = renderer.frame_slots()
        outs = [torch.zeros((Hh, W, 4), dtype=torch.float32, device="cuda") for _ in range(slots)]
        zs = [torch.full((Hh, W), -1.0, dtype=torch.float32, device="cuda") for _ in range(slots)]
        ps = [torch.full((Hh, W, 4), -1, dtype=torch.int32, device="cuda") for _ in range(slots)]
        torch.cuda.synchronize()
        tickets = [renderer.render_async(cu, su, W, Hh, o.data_ptr(), out_depth_ptr=z.data_ptr(), out_pick_ptr=p.data_ptr(), **akw)
                   for o, z, p in zip(outs, zs, ps)]
        assert len(set(tickets)) == slots                       # frames in flight write their own pick buffers
        for t in tickets:
            renderer.render_wait(t)
        torch.cuda.synchronize()
        for o, z, p in zip(outs, zs, ps):
            assert _same(o.cpu().numpy(), img0) and _same(z.cpu().numpy(), z0) and _same(p.cpu().numpy(), p0)
        # GSWT_OPT_GRAPH: pick frames replay as graphs like depth-output frames (two pick buffers in turn, a frame without pick between)
        renderer.set_option(L.GSWT_OPT_TIMING, 0)
        renderer.set_option(L.GSWT_OPT_GRAPH, 1)
        try:
            launches0 = renderer.graph_stats()[0]
            for p in (ps[0], ps[1], None, ps[0]):
                if p is not None:
                    p.fill_(-1)
                    torch.cuda.synchronize()
                renderer.render_wait(renderer.render_async(cu, su, W, Hh, outs[0].data_ptr(), out_pick_ptr=p.data_ptr() if p is not None else 0, **akw))
            torch.cuda.synchronize()
            assert renderer.graph_stats()[0] - launches0 == 4
            assert _same(ps[0].cpu().numpy(), p0) and _same(ps[1].cpu().numpy(), p0) and _same(outs[0].cpu().numpy(), img0)
        finally:
            renderer.set_option(L.GSWT_OPT_GRAPH, 0)
            renderer.set_option(L.GSWT_OPT_TIMING, 2)


def test_short_against_long_segments(renderer, c3):
    """GSWT_OPT_SEGMENT 256 against 4096: weights within tol, and identities equal wherever the two runs' weights differ by less than tol
    and the winner is decisive in either run.  Decisive is shown from a run's own outputs: the weights of a pixel sum to its alpha (the f32
    colour's, 1 - T_final without a bg_rgba), so every other splat weighs at most alpha - weight, and weight > alpha / 2 + tol puts the
    winner more than 2 tol in front of any runner-up."""
    _bind(renderer, c3)
    W, Hh, cu, su = c3["W"], c3["H"], c3["cu"], c3["su"]
    bgd = _bg_depth(W, Hh)
    for kw in (dict(), dict(bg_depth=bgd, order_mode=L.GSWT_ORDER_DEPTH)):
        runs = []
        try:
            for seg in (256, 4096):
                renderer.set_option(L.GSWT_OPT_SEGMENT, seg)
                runs.append(renderer.render(cu, su, W, Hh, pick=True, **kw))
                if seg == 256:
                    assert renderer.timings()["n_pairs"] > 256 * renderer.timings()["n_tiles"] / 4      # many tiles have several segments
                    lens = renderer.read_ranges().astype(np.int64)
                    assert ((lens[:, 1] - lens[:, 0]) > 256).mean() > 0.1
        finally:
            renderer.set_option(L.GSWT_OPT_SEGMENT, L.GSWT_DEFAULT_SEGMENT)
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
    _bind(renderer, c3)
    W, Hh, cu, su = c3["W"], c3["H"], c3["cu"], c3["su"]
    _, full = renderer.render(cu, su, W, Hh, pick=True)
    n = 8
    bw = renderer.shard_cols_padded(W, n)
    p = np.zeros((Hh, W), PICK_DTYPE)
    for r in range(n):
        _, part = renderer.render(cu, su, W, Hh, shard=(r, n, "cols"), pick=True)
        assert part.shape == (Hh, bw)
        x0, x1 = r * bw, min(W, (r + 1) * bw)
        if x1 > x0:
            p[:, x0:x1] = part[:, :x1 - x0]
        assert not _raw(part[:, max(0, x1 - x0):]).any()          # padding columns are zero bytes
    assert _same(p, full)
    n = 3
    rows = renderer.shard_rows_padded(Hh, n)
    p = np.zeros((Hh, W), PICK_DTYPE)
    for r in range(n):
        _, part = renderer.render(cu, su, W, Hh, shard=(r, n), pick=True)
        assert part.shape == (rows, W)
        k = 0
        for ty in range(r, (Hh + 15) // 16, n):
            y0, y1 = ty * 16, min(Hh, ty * 16 + 16)
            p[y0:y1] = part[k * 16:k * 16 + (y1 - y0)]
            k += 1
        assert not _raw(part[k * 16:]).any()                      # padding rows are zero bytes
    assert _same(p, full)


def test_overflow_rerun_and_composite_variant_leave_the_same_pick(renderer, c3):
    import torch
    _bind(renderer, c3)
    W, Hh, cu, su = c3["W"], c3["H"], c3["cu"], c3["su"]
    img0, p0 = renderer.render(cu, su, W, Hh, pick=True)
    n_pairs = renderer.timings()["n_pairs"]
    try:
        renderer.set_option(L.GSWT_OPT_PAIR_CAP, 256)             # the next frame overflows and is re-run with grown buffers
        img1, p1 = renderer.render(cu, su, W, Hh, pick=True)
        assert renderer.timings()["n_pairs"] == n_pairs
        assert _same(img1, img0) and _same(p1, p0)
        renderer.set_option(L.GSWT_OPT_PAIR_CAP, 256)
        out = torch.zeros((Hh, W, 4), dtype=torch.float32, device="cuda")
        pt = torch.full((Hh, W, 4), -1, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        renderer.render_wait(renderer.render_async(cu, su, W, Hh, out.data_ptr(), out_pick_ptr=pt.data_ptr()))
        torch.cuda.synchronize()
        assert _same(pt.cpu().numpy(), p0)
    finally:
        renderer.set_option(L.GSWT_OPT_PAIR_CAP, 0)
    # GSWT_OPT_COMPOSITE = 1 (decoupled waves): a pick frame is composited by the default kernel, bit-identical
    renderer.set_option(L.GSWT_OPT_COMPOSITE, 1)
    try:
        img2, z2, p2 = renderer.render(cu, su, W, Hh, depth=True, pick=True)
        img3, z3 = renderer.render(cu, su, W, Hh, depth=True)
    finally:
        renderer.set_option(L.GSWT_OPT_COMPOSITE, 0)
    assert _same(p2, p0) and _same(img2, img0) and _same(img3, img0) and _same(z2, z3)


def test_argument_errors_refused_before_enqueue(renderer, c3):
    import torch
    _bind(renderer, c3)
    W, Hh, cu, su = c3["W"], c3["H"], c3["cu"], c3["su"]
    lib, h = renderer._lib, renderer._h
    cam = (C.c_char * 176).from_buffer_copy(bytes(cu))
    sc = (C.c_char * 160).from_buffer_copy(bytes(su))
    cfg = L.RenderConfig()
    cfg.culling_dist, cfg.lod_enable_mask = 1.0, 0xFFFFFFFF
    p = np.full((Hh, W, 4), 0x55555555, np.uint32)
    pp = p.ctypes.data_as(C.c_void_p)
    # host path: a pick without out_rgba; a pick aliasing out_rgba; a pick aliasing out_depth
    assert lib.gswt_render_pick(h, cam, sc, C.byref(cfg), W, Hh, None, None, 0, None, None, pp, 0) == L.GSWT_ERR_BAD_ARG
    assert lib.gswt_render_pick(h, cam, sc, C.byref(cfg), W, Hh, None, None, 0, pp, None, pp, 0) == L.GSWT_ERR_BAD_ARG
    img = np.zeros((Hh, W, 4), np.float32)
    assert lib.gswt_render_pick(h, cam, sc, C.byref(cfg), W, Hh, None, None, 0, img.ctypes.data_as(C.c_void_p), pp, pp, 0) == L.GSWT_ERR_BAD_ARG
    assert (p == 0x55555555).all() and not img.any()
    # device path: the same, plus a bad out_format -- nothing is written
    out = torch.zeros((Hh, W, 4), dtype=torch.float32, device="cuda")
    pt = torch.full((Hh, W, 4), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ticket = C.c_int(-7)
    pd, od = C.c_void_p(pt.data_ptr()), C.c_void_p(out.data_ptr())
    assert lib.gswt_render_async_pick(h, cam, sc, C.byref(cfg), W, Hh, None, None, None, None, pd, C.byref(ticket)) == L.GSWT_ERR_BAD_ARG
    assert lib.gswt_render_async_pick(h, cam, sc, C.byref(cfg), W, Hh, None, None, pd, None, pd, C.byref(ticket)) == L.GSWT_ERR_BAD_ARG
    assert lib.gswt_render_async_pick(h, cam, sc, C.byref(cfg), W, Hh, None, None, od, pd, pd, C.byref(ticket)) == L.GSWT_ERR_BAD_ARG
    cfg.out_format = 7
    assert lib.gswt_render_async_pick(h, cam, sc, C.byref(cfg), W, Hh, None, None, od, None, pd, C.byref(ticket)) == L.GSWT_ERR_BAD_ARG
    assert ticket.value == -7
    torch.cuda.synchronize()
    assert bool((pt == -1).all()) and not bool(out.any())
    # and the ctx still renders
    _, p_ok = renderer.render(cu, su, W, Hh, pick=True)
    _sane(p_ok, Hh, W)
