"""What the GPU tests of the per-frame modes share (orthographic projection, the anti-aliasing filter, the atmosphere block, the
tile-style table, the sun shadow: tests/test_ortho_gpu.py, test_antialias_gpu.py, test_atmosphere_gpu.py, test_tile_style_gpu.py,
test_shadow_gpu.py, all of them stacked, test_mode_stack_gpu.py, and under the debug draw modes, test_debug_modes_gpu.py).  A mode is a
setting that a frame takes when it is submitted and keeps however it is run: the battery below renders a handful of named states of
one mode synchronously (`plain_frames`) and wants the same bytes back through graphs, frames in flight, the chunk cull switched
off, a pair-buffer overflow, output formats and shards.  Frames are 72 x 40 (tests/ortho_ref.py) on the golden cases.

A plain module: helpers, one descriptor (`Mode`), one function per shared check.  "The same" is always byte for byte (`same`)."""
import ctypes as C
from dataclasses import dataclass
from typing import Callable

import numpy as np

from gswt_renderer_amd import _lib as L
from gswt_renderer_amd import atmosphere
from gswt_renderer_amd.renderer import PICK_DTYPE, GSWTRenderer, make_draw
from oracle import gswt_oracle as orc
from tests import depth_ref as DR
from tests import helpers as H
from tests import ortho_ref as OR
from tests import pick_ref as PR
from tests import unorm8_ref as U8
from tests import yuv_ref as YUV

W, Hh = OR.W, OR.H
ORTHO, PERSP = L.GSWT_PROJECTION_ORTHO, L.GSWT_PROJECTION_PERSPECTIVE
TOL = 1e-4          # colour parity tolerance of the image tests
ZTOL = 1e-5         # depth against the reference, outside pixels whose colour already differs beyond TOL
FIELDS = ("ndc", "depth", "major", "minor", "rgba")


# ---- byte equality, the reference check ------------------------------------------------------------------------------------------------
def _raw(a):
    return np.ascontiguousarray(a).reshape(-1).view(np.uint8)


def same(a, b):
    return np.array_equal(_raw(a), _raw(b))


def bits_equal(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def bits_equal_or_nan(a, b):
    """bits_equal, but an element that is a NaN on both sides counts as equal whatever its payload (tests/test_special_splats_gpu.py's rule
    for records outside the benign region); an Inf, a zero's sign or a finite value must still match bit for bit."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())


def check_against_ref(img, z, ref_img, ref_z, tol=TOL):
    n = ref_z.size
    bad = (np.abs(img.astype(np.float64) - ref_img.astype(np.float64)) > tol).any(axis=-1)
    assert bad.sum() <= 2e-3 * n, int(bad.sum())
    dz = np.abs(z.astype(np.float64) - ref_z.astype(np.float64))
    assert dz[~bad].max() <= ZTOL, float(dz[~bad].max())
    return float(dz.max())


# ---- scenes, cameras, the context ------------------------------------------------------------------------------------------------------
def bind(renderer, g):
    """The case's scene and the oracle's draw list through gswt_upload_scene / gswt_set_draws, list for list (no LOD pre-filter), so that
    gswt_debug_read_projected is in the order of the oracle's instances."""
    pp = g["pp"]
    renderer.set_option(L.GSWT_OPT_NO_LOD_PREFILTER, 1)
    renderer.configure(g["hm"])
    renderer.upload_scene(pp.tex, pp.gs_index, pp.gs_lod_id)
    draws, m_gs, m_map, m_lod, off = [], [], [], [], 0
    for d in g["draws"]:
        tile = H.to_product_tile(d.tile)
        if d.base is not None:
            draws.append(make_draw(tile, base=d.base, lod=int(d.tile.tile_id[0])))
        else:
            n = len(d.gs_index)
            draws.append(make_draw(tile, merged_range=(off, n), merged_has_lod=d.lod_id is not None, lod=int(d.tile.tile_id[0])))
            m_gs.append(np.asarray(d.gs_index, np.uint32))
            m_map.append(np.asarray(d.map_id, np.uint32))
            m_lod.append(np.asarray(d.lod_id, np.uint32) if d.lod_id is not None else np.zeros(n, np.uint32))
            off += n
    cat = lambda a: np.concatenate(a) if a else None
    renderer.set_draws(draws, cat(m_gs), cat(m_map), cat(m_lod))


def ortho_cam(which, g, name="case_plane"):
    plane = name in ("case_plane", "case_plane_hostile")
    args = OR.camera_args(which, lod_pos=g["pos"]) if plane else OR.surface_camera_args(name, which, lod_pos=g["pos"])
    return OR.ortho_camera_of(args)


def persp_cam(g):
    from gswt_renderer_amd import host
    return host.camera_uniforms(g["pos"], g["tgt"], (0, 0, 1), 45.0, 0.1, 2400.0, W, Hh)[0]


def restore_defaults(renderer):
    """The shared context as every test has to leave it: no table, no atmosphere, no filter, perspective, default options."""
    renderer.set_tile_styles(None)
    renderer.set_atmosphere(atmosphere.OFF)
    for key, value in L.OPTION_DEFAULTS.items():
        renderer.set_option(key, value)
    renderer.configure(None)


def varyings(renderer, cu, su, **mode_kw):
    """(projected records, timings) of one debug-varyings frame under the mode keywords of GSWTRenderer.render."""
    with renderer.options(DEBUG_VARYINGS=1):
        renderer.render(cu, su, W, Hh, **mode_kw)
        return renderer.read_projected().view(orc.SPLAT_DTYPE), renderer.timings()


_VIEWS = {}


def view(name, cam, splat_scale=OR.SPLAT_SCALE):
    """(golden case, camera block, scene block, projection, reference records WITHOUT any mode but the projection) of case `name` under
    camera `cam`: "persp" (the oracle's vertex stage) or one of OR.CAMERAS (on the plane case tests/ortho_ref.py's restatement, on the
    HeightMap and Sphere cases and on the hostile ones (tests/hostile_cases.py) the oracle's own orthographic stage with the `visible`
    of its pair rectangles, the product's); computed once."""
    k = (name, cam, splat_scale)
    if k not in _VIEWS:
        g = OR.golden(name)
        if cam == "persp":
            cu, su = persp_cam(g), OR.scene_of(g, splat_scale)
            sp = orc.project_draws(orc.Camera176.from_buffer_copy(bytes(cu)), su, g["pp"].tex, g["draws"], height_map=g["hm"])
            _VIEWS[k] = (g, cu, su, PERSP, sp)
        elif name == "case_plane":
            _, su, sp = OR.plane_records(cam, splat_scale)
            _VIEWS[k] = (g, ortho_cam(cam, g).uniforms(), su, ORTHO, sp)
        else:
            cu, su = ortho_cam(cam, g, name).uniforms(), OR.scene_of(g, splat_scale)
            block = orc.Camera176.from_buffer_copy(bytes(cu))
            with orc.frame_mode(ortho=1):
                sp = orc.project_draws(block, su, g["pp"].tex, g["draws"], height_map=g["hm"]).copy()
                sp["visible"] = orc.pair_rects(block, su, g["pp"].tex, g["draws"], W, Hh, height_map=g["hm"])["visible"]
            _VIEWS[k] = (g, cu, su, ORTHO, sp)
    return _VIEWS[k]


# ---- frames out of shards (numpy only) ---------------------------------------------------------------------------------------------------
def new_outputs(H_, W_):
    """Zeroed (colour, depth, pick) of an H_ x W_ frame."""
    return [np.zeros((H_, W_, 4), np.float32), np.zeros((H_, W_), np.float32), np.zeros((H_, W_), PICK_DTYPE)]


def assemble_row_shards(parts_per_rank, H_, n):
    """The frame's outputs (colour, depth, pick, or the ones a rank's tuple holds) out of those of its n row shards: rank r holds the
    16-row screen tile rows r, r + n, ... one below the other, the frame's last one with the rows it has."""
    out = [np.zeros((H_,) + p.shape[1:], p.dtype) for p in parts_per_rank[0]]
    for r, got in enumerate(parts_per_rank):
        for k, ty in enumerate(range(r, (H_ + 15) // 16, n)):
            y0, y1 = ty * 16, min(H_, ty * 16 + 16)
            for dst, src in zip(out, got):
                dst[y0:y1] = src[k * 16:k * 16 + (y1 - y0)]
    return out


def assemble_column_bands(parts_per_rank, W_, band_w):
    """The frame's outputs (as in assemble_row_shards) out of those of its column bands: rank r holds columns r band_w ... of the
    frame, the last band as many as are left."""
    out = [np.zeros(p.shape[:1] + (W_,) + p.shape[2:], p.dtype) for p in parts_per_rank[0]]
    for r, got in enumerate(parts_per_rank):
        x0, x1 = r * band_w, min(W_, (r + 1) * band_w)
        for dst, src in zip(out, got):
            dst[:, x0:x1] = src[:, :x1 - x0]
    return out


# ---- a mode and its plain frames -----------------------------------------------------------------------------------------------------------
@dataclass
class Mode:
    states: dict                # state name -> (camera block, or None for the plain dict's "cu"; keywords of render / render_async[;
                                # a scene block in the place of the plain dict's "su": a state that lives there, such as draw_mode])
    set_state: Callable         # set_state(renderer, name) puts the context (not a frame) into a state
    on: object = None           # the name of the state that the single-frame checks use


def _submit_kw(s, mode, name):
    """(camera block, keywords, scene block) of a frame of state `name`."""
    cu, kw, *su = mode.states[name]
    return (s["cu"] if cu is None else cu), kw, (su[0] if su else s["su"])


def render_state(renderer, s, mode, name, **kw):
    """The synchronous frame of state `name` over the plain dict's scene (or the state's own) and background: (colour, depth, pick)
    unless `kw` says otherwise."""
    cu, mode_kw, su = _submit_kw(s, mode, name)
    kw = {"depth": True, "pick": True, **kw}
    return renderer.render(cu, su, W, Hh, **mode_kw, **s["kw"], **kw)


def plain_frames(renderer, mode, g, su, cu=None):
    """Binds case `g` and returns the plain dict: scene, depth order over a background, and under "frames" / "pairs" the synchronous
    frame (colour, depth, pick) and n_pairs of every state of `mode`.  The context is left in the last state."""
    bind(renderer, g)
    bgc, bgd = DR.bg_images(W, Hh)
    s = dict(g=g, cu=cu, su=su, kw=dict(order_mode=L.GSWT_ORDER_DEPTH, bg_rgba=bgc, bg_depth=bgd), bgc=bgc, bgd=bgd, frames={}, pairs={})
    for name in mode.states:
        s["frames"][name] = render_state(renderer, s, mode, name)
        s["pairs"][name] = renderer.timings()["n_pairs"]
    return s


def device_frames(renderer, s, seq, *, waves, submit_kw, then=None):
    """Submits the frames named in `seq` with render_async, `waves` at a time in flight, into buffers of their own; submit_kw(name) gives
    a frame's camera block and keywords, and optionally a scene block in the place of the plain dict's; then(names of the wave) runs
    between a wave's submits and its waits, and what it sets must not reach the frames already submitted.  Returns their (colour,
    depth, pick) as numpy arrays."""
    import torch
    bgc, bgd = torch.from_numpy(s["bgc"]).cuda(), torch.from_numpy(s["bgd"]).cuda()
    outs = [(torch.zeros((Hh, W, 4), dtype=torch.float32, device="cuda"), torch.full((Hh, W), -1.0, dtype=torch.float32, device="cuda"),
             torch.full((Hh, W, 4), -1, dtype=torch.int32, device="cuda")) for _ in seq]
    torch.cuda.synchronize()
    for i in range(0, len(seq), waves):
        tickets = []
        for name, (o, z, p) in zip(seq[i:i + waves], outs[i:i + waves]):
            cu, kw, *su = submit_kw(name)
            tickets.append(renderer.render_async(cu, su[0] if su else s["su"], W, Hh, o.data_ptr(), order_mode=L.GSWT_ORDER_DEPTH, bg_rgba_ptr=bgc.data_ptr(),
                                                 bg_depth_ptr=bgd.data_ptr(), out_depth_ptr=z.data_ptr(), out_pick_ptr=p.data_ptr(), **kw))
        assert len(set(tickets)) == len(tickets)
        if then is not None:
            then(seq[i:i + waves])
        for t in tickets:
            renderer.render_wait(t)
    torch.cuda.synchronize()
    return [(o.cpu().numpy(), z.cpu().numpy(), p.cpu().numpy()) for o, z, p in outs]


def assert_frames(got, seq, s, what):
    for k, (name, f) in enumerate(zip(seq, got)):
        want = s["frames"][name]
        assert same(f[0], want[0]) and same(f[1], want[1]) and same(f[2], want[2]), (what, k, name)


def check_in_flight(renderer, s, mode, seq, *, waves, then=None, what="async"):
    """The frames of `seq` through device_frames equal the plain ones.  then: a state, or a function of a wave's names that gives one,
    which the context is put into while the wave is in flight."""
    after = None if then is None else (lambda wave: mode.set_state(renderer, then(wave) if callable(then) else then))
    got = device_frames(renderer, s, seq, waves=waves, submit_kw=lambda name: _submit_kw(s, mode, name), then=after)
    assert_frames(got, seq, s, what)


# ---- the shared checks ---------------------------------------------------------------------------------------------------------------------
def check_graph_replay(renderer, s, mode, seq1, seq2, then=None):
    """seq1 one frame at a time (slot 0 changes state from frame to frame), then seq2 two in flight (slots 0 and 1 each change from
    wave to wave), as graph launches.  Returns what graph_stats() grew by: (launches, rebuilds, updates)."""
    renderer.set_option(L.GSWT_OPT_TIMING, 0)
    renderer.set_option(L.GSWT_OPT_GRAPH, 1)
    before = renderer.graph_stats()
    check_in_flight(renderer, s, mode, seq1, waves=1, then=then, what="graph, one slot")
    check_in_flight(renderer, s, mode, seq2, waves=2, then=then, what="graph, two slots")
    grown = tuple(b - a for a, b in zip(before, renderer.graph_stats()))
    assert grown[0] == len(seq1) + len(seq2)
    return grown


def check_with_option_on(renderer, s, mode, opt, names):
    """The named states under a plain option that may not change a frame (GSWT_OPT_NO_CHUNK_CULL: k_cull keeps every chunk of a surviving
    draw): the plain frames' bytes."""
    renderer.set_option(opt, 1)
    for name in names:
        assert_frames([render_state(renderer, s, mode, name)], [name], s, opt)


def check_overflow_rerun(renderer, s, mode, name, then):
    assert s["pairs"][name] > 256
    renderer.set_option(L.GSWT_OPT_PAIR_CAP, 256)             # the next frame overflows and is re-run with grown buffers
    got = render_state(renderer, s, mode, name)
    assert renderer.timings()["n_pairs"] == s["pairs"][name]
    assert_frames([got], [name], s, "overflow, synchronous")
    # ... and in flight, with the context in state `then` between submit and the wait that re-runs the frame
    renderer.set_option(L.GSWT_OPT_PAIR_CAP, 256)
    check_in_flight(renderer, s, mode, [name], waves=1, then=then, what="overflow, in flight")
    assert renderer.timings()["n_pairs"] == s["pairs"][name]


def check_output_formats(renderer, s, mode, names, bgra=False):
    for name in names:
        f32 = s["frames"][name][0]
        frame = lambda fmt: render_state(renderer, s, mode, name, depth=False, pick=False, out_format=fmt)
        assert np.array_equal(frame(L.GSWT_OUT_RGBA8_UNORM), U8.rgba8(f32)), name
        if bgra:
            assert np.array_equal(frame(L.GSWT_OUT_BGRA8_UNORM), U8.bgra8(f32)), name
        y, cbcr = frame(L.GSWT_VIDEO_NV12)
        wy, wc = YUV.nv12(f32)
        assert np.array_equal(y, wy) and np.array_equal(cbcr, wc), name


def check_row_shards(renderer, s, mode, n, names):
    rows = renderer.shard_rows_padded(Hh, n)
    for name in names:
        parts = [render_state(renderer, s, mode, name, shard=(r, n)) for r in range(n)]
        assert all(p[0].shape == (rows, W, 4) for p in parts)
        for a, b in zip(assemble_row_shards(parts, Hh, n), s["frames"][name]):
            assert same(a, b), (name, n)


def check_column_bands(renderer, s, mode, n, names):
    bw = renderer.shard_cols_padded(W, n)
    for name in names:
        parts = [render_state(renderer, s, mode, name, shard=(r, n, "cols")) for r in range(n)]
        assert all(p[0].shape == (Hh, bw, 4) for p in parts)
        for a, b in zip(assemble_column_bands(parts, W, bw), s["frames"][name]):
            assert same(a, b), (name, n)


def check_off_is_untouched(cam, on_kw, offs):
    """A context on which the mode was never set; then frames with it (`on_kw`); then each way of switching it off, `offs`: (label,
    off) with off(r) doing what it takes on the context and returning the keywords of the next frame.  That frame is the first one
    byte for byte -- colour, depth, pick, counts -- and the vertex stage is the reference's bit for bit, `visible` included."""
    g, cu, su, proj, unf = view("case_plane", cam)
    vis = unf["visible"] == 1
    r = GSWTRenderer(0)
    try:
        bind(r, g)
        bgc, bgd = DR.bg_images(W, Hh)
        kw = dict(order_mode=L.GSWT_ORDER_DEPTH, bg_rgba=bgc, bg_depth=bgd, projection=proj, depth=True, pick=True)
        before = r.render(cu, su, W, Hh, **kw)
        t0 = r.timings()
        assert (before[2]["weight"] > 0).mean() > 0.3
        on = r.render(cu, su, W, Hh, **on_kw, **kw)
        assert not same(on[0], before[0])
        for _ in range(2):                                      # (no argument: the context keeps the mode)
            assert same(r.render(cu, su, W, Hh, **kw)[0], on[0])
        for label, off in offs:
            after = r.render(cu, su, W, Hh, **off(r), **kw)
            t1 = r.timings()
            for a, b in zip(before, after):
                assert same(a, b), label
            assert (t0["n_visible"], t0["n_pairs"]) == (t1["n_visible"], t1["n_pairs"]), label
            got, _ = varyings(r, cu, su, projection=proj)
            assert np.array_equal(got["visible"] == 1, vis), label
            for fld in FIELDS:
                assert bits_equal(np.ascontiguousarray(got[fld][vis]), np.ascontiguousarray(unf[fld][vis])), (label, fld)
    finally:
        r.close()


def frame_blocks(cu, su, **cfg_kw):
    """The camera and scene blocks and a RenderConfig (depth order, everything else default but `cfg_kw`) as the C ABI takes them."""
    cfg = L.RenderConfig()
    cfg.culling_dist, cfg.lod_enable_mask, cfg.order_mode = 1.0, 0xFFFFFFFF, L.GSWT_ORDER_DEPTH
    for k, v in cfg_kw.items():
        setattr(cfg, k, v)
    return (C.c_char * 176).from_buffer_copy(bytes(cu)), (C.c_char * 160).from_buffer_copy(bytes(su)), cfg


def refusal_probe(renderer):
    """(refused, rendered) over host and device outputs (colour, depth, pick) filled with sentinels.  refused(cam, sc, cfg, needles, what):
    gswt_render_pick and gswt_render_async_pick both return GSWT_ERR_BAD_ARG, with every needle in the message of the first; no ticket is
    given and no output byte has changed.  rendered(cam, sc, cfg): gswt_render_pick succeeds; returns whether the host colour changed."""
    import torch
    lib, h = renderer._lib, renderer._h
    out = np.full((Hh, W, 4), 7.0, np.float32)
    z = np.full((Hh, W), -1.0, np.float32)
    pk = np.full((Hh, W, 4), 0x55555555, np.uint32)
    o_d = torch.full((Hh, W, 4), 7.0, dtype=torch.float32, device="cuda")
    z_d = torch.full((Hh, W), -1.0, dtype=torch.float32, device="cuda")
    p_d = torch.full((Hh, W, 4), 0x55555555, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    vp = lambda a: a.ctypes.data_as(C.c_void_p)

    def refused(cam, sc, cfg, needles, what):
        assert lib.gswt_render_pick(h, cam, sc, C.byref(cfg), W, Hh, None, None, 0, vp(out), vp(z), vp(pk), 0) == L.GSWT_ERR_BAD_ARG, what
        assert all(needle in lib.gswt_last_error(h) for needle in needles), (what, lib.gswt_last_error(h))
        ticket = C.c_int(-7)
        assert lib.gswt_render_async_pick(h, cam, sc, C.byref(cfg), W, Hh, None, None, C.c_void_p(o_d.data_ptr()), C.c_void_p(z_d.data_ptr()),
                                          C.c_void_p(p_d.data_ptr()), C.byref(ticket)) == L.GSWT_ERR_BAD_ARG, what
        assert ticket.value == -7
        torch.cuda.synchronize()
        assert (out == 7.0).all() and (z == -1.0).all() and (pk == 0x55555555).all(), what
        assert bool((o_d == 7.0).all()) and bool((z_d == -1.0).all()) and bool((p_d == 0x55555555).all()), what

    def rendered(cam, sc, cfg):
        assert lib.gswt_render_pick(h, cam, sc, C.byref(cfg), W, Hh, None, None, 0, vp(out), vp(z), vp(pk), 0) == L.GSWT_OK
        return not (out == 7.0).all()

    return refused, rendered


def check_refused(renderer, refused, cam, sc, cfg, needles, what, opt=None):
    """refused(...) with the options `opt` (keywords of GSWTRenderer.options) set for the two calls and put back whatever they do."""
    with renderer.options(**(opt or {})):
        refused(cam, sc, cfg, needles, what)


def check_v2_refused_at_submit(renderer, s, mode, names, needles, off="off"):
    """Under each state of `names`, a frame of vertex-stage sequence v2 (GSWT_OPT_STRICT_VS = 0) is refused at submit (refusal_probe), and
    the next frame renders with the state still in force.  In state `off` sequence v2 renders."""
    refused, rendered = refusal_probe(renderer)
    cam, sc, cfg = frame_blocks(s["cu"], s["su"])
    for name in names:
        mode.set_state(renderer, name)
        check_refused(renderer, refused, cam, sc, cfg, needles, name, opt=dict(STRICT_VS=0))
        got = renderer.render(s["cu"], s["su"], W, Hh, depth=True, pick=True, **s["kw"])
        assert_frames([got], [name], s, ("after the refused v2 frame", name))
    mode.set_state(renderer, off)
    renderer.set_option(L.GSWT_OPT_STRICT_VS, 0)
    assert rendered(cam, sc, cfg)


def image_case(renderer, cam, order_mode, bg, splat_scale, mode_kw, label, min_cover=0.3, name="case_plane", scene=None, tol=TOL,
               transmittance_eps=0.0):
    """Image, depth and pick of case `name` (the plane case unless said otherwise) under `cam` and the mode keywords against
    tests/depth_ref.py and tests/pick_ref.py over the GPU's own projected records; the context keeps the mode from the debug-varyings
    frame on.  Returns what the caller's own checks need: timings `t`, the frame's `img` and `pick`, `again(**kw)`, the same view and
    background rendered once more, and the debug-varyings frame's records `sp` and timings `t_debug`.
    scene: scene(su) gives the scene block the frames are rendered with, from the view's own (a draw mode, a point-cloud radius);
    transmittance_eps: of the frames, with `tol` the colour tolerance that goes with it."""
    g, cu, su, proj, _ = view(name, cam, splat_scale)
    if scene is not None:
        su = scene(su)
    bind(renderer, g)
    sp, t_debug = varyings(renderer, cu, su, projection=proj, **mode_kw)
    bgc, bgd = DR.bg_images(W, Hh) if bg else (None, None)
    kw = dict(order_mode=order_mode, bg_rgba=bgc, bg_depth=bgd)
    again = lambda **more: renderer.render(cu, su, W, Hh, projection=proj, transmittance_eps=transmittance_eps, **kw, **more)
    img, z, pick = again(depth=True, pick=True)
    t = renderer.timings()
    assert z.shape == (Hh, W) and pick.shape == (Hh, W) and pick.dtype == PICK_DTYPE
    ref_img, ref_z, n_cover = DR.composite(sp, W, Hh, splat_scale=splat_scale, with_cover=True, **kw)
    assert (n_cover > 0).mean() > min_cover and ref_img[..., 3].max() > 0.5
    dz = check_against_ref(img, z, ref_img, ref_z, tol)
    ev = PR.composite(sp, W, Hh, splat_scale=splat_scale, **kw)
    mi, en = PR.identities(g["draws"])
    label = f"{label} {cam} order={order_mode} bg={bg} scale={splat_scale}"
    dw = PR.check_pick(pick, ev, sp, mi, en, label=label)
    print(f"{label}: visible {t['n_visible']} pairs {t['n_pairs']} max|dz| {dz:.3e} max|dw| {dw:.3e}")
    assert t["n_visible"] == int((sp["visible"] == 1).sum())
    assert same(img, again())                                   # colour is what a frame without the other outputs writes, twice the same
    return dict(t=t, img=img, pick=pick, again=again, sp=sp, t_debug=t_debug)
