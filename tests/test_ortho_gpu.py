"""Orthographic frames (GSWT_OPT_PROJECTION = 1, include/gswt_hip.h) on the GPU.  Frames are 72 x 40: 5 x 3 screen tiles, partial on
the right and bottom edges.  The scenes are the golden cases with the draws of their own perspective sort event, seen by a top-down
and an oblique orthographic camera (tests/ortho_ref.py).

The vertex stage against the float32 restatement bit for bit; the surface mappings against the oracle on the outputs the Jacobian
does not touch; image, depth and pick against the CPU references over the GPU's own projected records; a known-answer height field;
the same bits through graphs, frames in flight, compositor and cull variants, output formats and row shards; the refusals; and the
perspective path untouched by switching the option on and off."""
import ctypes as C

import numpy as np
import pytest

from gswt_renderer_amd import _lib as L
from gswt_renderer_amd import ortho
from gswt_renderer_amd.renderer import PICK_DTYPE, PICK_NONE, GSWTError, make_draw
from oracle import gswt_oracle as orc
from tests import depth_ref as DR
from tests import helpers as H
from tests import ortho_ref as OR
from tests import pick_ref as PR
from tests import special_splats as S
from tests import unorm8_ref as U8
from tests import yuv_ref as YUV
from tests.test_depth_out_gpu import TOL, ZTOL, _check_against_ref

pytestmark = pytest.mark.gpu
W, Hh = OR.W, OR.H
ORTHO, PERSP = L.GSWT_PROJECTION_ORTHO, L.GSWT_PROJECTION_PERSPECTIVE


@pytest.fixture(autouse=True)
def _defaults(renderer):
    """Every test leaves the shared context as it found it: perspective, default options."""
    yield
    for key, value in ((L.GSWT_OPT_PROJECTION, PERSP), (L.GSWT_OPT_STRICT_VS, 1), (L.GSWT_OPT_GRAPH, 0), (L.GSWT_OPT_TIMING, 2),
                       (L.GSWT_OPT_SEGMENT, L.GSWT_DEFAULT_SEGMENT), (L.GSWT_OPT_COMPOSITE, 0), (L.GSWT_OPT_NO_CHUNK_CULL, 0),
                       (L.GSWT_OPT_DEBUG_VARYINGS, 0), (L.GSWT_OPT_NO_LOD_PREFILTER, 0)):
        renderer.set_option(key, value)
    renderer.configure(None)


def _bind(renderer, g):
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


def _varyings(renderer, cu, su, projection=ORTHO):
    renderer.set_option(L.GSWT_OPT_DEBUG_VARYINGS, 1)
    try:
        renderer.render(cu, su, W, Hh, projection=projection)
        return renderer.read_projected().view(orc.SPLAT_DTYPE)
    finally:
        renderer.set_option(L.GSWT_OPT_DEBUG_VARYINGS, 0)


def _cam(which, g, name="case_plane"):
    args = OR.camera_args(which, lod_pos=g["pos"]) if name == "case_plane" else OR.surface_camera_args(name, which, lod_pos=g["pos"])
    return OR.ortho_camera_of(args)


def _persp(g):
    from gswt_renderer_amd import host
    return host.camera_uniforms(g["pos"], g["tgt"], (0, 0, 1), 45.0, 0.1, 2400.0, W, Hh)[0]


def _raw(a):
    return np.ascontiguousarray(a).reshape(-1).view(np.uint8)


def _same(a, b):
    return np.array_equal(_raw(a), _raw(b))


def _bits_equal(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


# ---- 1. the vertex stage, bit for bit ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", OR.CAMERAS)
def test_vertex_stage_is_bit_exact(renderer, which):
    g = OR.golden()
    _bind(renderer, g)
    cu, su, want = OR.plane_records(which)
    cam = _cam(which, g)
    assert bytes(cam.uniforms()) == bytes(cu)
    got = _varyings(renderer, cam.uniforms(), su)
    assert got.shape == want.shape
    assert np.array_equal(got["visible"], want["visible"])
    vis = want["visible"] == 1
    assert vis.sum() > 300
    for fld in ("ndc", "depth", "major", "minor", "rgba"):
        assert _bits_equal(got[fld][vis], want[fld][vis]), fld


# ---- 2. the surface mappings inside the FULL x ORTHO instantiations ------------------------------------------------------------------
@pytest.mark.parametrize("which", OR.CAMERAS)
@pytest.mark.parametrize("name", ["case_hmap", "case_sphere"])
def test_surfaces_agree_with_the_oracle_where_the_jacobian_plays_no_part(renderer, name, which):
    g = OR.golden(name)
    _bind(renderer, g)
    su = OR.scene_of(g)
    cu = _cam(which, g, name).uniforms()
    got = _varyings(renderer, cu, su)
    want = orc.project_draws(orc.Camera176.from_buffer_copy(bytes(cu)), su, g["pp"].tex, g["draws"], height_map=g["hm"])
    assert got.shape == want.shape
    both = (got["visible"] == 1) & (want["visible"] == 1)
    assert both.sum() > 150 and not ((got["visible"] == 1) & (want["visible"] == 0)).any()
    for fld in ("ndc", "depth", "rgba"):
        assert _bits_equal(got[fld][both], want[fld][both]), fld
    maj, mnr = got["major"][got["visible"] == 1].astype(np.float64), got["minor"][got["visible"] == 1].astype(np.float64)
    assert np.isfinite(maj).all() and np.isfinite(mnr).all()
    assert (np.hypot(maj[:, 0], maj[:, 1]) >= np.hypot(mnr[:, 0], mnr[:, 1])).all()


@pytest.mark.parametrize("which", OR.CAMERAS)
@pytest.mark.parametrize("name", ["case_hmap", "case_sphere"])
def test_surfaces_equal_the_oracle_bit_for_bit(renderer, name, which):
    """The same frames against the oracle's own orthographic stage (oracle.frame_mode(ortho=1); tests/test_pair_list_modes_cpu.py pins it to
    the float32 restatement on the plane): every output, the axes included, bit for bit, and the same `visible`."""
    g = OR.golden(name)
    _bind(renderer, g)
    su = OR.scene_of(g)
    cu = _cam(which, g, name).uniforms()
    got = _varyings(renderer, cu, su)
    block = orc.Camera176.from_buffer_copy(bytes(cu))
    with orc.frame_mode(ortho=1):
        want = orc.project_draws(block, su, g["pp"].tex, g["draws"], height_map=g["hm"])
        rects = orc.pair_rects(block, su, g["pp"].tex, g["draws"], W, Hh, height_map=g["hm"])
    assert got.shape == want.shape
    assert np.array_equal(got["visible"], rects["visible"])           # (the product's `visible`: the fragment setup passed too)
    vis = rects["visible"] == 1
    assert vis.sum() > 150
    for fld in ("ndc", "depth", "major", "minor", "rgba"):
        assert _bits_equal(got[fld][vis], want[fld][vis]), fld


# ---- 3. image, depth and pick against the CPU references over the GPU's own records --------------------------------------------------
def _image_case(renderer, which, order_mode, bg, splat_scale):
    g = OR.golden()
    _bind(renderer, g)
    su = OR.scene_of(g, splat_scale)
    cu = _cam(which, g).uniforms()
    sp = _varyings(renderer, cu, su)
    bgc, bgd = DR.bg_images(W, Hh) if bg else (None, None)
    kw = dict(order_mode=order_mode, bg_rgba=bgc, bg_depth=bgd)
    img, z, pick = renderer.render(cu, su, W, Hh, projection=ORTHO, depth=True, pick=True, **kw)
    t = renderer.timings()
    assert z.shape == (Hh, W) and pick.shape == (Hh, W) and pick.dtype == PICK_DTYPE
    ref_img, ref_z, n_cover = DR.composite(sp, W, Hh, splat_scale=splat_scale, with_cover=True, **kw)
    assert (n_cover > 0).mean() > 0.5 and ref_img[..., 3].max() > 0.5
    dz = _check_against_ref(img, z, ref_img, ref_z)
    ev = PR.composite(sp, W, Hh, splat_scale=splat_scale, **kw)
    mi, en = PR.identities(g["draws"])
    dw = PR.check_pick(pick, ev, sp, mi, en, label=f"ortho {which} order={order_mode} bg={bg} scale={splat_scale}")
    print(f"ortho {which} order={order_mode} bg={bg} scale={splat_scale}: visible {t['n_visible']} pairs {t['n_pairs']} max|dz| {dz:.3e} max|dw| {dw:.3e}")
    assert t["n_visible"] == int((sp["visible"] == 1).sum())
    # colour and depth are what frames without the other outputs write
    assert _same(img, renderer.render(cu, su, W, Hh, projection=ORTHO, **kw))
    return t


@pytest.mark.parametrize("bg", [False, True], ids=["clear", "bg"])
@pytest.mark.parametrize("order_mode", [0, 1], ids=["reference", "depth"])
@pytest.mark.parametrize("which", OR.CAMERAS)
def test_image_depth_and_pick_match_the_references(renderer, which, order_mode, bg):
    _image_case(renderer, which, order_mode, bg, OR.SPLAT_SCALE)


def test_image_depth_and_pick_with_several_segments_per_tile(renderer):
    renderer.set_option(L.GSWT_OPT_SEGMENT, 256)
    t = _image_case(renderer, "oblique", L.GSWT_ORDER_DEPTH, True, OR.SPLAT_SCALE_DENSE)
    assert t["n_pairs"] > 256 * t["n_tiles"] / 4          # many tiles have several segments
    lens = renderer.read_ranges().astype(np.int64)
    assert ((lens[:, 1] - lens[:, 0]) > 256).sum() >= 2


# ---- 4. a known-answer height field --------------------------------------------------------------------------------------------------
def test_known_answer_height_field(renderer):
    """Five opaque splats at known heights under a top_down camera of 4 px per world unit: the pick image's depth at each splat's centre
    pixel, through height_from_depth, is the splat's height.

    The bound, from the binary32 chain of that depth (all other terms of the three expressions are products with exact zeros):
      view z   cv.z = fl(z - z_top)                      1 rounding  (V[10] = 1, V[14] = -z_top exactly: z_top is a binary32 number)
      clip z   q.z  = fl(GP[10] * cv.z),  GP[10] = 0.5 fl(-2 / range)    2 roundings  (GP[14] = fl(0.5 * -1 + 0.5) = 0, q.w = 1 exactly)
      depth    q.z / q.w = q.z                           exact
    so depth = d (1 + e)^3 with |e| <= u = 2^-24 and d = (z_top - z) / range <= 1 the largest intermediate: |depth - d| <= 3 u (1 + 2 u) d,
    and the height, z_top - depth * range in binary64, is within 3 u (1 + 2 u) d range of z (+ 2^-50 for the binary64 steps)."""
    # (The splats are longer in y than in x.  vs_main takes the major axis' direction from (cov01, lambda1 - cov00), gswt.wgsl:245-250, which is
    # 0 / 0 for an exactly diagonal cov2d with cov00 >= cov11: such a splat draws nothing, in the shader as here.  A perspective view meets that
    # case only on the view axis; a straight-down orthographic one meets it for every exactly axis-aligned covariance.)
    z_top, z_bottom = 3.0, -1.0
    cam = ortho.top_down((0.0, 0.0), 5.0, z_top, z_bottom, W, Hh)
    assert cam.focal() == (4.0, 4.0)
    px = [(8, 6, 0.5), (30, 10, 1.25), (60, 8, -0.75), (20, 30, 2.5), (50, 31, 0.0)]          # (pixel x, pixel y, height)
    rows = [((( x + 0.5) / 4.0 - 9.0, 5.0 - (y + 0.5) / 4.0, z), S.diag_halves((0.2, 0.3, 0.25)), (200, 100 + 20 * k, 50, 255))
            for k, (x, y, z) in enumerate(px)]
    scene = S.raw_scene(rows)
    _, pd = scene.draws(map_index=7)
    renderer.configure(None)
    scene.upload(renderer)
    renderer.set_draws(pd)
    su = orc.scene_uniforms(num_lod=1)
    for order_mode in (0, 1):
        img, z, pick = renderer.render(cam.uniforms(), su, W, Hh, projection=ORTHO, depth=True, pick=True, order_mode=order_mode)
        assert renderer.timings()["n_visible"] == len(px)
        rng = z_top - z_bottom
        for k, (x, y, h) in enumerate(px):
            p = pick[y, x]
            assert p["map_index"] == 7 and p["entry"] == k and 1.0 - TOL <= p["weight"] <= 1.0
            d = (z_top - h) / rng
            bound = 3 * OR.U * (1 + 2 * OR.U) * d * rng + 2.0 ** -50
            got = float(ortho.height_from_depth(cam, p["depth"]))
            print(f"splat {k}: height {h} from depth {p['depth']!r} -> {got!r} (bound {bound:.3e})")
            assert abs(got - h) <= bound
            assert abs(float(z[y, x]) - float(p["depth"])) <= ZTOL      # an opaque splat's centre: weight 1, the depth image holds the same value
        free = pick["weight"] == 0
        assert free.sum() > 0.9 * W * Hh and (~free).sum() >= len(px)
        assert (pick["depth"][free] == 1.0).all() and (z[free] == 1.0).all()
        assert (pick["map_index"][free] == PICK_NONE).all() and (pick["entry"][free] == PICK_NONE).all()
        assert (ortho.height_from_depth(cam, pick["depth"][free]) == z_bottom).all()


# ---- 5. the same bits every way ------------------------------------------------------------------------------------------------------
@pytest.fixture()
def plain(renderer):
    """The plane case bound, and the plain synchronous frames (colour, depth, pick) of the two orthographic cameras and the case's
    perspective camera, depth order, over a background."""
    g = OR.golden()
    _bind(renderer, g)
    su = OR.scene_of(g)
    bgc, bgd = DR.bg_images(W, Hh)
    kw = dict(order_mode=L.GSWT_ORDER_DEPTH, bg_rgba=bgc, bg_depth=bgd)
    cams = {"top": (_cam("top", g).uniforms(), ORTHO), "oblique": (_cam("oblique", g).uniforms(), ORTHO), "persp": (_persp(g), PERSP)}
    frames = {k: renderer.render(cu, su, W, Hh, projection=pr, depth=True, pick=True, **kw) for k, (cu, pr) in cams.items()}
    renderer.set_option(L.GSWT_OPT_PROJECTION, PERSP)
    assert not _same(frames["top"][0], frames["oblique"][0]) and not _same(frames["top"][0], frames["persp"][0])
    for f in frames.values():
        assert (f[2]["weight"] > 0).mean() > 0.3
    return dict(g=g, su=su, kw=kw, bgc=bgc, bgd=bgd, cams=cams, frames=frames)


def _device_frames(renderer, s, seq, *, waves):
    """Submits the frames named in `seq` with render_async, `waves` at a time in flight, into buffers of their own; returns their
    (colour, depth, pick) as numpy arrays."""
    import torch
    bgc, bgd = torch.from_numpy(s["bgc"]).cuda(), torch.from_numpy(s["bgd"]).cuda()
    outs = [(torch.zeros((Hh, W, 4), dtype=torch.float32, device="cuda"), torch.full((Hh, W), -1.0, dtype=torch.float32, device="cuda"),
             torch.full((Hh, W, 4), -1, dtype=torch.int32, device="cuda")) for _ in seq]
    torch.cuda.synchronize()
    for i in range(0, len(seq), waves):
        tickets = []
        for name, (o, z, p) in zip(seq[i:i + waves], outs[i:i + waves]):
            cu, pr = s["cams"][name]
            tickets.append(renderer.render_async(cu, s["su"], W, Hh, o.data_ptr(), order_mode=L.GSWT_ORDER_DEPTH, bg_rgba_ptr=bgc.data_ptr(),
                                                 bg_depth_ptr=bgd.data_ptr(), out_depth_ptr=z.data_ptr(), out_pick_ptr=p.data_ptr(), projection=pr))
        assert len(set(tickets)) == len(tickets)
        # the option as it stands now must not reach the frames already submitted
        renderer.set_option(L.GSWT_OPT_PROJECTION, PERSP if seq[i] != "persp" else ORTHO)
        for t in tickets:
            renderer.render_wait(t)
    torch.cuda.synchronize()
    return [(o.cpu().numpy(), z.cpu().numpy(), p.cpu().numpy()) for o, z, p in outs]


def _assert_frames(got, seq, s, what):
    for k, (name, f) in enumerate(zip(seq, got)):
        want = s["frames"][name]
        assert _same(f[0], want[0]) and _same(f[1], want[1]) and _same(f[2], want[2]), (what, k, name)


def test_graph_replay_with_alternating_projections(renderer, plain):
    renderer.set_option(L.GSWT_OPT_TIMING, 0)
    renderer.set_option(L.GSWT_OPT_GRAPH, 1)
    launches0, rebuilds0, _ = renderer.graph_stats()
    # one frame at a time: slot 0 alternates; then two in flight: slots 0 and 1 each alternate from wave to wave
    seq1 = ["top", "persp", "oblique", "persp", "top"]
    _assert_frames(_device_frames(renderer, plain, seq1, waves=1), seq1, plain, "graph, one slot")
    seq2 = ["top", "persp", "persp", "oblique", "top", "persp"]
    _assert_frames(_device_frames(renderer, plain, seq2, waves=2), seq2, plain, "graph, two slots")
    launches, rebuilds, _ = renderer.graph_stats()
    assert launches - launches0 == len(seq1) + len(seq2)
    assert rebuilds - rebuilds0 >= 4                        # another k_project instantiation: the slot's graph is rebuilt


def test_async_frames_in_flight_keep_their_projection(renderer, plain):
    slots = renderer.frame_slots()
    seq = [("top", "persp", "oblique", "persp")[k % 4] for k in range(slots)]
    _assert_frames(_device_frames(renderer, plain, seq, waves=slots), seq, plain, "async")


@pytest.mark.parametrize("opt", [L.GSWT_OPT_NO_CHUNK_CULL, L.GSWT_OPT_COMPOSITE], ids=["no_chunk_cull", "composite_dw"])
def test_cull_and_compositor_variants(renderer, plain, opt):
    renderer.set_option(opt, 1)
    for name in ("top", "oblique"):
        cu, pr = plain["cams"][name]
        got = renderer.render(cu, plain["su"], W, Hh, projection=pr, depth=True, pick=True, **plain["kw"])
        _assert_frames([got], [name], plain, opt)


def test_output_formats(renderer, plain):
    for name in ("top", "oblique"):
        cu, pr = plain["cams"][name]
        f32 = plain["frames"][name][0]
        kw = dict(projection=pr, **plain["kw"])
        assert np.array_equal(renderer.render(cu, plain["su"], W, Hh, out_format=L.GSWT_OUT_RGBA8_UNORM, **kw), U8.rgba8(f32))
        assert np.array_equal(renderer.render(cu, plain["su"], W, Hh, out_format=L.GSWT_OUT_BGRA8_UNORM, **kw), U8.bgra8(f32))
        y, cbcr = renderer.render(cu, plain["su"], W, Hh, out_format=L.GSWT_VIDEO_NV12, **kw)
        wy, wc = YUV.nv12(f32)
        assert np.array_equal(y, wy) and np.array_equal(cbcr, wc)


def test_two_row_shards_tile_the_frame(renderer, plain):
    for name in ("top", "oblique"):
        cu, pr = plain["cams"][name]
        full = plain["frames"][name]
        rows = renderer.shard_rows_padded(Hh, 2)
        parts = [np.zeros((Hh, W, 4), np.float32), np.zeros((Hh, W), np.float32), np.zeros((Hh, W), PICK_DTYPE)]
        for r in range(2):
            got = renderer.render(cu, plain["su"], W, Hh, projection=pr, depth=True, pick=True, shard=(r, 2), **plain["kw"])
            assert got[0].shape == (rows, W, 4)
            k = 0
            for ty in range(r, (Hh + 15) // 16, 2):
                y0, y1 = ty * 16, min(Hh, ty * 16 + 16)
                for dst, src in zip(parts, got):
                    dst[y0:y1] = src[k * 16:k * 16 + (y1 - y0)]
                k += 1
        for a, b in zip(parts, full):
            assert _same(a, b), name


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals(renderer, plain):
    import torch
    lib, h = renderer._lib, renderer._h
    su = plain["su"]
    sc = (C.c_char * 160).from_buffer_copy(bytes(su))
    good = plain["cams"]["top"][0]

    def block(edit=None, base=good):
        cu = L.CameraUniforms.from_buffer_copy(bytes(base))
        if edit:
            edit(cu)
        return (C.c_char * 176).from_buffer_copy(bytes(cu))

    def cfg(**kw):
        c = L.RenderConfig()
        c.culling_dist, c.lod_enable_mask, c.order_mode = 1.0, 0xFFFFFFFF, L.GSWT_ORDER_DEPTH
        for k, v in kw.items():
            setattr(c, k, v)
        return c

    # option values
    for bad in (2, -1):
        assert lib.gswt_set_option(h, L.GSWT_OPT_PROJECTION, bad) == L.GSWT_ERR_BAD_ARG
        assert b"GSWT_OPT_PROJECTION" in lib.gswt_last_error(h)
    with pytest.raises(GSWTError):
        renderer.render(good, su, W, Hh, projection=2)

    def setfocal(k, v):
        def f(cu):
            cu.focal[k] = v
        return f

    cases = [("perspective matrix", block(base=plain["cams"]["persp"][0]), cfg(), None, b"affine"),
             ("focal 0", block(setfocal(0, 0.0)), cfg(), None, b"focal"),
             ("focal NaN", block(setfocal(1, float("nan"))), cfg(), None, b"focal"),
             ("focal inf", block(setfocal(0, float("inf"))), cfg(), None, b"focal"),
             ("sequence v2", block(), cfg(), (L.GSWT_OPT_STRICT_VS, 0), b"GSWT_OPT_STRICT_VS"),
             ("column shards", block(), cfg(shard_index=1, shard_count=2, shard_mode=L.GSWT_SHARD_COLUMNS), None, b"column")]
    out = np.full((Hh, W, 4), 7.0, np.float32)
    z = np.full((Hh, W), -1.0, np.float32)
    pk = np.full((Hh, W, 4), 0x55555555, np.uint32)
    o_d = torch.full((Hh, W, 4), 7.0, dtype=torch.float32, device="cuda")
    z_d = torch.full((Hh, W), -1.0, dtype=torch.float32, device="cuda")
    p_d = torch.full((Hh, W, 4), 0x55555555, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    renderer.set_option(L.GSWT_OPT_PROJECTION, ORTHO)
    for what, cam, c, opt, word in cases:
        if opt:
            renderer.set_option(*opt)
        try:
            assert lib.gswt_render_pick(h, cam, sc, C.byref(c), W, Hh, None, None, 0, vp(out), vp(z), vp(pk), 0) == L.GSWT_ERR_BAD_ARG, what
            assert word in lib.gswt_last_error(h), (what, lib.gswt_last_error(h))
            ticket = C.c_int(-7)
            assert lib.gswt_render_async_pick(h, cam, sc, C.byref(c), W, Hh, None, None, C.c_void_p(o_d.data_ptr()), C.c_void_p(z_d.data_ptr()),
                                              C.c_void_p(p_d.data_ptr()), C.byref(ticket)) == L.GSWT_ERR_BAD_ARG, what
            assert ticket.value == -7
        finally:
            if opt:
                renderer.set_option(opt[0], 1)
        torch.cuda.synchronize()
        assert (out == 7.0).all() and (z == -1.0).all() and (pk == 0x55555555).all(), what
        assert bool((o_d == 7.0).all()) and bool((z_d == -1.0).all()) and bool((p_d == 0x55555555).all()), what
        # the next valid frame renders
        cu, pr = plain["cams"]["top"]
        got = renderer.render(cu, su, W, Hh, projection=pr, depth=True, pick=True, **plain["kw"])
        _assert_frames([got], ["top"], plain, "after " + what)
    # row shards are not refused, and the perspective path takes its usual matrix with the option off
    renderer.render(good, su, W, Hh, projection=ORTHO, shard=(0, 2))
    renderer.render(plain["cams"]["persp"][0], su, W, Hh, projection=PERSP, shard=(1, 2, "cols"))


# ---- 7. perspective is untouched --------------------------------------------------------------------------------------------------------
def test_perspective_untouched_by_the_switch(renderer):
    g = OR.golden()
    _bind(renderer, g)
    su, cu = OR.scene_of(g), _persp(g)
    before = renderer.render(cu, su, W, Hh, depth=True, pick=True)
    v_before = _varyings(renderer, cu, su, projection=PERSP)
    renderer.render(_cam("top", g).uniforms(), su, W, Hh, projection=ORTHO)
    renderer.set_option(L.GSWT_OPT_PROJECTION, PERSP)
    after = renderer.render(cu, su, W, Hh, depth=True, pick=True)           # (no projection argument: the context is left as it is)
    for a, b in zip(before, after):
        assert _same(a, b)
    assert _same(v_before, _varyings(renderer, cu, su, projection=PERSP))
    assert (before[2]["weight"] > 0).mean() > 0.1
    # the perspective vertex stage still equals the oracle's
    want = orc.project_draws(orc.Camera176.from_buffer_copy(bytes(cu)), su, g["pp"].tex, g["draws"])
    vis = want["visible"] == 1
    assert np.array_equal(v_before["visible"][vis], want["visible"][vis])
    for fld in ("ndc", "depth", "major", "minor", "rgba"):
        assert _bits_equal(v_before[fld][vis], want[fld][vis]), fld
