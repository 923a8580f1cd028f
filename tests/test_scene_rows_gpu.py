"""gswt_upload_scene_rows (scene preparation on the device) against the host path gswt_upload_scene(preload) +
gswt_upload_raw_depth(raw_depth_tables) of a full wang: the state both leave in a context, read back through
gswt_debug_read_scene, is the same byte for byte (chunk boxes and local bounds compared as floats, so +0 == -0), on tile sets
that reach the build's edge cases; c3 frames rendered from either scene are the same bit for bit; and the refusals."""
import ctypes as C

import numpy as np
import pytest

from gswt_renderer_amd import _lib as L
from gswt_renderer_amd import flypath, host, synth, workloads

pytestmark = pytest.mark.gpu

ITEMS = [L.GSWT_SCENE_TEX, L.GSWT_SCENE_RAW_DEPTH, L.GSWT_SCENE_RAW_TABLES, L.GSWT_SCENE_STATIC_LIST, L.GSWT_SCENE_LISTS]
FLOAT_ITEMS = [L.GSWT_SCENE_STATIC_BOXES, L.GSWT_SCENE_BOUNDS]


@pytest.fixture(scope="module")
def ctxs():
    from gswt_renderer_amd.renderer import GSWTRenderer
    a, b = GSWTRenderer(0), GSWTRenderer(0)
    yield a, b
    a.close(); b.close()


def _tileset_from_rows(rows):
    """rows[lod][tile] = [n, 32] uint8 -> TileSet"""
    lib = host.load()
    h = C.c_void_p()
    host._check(lib.gswt_tileset_create(len(rows), len(rows[0]), C.byref(h)))
    for l, lod in enumerate(rows):
        for t, r in enumerate(lod):
            r = np.ascontiguousarray(r, dtype=np.uint8)
            host._check(lib.gswt_tileset_set_rows(h, l, t, r.ctypes.data, r.shape[0]))
    return host.TileSet(h)


def _rows(xyz, scale, rng):
    n = xyz.shape[0]
    r = np.zeros((n, 32), np.uint8)
    f = np.zeros((n, 6), np.float32)
    f[:, :3] = xyz
    f[:, 3:] = scale
    r[:, :24] = f.view(np.uint8).reshape(n, 24)
    r[:, 24:] = rng.integers(0, 256, (n, 8), dtype=np.uint8)
    return r


def _hostile_rows():
    """Two LODs, six tiles: a 1-splat tile; one position shared by every splat (max == min: bucket 0); a depth span beyond 2^31
    (wrapping differences); -0.0 coordinates; scales that overflow the halves (Inf and NaN packing); a non-finite position; lists
    that cross several 256-entry chunks with an uneven last chunk."""
    rng = np.random.default_rng(7)
    sc = lambda n, s: np.full((n, 3), s, np.float32) * rng.uniform(0.5, 1.5, (n, 3)).astype(np.float32)
    pos = lambda n, w: rng.uniform(-w, w, (n, 3)).astype(np.float32)
    lod0, lod1 = [], []
    lod0.append(_rows(pos(1, 2.0), sc(1, 0.02), rng)); lod1.append(_rows(pos(1, 2.0), sc(1, 0.08), rng))
    same = np.tile(np.array([[1.25, -0.5, 0.75]], np.float32), (300, 1))
    lod0.append(_rows(same, sc(300, 0.02), rng)); lod1.append(_rows(same[:90], sc(90, 0.08), rng))
    wide = pos(700, 1.0e6)
    lod0.append(_rows(wide, sc(700, 0.02), rng)); lod1.append(_rows(wide[:170], sc(170, 0.08), rng))
    negz = pos(520, 2.0)
    negz[::3] = -0.0
    negz[1::7, 0] = -0.0
    lod0.append(_rows(negz, sc(520, 0.02), rng)); lod1.append(_rows(-np.abs(negz[:131]), sc(131, 0.08), rng))
    big = sc(400, 0.02)
    big[::10] = 300.0             # 4 s^2 > 65504: Inf halves
    big[5] = 1.0e20               # squares overflow f32: Inf - Inf -> NaN halves
    big1 = sc(120, 0.08)
    big1[3] = 1.0e22
    lod0.append(_rows(pos(400, 2.0), big, rng)); lod1.append(_rows(pos(120, 2.0), big1, rng))
    odd = pos(1000, 2.0)
    odd[17, 0] = np.inf
    odd[600, 1] = np.nan
    odd1 = pos(333, 2.0)
    odd1[5, 0] = -np.inf
    lod0.append(_rows(odd, sc(1000, 0.02), rng)); lod1.append(_rows(odd1, sc(333, 0.08), rng))
    return [lod0, lod1]


SETS = {
    "c1": lambda: host.TileSet.from_vertices(synth.make_tileset(n_lod=3, n_tile=16, lod0_count=50000)),
    "c3": lambda: host.TileSet.from_vertices(synth.make_tileset(n_lod=3, n_tile=16, lod0_count=9800)),
    "one_lod": lambda: host.TileSet.from_vertices(synth.make_tileset(n_lod=1, n_tile=16, lod0_count=3000)),
    "hostile": lambda: _tileset_from_rows(_hostile_rows()),
}


def _read_all(r):
    return {k: r.read_scene(k) for k in ITEMS + FLOAT_ITEMS}


def _compare(dev, ref):
    for k in ITEMS:
        assert dev[k] == ref[k], f"scene item {k} differs"
    for k in FLOAT_ITEMS:
        a, b = np.frombuffer(dev[k], np.float32), np.frombuffer(ref[k], np.float32)
        assert a.shape == b.shape and bool(np.all(a == b)), f"scene item {k} differs"


def _host_path(r, make):
    full = host.WangTile(make())
    full.upload_to(r)
    full.upload_raw_depth_to(r)
    return full


@pytest.mark.parametrize("name", ["c1", "c3", "one_lod", "hostile"])
def test_device_scene_matches_host_scene(ctxs, name):
    dev_r, ref_r = ctxs
    rows = host.WangTile(SETS[name](), rows_only=True)
    dev_r.upload_scene_rows(rows)
    full = _host_path(ref_r, SETS[name])
    dev, ref = _read_all(dev_r), _read_all(ref_r)
    _compare(dev, ref)
    if name == "hostile":
        boxes = np.frombuffer(dev[L.GSWT_SCENE_STATIC_BOXES], np.float32).reshape(-1, 6)
        assert np.isinf(boxes).any() and np.isfinite(boxes).any()       # the non-finite chunks and the others
        bounds = np.frombuffer(dev[L.GSWT_SCENE_BOUNDS], np.float32)
        assert bounds[0] < -3e38 and bounds[3] > 3e38                   # never cull
        lists = np.frombuffer(dev[L.GSWT_SCENE_LISTS], np.uint32).reshape(-1, 6)
        assert lists[:, 1].max() > 3 * 256 and (lists[:, 1] % 256 != 0).all()
        tex = np.frombuffer(dev[L.GSWT_SCENE_TEX], np.uint32).reshape(-1, 8)
        halves = np.concatenate([tex[:, 4:7] & 0xFFFF, tex[:, 4:7] >> 16]).ravel()
        assert ((halves & 0x7FFF) == 0x7C00).any() and ((halves & 0x7C00) == 0x7C00).sum() > ((halves & 0x7FFF) == 0x7C00).sum()
    rows.close(); full.close()


def test_second_upload_replaces_the_first(ctxs):
    dev_r, ref_r = ctxs
    a = host.WangTile(SETS["c3"](), rows_only=True)
    dev_r.upload_scene_rows(a)
    b = host.WangTile(SETS["one_lod"](), rows_only=True)
    dev_r.upload_scene_rows(b)
    full = _host_path(ref_r, SETS["one_lod"])
    _compare(_read_all(dev_r), _read_all(ref_r))
    a.close(); b.close(); full.close()


def test_refusals_before_anything_is_enqueued(ctxs):
    dev_r, _ = ctxs
    lib, h = dev_r._lib, dev_r._h
    vp = np.zeros(9 * 16, np.float32)
    row = np.zeros((1, 32), np.uint8)
    ptrs = (C.c_void_p * 4)(*([row.ctypes.data] * 4))
    cnt = np.ones(4, np.uint32)
    assert lib.gswt_upload_scene_rows(h, None, cnt.ctypes.data, 2, 2, vp.ctypes.data, 9) == L.GSWT_ERR_BAD_ARG
    nul = (C.c_void_p * 4)(row.ctypes.data, None, row.ctypes.data, row.ctypes.data)
    assert lib.gswt_upload_scene_rows(h, nul, cnt.ctypes.data, 2, 2, vp.ctypes.data, 9) == L.GSWT_ERR_BAD_ARG
    assert b"null rows" in lib.gswt_last_error(h)
    zero = np.array([1, 0, 1, 1], np.uint32)
    assert lib.gswt_upload_scene_rows(h, ptrs, zero.ctypes.data, 2, 2, vp.ctypes.data, 9) == L.GSWT_ERR_BAD_ARG
    ptrs17 = (C.c_void_p * 17)(*([row.ctypes.data] * 17))
    cnt17 = np.ones(17, np.uint32)
    assert lib.gswt_upload_scene_rows(h, ptrs17, cnt17.ctypes.data, 17, 1, vp.ctypes.data, 9) == L.GSWT_ERR_BAD_ARG
    assert b"16" in lib.gswt_last_error(h)
    huge = np.full(4, (1 << 26) + 1, np.uint32)          # 2^28 + 4 splats counted (the rows are never read)
    assert lib.gswt_upload_scene_rows(h, ptrs, huge.ctypes.data, 2, 2, vp.ctypes.data, 9) == L.GSWT_ERR_CAPACITY
    assert b"2^28" in lib.gswt_last_error(h)
    n_many = 65537
    ptrs_m = (C.c_void_p * n_many)(*([row.ctypes.data] * n_many))
    cnt_m = np.ones(n_many, np.uint32)
    assert lib.gswt_upload_scene_rows(h, ptrs_m, cnt_m.ctypes.data, 1, n_many, vp.ctypes.data, 9) == L.GSWT_ERR_CAPACITY
    assert b"lists" in lib.gswt_last_error(h)


def test_c3_frames_from_the_device_scene_are_bit_identical():
    from gswt_renderer_amd.pipeline import GSWTPipeline
    w = workloads.WORKLOADS["c3"]
    verts = synth.make_tileset(n_lod=w["n_lod"], n_tile=16, lod0_count=w["lod0"])
    user = workloads.user_data_for("c3")
    ref = GSWTPipeline(verts, user, device_merge=True)
    dev = GSWTPipeline(verts, user, device_preprocess=True)
    try:
        assert dev.wang.rows_only and dev.device_merge
        W, H = w["width"], w["height"]
        n_merged = 0
        for pos, target in flypath.sample(flypath.load("c3"), 4):
            cu, vp = host.camera_uniforms(pos, target, (0, 0, 1), 45.0, 0.1, 2400.0, W, H)
            assert ref.update(pos, vp, force_sort=True) and dev.update(pos, vp, force_sort=True)
            n_merged += len(dev.sort.groups)
            for order in (L.GSWT_ORDER_REFERENCE, L.GSWT_ORDER_DEPTH):
                a = ref.render(cu, W, H, order_mode=order)
                b = dev.render(cu, W, H, order_mode=order)
                assert a.tobytes() == b.tobytes()
                assert np.count_nonzero(a[..., 3]) > 0
        assert n_merged > 0
    finally:
        ref.renderer.close(); dev.renderer.close()


def _half_val(h):
    """gswt_upload_scene's decode of a stored half (Inf / NaN read as 0), exact in f32, widened to f64"""
    h = h.astype(np.uint32)
    e, fr = (h >> 10) & 0x1F, (h & 0x3FF).astype(np.float32)
    m = np.where(e == 0, fr * np.float32(2.98023223876953125e-08),
                 np.ldexp(np.float32(1.0) + fr / np.float32(1024.0), e.astype(np.int32) - 15).astype(np.float32))
    m = np.where(e == 31, np.float32(0.0), m).astype(np.float32)
    return np.where(h & 0x8000, -m, m).astype(np.float64)


def _cov_bound(tex):
    """per splat: the covariance bound of gswt_upload_scene (numpy's f64 sqrt is correctly rounded) and whether it took the PSD branch"""
    w = tex[:, 4:7].astype(np.uint32)
    xx, xy, xz = _half_val(w[:, 0] & 0xFFFF), _half_val(w[:, 0] >> 16), _half_val(w[:, 1] & 0xFFFF)
    yy, yz, zz = _half_val(w[:, 1] >> 16), _half_val(w[:, 2] & 0xFFFF), _half_val(w[:, 2] >> 16)
    tr_d = (xx + yy) + zz
    psd = (xx >= 0) & (yy >= 0) & (zz >= 0) & (xx * yy - xy * xy >= 0) & (xx * zz - xz * xz >= 0) & (yy * zz - yz * yz >= 0) & \
          (xx * (yy * zz - yz * yz) - xy * (xy * zz - yz * xz) + xz * (xy * yz - yy * xz) >= 0)
    fro = np.sqrt((((((xx * xx + yy * yy) + zz * zz)) + 2.0 * ((xy * xy + xz * xz) + yz * yz))))
    return np.where(psd, tr_d, (0.5 * (tr_d + 1.7320508075688772 * fro)) * (1.0 + 1e-6)).astype(np.float32), psd


def test_indefinite_covariance_bounds_match_the_host(ctxs):
    """The band-cull bound of an indefinite decoded covariance goes through an f64 sqrt: 96 one-splat scenes, each splat chosen
    non-PSD, so that every compared bound is one sqrt of the device against one of the host (and of numpy)."""
    dev_r, ref_r = ctxs
    rng = np.random.default_rng(11)
    n = 2048
    f = np.zeros((n, 6), np.float32)
    f[:, :3] = rng.uniform(-2, 2, (n, 3))
    f[:, 3:] = rng.uniform(0.01, 0.1, (n, 3))
    f[:, 3] = rng.uniform(50, 200, n)          # one axis whose 4 s^2 overflows the half: indefinite after the decode
    cand = np.zeros((n, 32), np.uint8)
    cand[:, :24] = f.view(np.uint8).reshape(n, 24)
    cand[:, 24:] = rng.integers(0, 256, (n, 8), dtype=np.uint8)
    want, psd = _cov_bound(host.generate_texture(cand))
    pick = np.flatnonzero(~psd)[:96]
    assert pick.size == 96
    for i in pick:
        rows = [[cand[i:i + 1]]]
        dev_w = host.WangTile(_tileset_from_rows(rows), rows_only=True)
        dev_r.upload_scene_rows(dev_w)
        full = _host_path(ref_r, lambda: _tileset_from_rows(rows))
        a = np.frombuffer(dev_r.read_scene(L.GSWT_SCENE_BOUNDS), np.float32)
        b = np.frombuffer(ref_r.read_scene(L.GSWT_SCENE_BOUNDS), np.float32)
        assert a[6].tobytes() == b[6].tobytes() == want[i].tobytes()
        dev_w.close(); full.close()


def test_upload_finishes_the_frames_in_flight_first():
    """A frame still in flight when the scene is replaced -- here one that overflows a pinned pair capacity, so that its re-run is
    enqueued when it is collected -- finishes against the scene it was submitted with."""
    import torch
    from gswt_renderer_amd.pipeline import GSWTPipeline
    w = workloads.WORKLOADS["c3"]
    verts = synth.make_tileset(n_lod=w["n_lod"], n_tile=16, lod0_count=w["lod0"])
    user = workloads.user_data_for("c3")
    ref = GSWTPipeline(verts, user, device_merge=True)
    dev = GSWTPipeline(verts, user, device_preprocess=True)
    small = host.WangTile(SETS["one_lod"](), rows_only=True)
    try:
        W, H = w["width"], w["height"]
        pos, target = flypath.sample(flypath.load("c3"), 4)[1]
        cu, vp = host.camera_uniforms(pos, target, (0, 0, 1), 45.0, 0.1, 2400.0, W, H)
        ref.update(pos, vp, force_sort=True); dev.update(pos, vp, force_sort=True)
        want = ref.render(cu, W, H)
        su = dev.wang.scene_uniforms()
        su.draw_mode, su.point_cloud_radius, su.use_clip, su.clip_height = 0, 0.0, 0, 0.0
        out = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
        dev.renderer.set_option(L.GSWT_OPT_PAIR_CAP, 4096)          # far below the frame's pairs: it is re-run when collected
        ticket = dev.renderer.render_async(cu, su, W, H, out.data_ptr())
        dev.renderer.upload_scene_rows(small)
        dev.renderer.render_wait(ticket)
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        assert np.count_nonzero(want[..., 3]) > 0
        assert got.tobytes() == want.tobytes()
    finally:
        small.close(); ref.renderer.close(); dev.renderer.close()
