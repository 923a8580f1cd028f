"""gswt_wang_new_rows (the rows-only WangTile whose texture, raw depths and base lists are built on the device) against
gswt_wang_new: the same normalised rows, tile bases, LOD scales, merge offsets and presort matrices, the same worker output
(configure / build_tiles / sort_tiles with device merge, worker config counts), and the calls it refuses."""
import ctypes as C

import numpy as np
import pytest

from gswt_renderer_amd import _lib as L
from gswt_renderer_amd import host, synth

CAMERAS = [((2.0, 2.0, 14.0), (2.0, 6.0, 0.0)), ((30.0, -10.0, 6.0), (8.0, 12.0, 0.0)), ((-5.0, 40.0, 3.0), (0.0, 0.0, 0.0))]


def _pair(verts):
    return host.WangTile(host.TileSet.from_vertices(verts)), host.WangTile(host.TileSet.from_vertices(verts), rows_only=True)


def _user(kind, n_tile):
    common = dict(tile_sort_type=host.SORT_GRAPH, merge_type=host.MERGE_EDGE, lod_blending=True, lod_transition_width_ratio=0.05,
                  merge_topk=100, merge_dot_threshold=0.2, lod_max_dist=24.0 * 4.0)
    if kind == "sphere":
        return host.user_data(tile_map_half_wh=(10, 4), surface_type=host.SURFACE_SPHERE, sphere_radius=12.7, **common)
    if kind == "heightmap":
        return host.user_data(tile_map_half_wh=(6, 6), surface_type=host.SURFACE_HEIGHTMAP, height_map_scale=(1.0, 1.0, 0.25), **common)
    return host.user_data(tile_map_half_wh=(6, 6), surface_type=host.SURFACE_NONE, **common)


def _draw_bytes(s):
    return [bytes(d) for d in s.draws], [bytes(g) for g in s.groups], [bytes(m) for m in s.members], [bytes(t) for t in s.tiles]


SETS = {
    "c3": dict(n_lod=3, n_tile=16, lod0_count=9800),     # c3's synthetic tile set (205 792 splats)
    "one_lod": dict(n_lod=1, n_tile=16, lod0_count=2000),
}


@pytest.mark.parametrize("name", sorted(SETS))
def test_rows_only_preprocess_matches_full(name):
    verts = synth.make_tileset(**SETS[name])
    full, rows = _pair(verts)
    n_lod, n_tile = SETS[name]["n_lod"], SETS[name]["n_tile"]
    assert full.n_tiles == rows.n_tiles == (n_lod, n_tile, 9)
    for l in range(n_lod):
        for t in range(n_tile):
            assert full.rows(l, t).tobytes() == rows.rows(l, t).tobytes()
            assert full.merge_offset(l, t) == rows.merge_offset(l, t)
    for t in range(n_tile):
        for a, b in zip(full.tile_base(t), rows.tile_base(t)):
            assert a.tobytes() == b.tobytes()
    assert full.lod_avg_scale().tobytes() == rows.lod_avg_scale().tobytes()
    assert full.presort_view_proj().tobytes() == rows.presort_view_proj().tobytes()
    # the rows are what the full wang's texture / raw depths were made from
    tex, _, _ = full.preload()
    r0 = rows.rows(0, 0)
    assert host.generate_texture(r0).tobytes() == tex[:r0.shape[0]].tobytes()
    vp = rows.presort_view_proj()
    xyz = r0[:, :12].copy().view(np.float32)
    for v in range(9):
        d = ((vp[v, 2] * xyz[:, 0] + vp[v, 6] * xyz[:, 1]) + vp[v, 10] * xyz[:, 2]) * np.float32(4096.0)
        want = np.clip(np.trunc(d.astype(np.float64)), -2.0 ** 31, 2.0 ** 31 - 1).astype(np.int64)     # Rust's `as i32`
        assert np.array_equal(want, full.raw_depth(0, 0, v).astype(np.int64))
    full.close(); rows.close()


@pytest.mark.parametrize("kind", ["plain", "sphere", "heightmap", "one_lod"])
def test_rows_only_worker_output_matches_full(kind):
    # one_lod: every base list is its own LOD alone (no second segment), which the counts of build_tiles / sort_tiles follow
    sizes = {"plain": SETS["c3"], "one_lod": SETS["one_lod"]}.get(kind, dict(n_lod=3, n_tile=16, lod0_count=1200))
    verts = synth.make_tileset(**sizes)
    full, rows = _pair(verts)
    full.set_device_merge(True)
    user = _user(kind, sizes["n_tile"])
    cf, cr = full.configure(user), rows.configure(user)
    for name, _ in type(cf)._fields_:
        if name != "height_map":             # (a pointer into each wang)
            assert bytes(getattr(cf, name)) == bytes(getattr(cr, name)) if hasattr(getattr(cf, name), "_length_") else getattr(cf, name) == getattr(cr, name)
    if kind == "heightmap":
        assert full.height_map().tobytes() == rows.height_map().tobytes()
    ids = None
    n_groups = 0
    for pos, target in CAMERAS:
        _, vp = host.camera_uniforms(pos, target, (0, 0, 1), 45.0, 0.1, 2400.0, 1280, 720)
        sf, sr = full.build_tiles(pos), rows.build_tiles(pos)
        assert bytes(sf) == bytes(sr)
        if ids is None:
            ids = full.tile_ids()
            rows.set_tile_ids(ids)          # the tile ids come from the same seeded RNG; pinned anyway
            full.set_tile_ids(ids)
        a, b = full.sort_tiles(pos, vp), rows.sort_tiles(pos, vp)
        assert _draw_bytes(a) == _draw_bytes(b)
        assert a.merged_gs_index.size == 0 and b.merged_gs_index.size == 0
        n_groups += len(a.groups)
    if kind != "sphere":
        assert n_groups > 0                  # merged groups were described
    if kind == "one_lod":
        assert all(sf.lod_splat_count[l] == 0 for l in range(1, 16)) and sf.splat_count == sf.blending_splat_count > 0
    wf, wr = full.worker_config(), rows.worker_config()
    n = sizes["n_lod"] * sizes["n_tile"]
    cnt_f = np.ctypeslib.as_array(C.cast(wf.splat_count, C.POINTER(C.c_uint32)), shape=(n,))
    cnt_r = np.ctypeslib.as_array(C.cast(wr.splat_count, C.POINTER(C.c_uint32)), shape=(n,))
    assert np.array_equal(cnt_f, cnt_r)
    assert cnt_r[0] == full.rows(0, 0).shape[0]
    full.close(); rows.close()


def test_rows_only_refusals():
    rows = host.WangTile(host.TileSet.from_vertices(synth.make_tileset(n_lod=2, n_tile=16, lod0_count=200)), rows_only=True)
    lib, h = rows._lib, rows._h
    p = host.Preload()
    assert lib.gswt_wang_preload(h, C.byref(p)) == L.GSWT_ERR_STATE
    assert b"rows-only" in lib.gswt_host_last_error()
    ptrs, cnts, offs = C.c_void_p(), C.c_void_p(), C.c_void_p()
    assert lib.gswt_wang_raw_depth_tables(h, C.byref(ptrs), C.byref(cnts), C.byref(offs)) == L.GSWT_ERR_STATE
    assert b"rows-only" in lib.gswt_host_last_error()
    n = C.c_size_t(7)
    assert lib.gswt_wang_raw_depth(h, 0, 0, 0, C.byref(n)) is None and n.value == 0
    assert b"rows-only" in lib.gswt_host_last_error()
    # host-side merged lists: sort_tiles without device merge
    rows.configure(_user("plain", 16))
    pos = (2.0, 2.0, 14.0)
    _, vp = host.camera_uniforms(pos, (2.0, 6.0, 0.0), (0, 0, 1), 45.0, 0.1, 2400.0, 640, 480)
    rows.build_tiles(pos)
    rows.sort_tiles(pos, vp)                  # device merge is on from the start
    rows.set_device_merge(False)
    with pytest.raises(host.GSWTHostError) as e:
        rows.sort_tiles(pos, vp)
    assert e.value.code == L.GSWT_ERR_STATE
    assert "device merge" in str(e.value)
    out = (C.c_float * 16)()
    assert lib.gswt_wang_presort_view_proj(h, out, 16) == L.GSWT_ERR_CAPACITY
    # the Python helpers that need host lists raise the same status with one message
    for call in (rows.preload, lambda: rows.raw_depth(0, 0, 0), lambda: rows.upload_raw_depth_to(None)):
        with pytest.raises(host.GSWTHostError) as e:
            call()
        assert e.value.code == L.GSWT_ERR_STATE and "rows-only" in str(e.value)
    rows.close()


def test_rows_only_new_refusals():
    # the same preprocess checks as gswt_wang_new: an empty tile scene, and the LOD-scale assertion
    lib = host.load()
    verts = synth.make_tileset(n_lod=2, n_tile=16, lod0_count=200)
    verts[1] = [v.copy() for v in verts[0]]          # LOD 1 no coarser than LOD 0
    h = C.c_void_p()
    ts = host.TileSet.from_vertices(verts)
    th, ts._h = ts._h, None
    assert lib.gswt_wang_new_rows(th, C.byref(h)) == L.GSWT_ERR_BAD_ARG
    assert b"avg_scale" in lib.gswt_host_last_error()
    assert lib.gswt_wang_new_rows(None, C.byref(h)) == L.GSWT_ERR_BAD_ARG
