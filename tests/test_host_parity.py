"""Host logic (libgswt_host.so: Scene loader, WangTile worker, draw-list builder) against the
Python oracle restatement, bit-exact (integer / index work and f32 with identical operand order).
CPU only."""
import io

import numpy as np
import pytest

from gswt_renderer_amd import host, synth
from oracle import gswt_oracle as orc
from oracle import wangtile_oracle as wo


@pytest.fixture(scope="module")
def tiles():
    verts = synth.make_tileset(n_lod=3, n_tile=16, lod0_count=300)
    rows_o = [[orc.scene_load(v) for v in lod] for lod in verts]
    pp = orc.preprocess(rows_o)
    return verts, rows_o, pp


def test_scene_load_rows_bit_exact(tiles):
    verts, rows_o, _ = tiles
    ts = host.TileSet.from_vertices(verts)
    for l in range(3):
        for t in range(16):
            assert np.array_equal(ts.rows(l, t), rows_o[l][t])


def test_ply_and_zip_loader(tiles, tmp_path):
    verts, rows_o, _ = tiles
    zbytes = synth.tile_zip_bytes(verts)
    p = tmp_path / "tiles.zip"
    p.write_bytes(zbytes)
    for src in (zbytes, str(p)):
        ts = host.TileSet.from_zip(src)
        assert ts.dims() == (3, 16)
        for l in range(3):
            for t in range(16):
                assert np.array_equal(ts.rows(l, t), rows_o[l][t])
    # oracle's own zip loader agrees
    orows = orc.load_scene_zip(str(p))
    assert all(np.array_equal(orows[l][t], rows_o[l][t]) for l in range(3) for t in range(16))


def test_ply_header_errors():
    ts = host.TileSet.from_vertices([[np.zeros((1, 62), np.float32)]])
    lib = host.load()
    bad = b"ply\nformat binary_little_endian 1.0\nelement vertex 2\nend_header \n" + b"\0" * 600
    buf = np.frombuffer(bad, dtype=np.uint8)
    assert lib.gswt_tileset_set_ply(ts._h, 0, 0, buf.ctypes.data, len(bad)) == -5     # never sees "end_header\n"
    short = synth.write_ply(np.zeros((2, 62), np.float32))[:-10]                        # read_exact fails
    buf = np.frombuffer(short, dtype=np.uint8)
    assert lib.gswt_tileset_set_ply(ts._h, 0, 0, buf.ctypes.data, len(short)) == -5
    with pytest.raises(ValueError):
        orc.parse_ply(bad)


def test_ply_body_at_any_alignment():
    """scene.rs:72-212 reads the body with read_exact from wherever `end_header\n` ends: the loader must not care how the header's length
    or the caller's buffer aligns the floats (tools/host_sanitizers.sh runs this under UBSan)."""
    rng = np.random.default_rng(5)
    v = rng.normal(size=(7, 62)).astype(np.float32)
    want = orc.scene_load(v)
    lib = host.load()
    ts = host.TileSet.from_vertices([[np.zeros((1, 62), np.float32)]])
    for pad in range(4):
        for shift in range(2):
            ply = b"\0" * shift + b"ply\nformat binary_little_endian 1.0\ncomment " + b"x" * pad + b"\nelement vertex 7\nend_header\n" + v.tobytes()
            buf = np.frombuffer(ply, dtype=np.uint8)[shift:]
            assert lib.gswt_tileset_set_ply(ts._h, 0, 0, buf.ctypes.data, buf.shape[0]) == 0
            assert np.array_equal(ts.rows(0, 0), want)


def test_texture_halves_and_counting_sort(tiles):
    _, rows_o, _ = tiles
    rows = np.concatenate([rows_o[0][0], rows_o[2][5]])
    assert np.array_equal(host.generate_texture(rows), orc.generate_texture(rows))
    rng = np.random.default_rng(1)
    for x, y in rng.normal(0, 100, size=(200, 2)).astype(np.float32):
        assert host.pack_half_2x16(float(x), float(y)) == orc.pack_half_2x16(float(x), float(y))
    for vals in ([1e-8, 65504.0], [70000.0, -70000.0], [float("inf"), float("nan")], [6e-5, 5.9e-8]):
        assert host.pack_half_2x16(*vals) == orc.pack_half_2x16(*vals)
    for d in (rng.integers(-50000, 50000, size=5000), np.full(17, 3), np.array([2]), rng.integers(0, 3, size=1000)):
        d = d.astype(np.int32)
        seg, idx = orc.sort_raw_depth_vec([d])
        assert np.array_equal(host.sort_raw_depth(d), idx.astype(np.uint32))


def test_preprocess_bit_exact(tiles):
    verts, _, pp = tiles
    w = host.WangTile(host.TileSet.from_vertices(verts))
    tex, gi, li = w.preload()
    assert np.array_equal(tex, pp.tex)
    assert np.array_equal(w.lod_avg_scale(), pp.lod_avg_scale)
    for t in range(16):
        c, a = w.tile_base(t)
        assert np.array_equal(c, pp.tile_center[t]) and np.array_equal(a, pp.aabb[t])
    for l in range(3):
        for t in range(16):
            assert w.merge_offset(l, t) == pp.merge_offset[l, t]
            for v in range(9):
                assert np.array_equal(w.raw_depth(l, t, v), pp.raw_depth[l][t][v])
                assert np.array_equal(gi[l][t][v], pp.gs_index[l][t][v])
                assert np.array_equal(li[l][t][v], pp.gs_lod_id[l][t][v])


def _far_cams(scale):
    """Cameras |x|, |y| ~ scale from the origin (the reference recentres its map on the camera, wangtile.rs:1684, so after a long
    flight every position is this far out), mixed signs; each second camera steps into the next tile so the map recentres."""
    cams = []
    for sx, sy in ((1, -1), (-1, 1), (-1, -1)):
        x, y = sx * scale + 0.37e-3 * scale, sy * scale - 0.61e-3 * scale
        cams += [((x, y, 3.0), (x + 1.0, y + 2.0, 2.5)), ((x + 4.3, y - 0.2, 3.0), (x + 5.0, y + 1.5, 2.5))]
    return cams


FAR_SCALES = [1e3, 1e4, 1e5]


def test_camera_uniforms_bit_exact():
    far = [(p, t, 640, 480) for s in FAR_SCALES for p, t in _far_cams(s)] + [(p, t, 333, 777) for p, t in _far_cams(1e5)]
    for (pos, tgt, W, H) in [((0, 0, 5), (0, 1, 5), 640, 480), ((4.2, 1.0, 3.0), (5.0, 3.0, 2.5), 1920, 1080),
                             ((-3.3, 7.1, 0.4), (-2.0, -5.0, 1.0), 333, 777)] + far:
        cu, vp = host.camera_uniforms(pos, tgt, (0, 0, 1), 45.0, 0.1, 2400.0, W, H)
        oc = orc.Camera(W, H, pos, tgt, [0, 0, 1])
        assert bytes(cu) == bytes(oc.uniforms())
        assert np.array_equal(vp, oc.view_proj())


def _status_code(st):
    if st[0] == "none":
        return host.TR_NONE
    if st[0] == "spawning":
        return host.TR_SPAWNING
    return host.TR_CHANGING_LOWER if st[1] else host.TR_CHANGING_HIGHER


CONFIGS = [
    dict(tile_map_half_wh=(3, 3), surface_type=0, lod_max_dist=20.0, tile_sort_type=3, merge_type=2),
    dict(tile_map_half_wh=(3, 4), surface_type=1, lod_max_dist=24.0, tile_sort_type=3, merge_type=2, height_map_wh=(4, 4)),
    dict(tile_map_half_wh=(2, 2), surface_type=0, lod_max_dist=16.0, tile_sort_type=0, merge_type=2, lod_blending=False),
    dict(tile_map_half_wh=(3, 3), surface_type=1, lod_max_dist=20.0, tile_sort_type=3, merge_type=1, merge_tile_dist=(1, 3),
         height_map_type=4, height_map_wh=(8, 8)),
    dict(tile_map_half_wh=(3, 3), surface_type=1, lod_max_dist=20.0, tile_sort_type=1, merge_type=2, height_map_type=2,
         height_map_wh=(8, 8)),
    dict(tile_map_half_wh=(3, 3), surface_type=0, lod_max_dist=20.0, tile_sort_type=2, merge_type=2, use_cache=False),
    dict(tile_map_half_wh=(2, 3), surface_type=0, lod_max_dist=18.0, tile_sort_type=3, merge_type=0, lod_bbox_check=False,
         lod_dist_tolerance=0.5),
]
CAMS = [((0, 0, 5), (0, 1, 5)), ((0.5, 0.3, 5), (1, 1, 4.5)), ((4.2, 1.0, 3), (5, 3, 2.5)), ((4.2, 1.0, 3), (3, -3, 2.0)),
        ((-7.9, -4.1, 2), (-9, -9, 1.5))]


SPHERE_CONFIGS = [
    dict(tile_map_half_wh=(5, 2), surface_type=2, sphere_radius=6.5, lod_max_dist=5.0, tile_sort_type=3, merge_type=2),
    dict(tile_map_half_wh=(5, 2), surface_type=2, sphere_radius=5.0, lod_max_dist=4.0, tile_sort_type=3, merge_type=1, merge_tile_dist=(0, 2)),
    dict(tile_map_half_wh=(10, 4), surface_type=2, sphere_radius=13.0, lod_max_dist=6.0, tile_sort_type=2, merge_type=2,
         lod_bbox_check=False),
]
SPHERE_CAMS = [((3.0, -19.0, 6.0), (0, 0, 0)), ((3.5, -18.0, 6.0), (0, 0, 0.5)), ((-14.0, 9.0, -8.0), (0, 0, 1)), ((0.5, 0.5, 21.0), (0, 0.1, 0))]


@pytest.mark.parametrize("cfg", SPHERE_CONFIGS)
def test_wangtile_worker_sphere_bit_exact(tiles, cfg):
    """Sphere topology (5 x 2 icosahedral-strip blocks, wrapped neighbour slots), the CPU sphere mapping through the
    canonical sin / cos, the static map (never shifts) and the nearest-tile merge centre."""
    _check_worker(tiles, cfg, SPHERE_CAMS)


def test_sphere_neighbours_are_mutual(tiles):
    """Every neighbour link of the sphere topology points back: nb(a, slot) = (b, s) implies nb(b, s) = (a, slot)
    (this is what makes Wang edge colours well defined across block seams)."""
    verts, _, pp = tiles
    ow = wo.WangTile(pp)
    ow.configure(wo.UserData(tile_map_half_wh=(10, 4), surface_type=2, sphere_radius=13.0, lod_max_dist=6.0))
    w, h = ow.user.tile_map_wh
    assert (w, h) == (20, 8)
    for x in range(w):
        for y in range(h):
            for slot, nb in enumerate(ow.neighbor_map[x][y]):
                assert nb is not None
                (bx, by), s = nb
                back = ow.neighbor_map[bx][by][s]
                assert back is not None and back[0] == (x, y) and back[1] == slot, (x, y, slot, nb, back)


@pytest.mark.parametrize("cfg", CONFIGS)
def test_wangtile_worker_bit_exact(tiles, cfg):
    _check_worker(tiles, cfg, CAMS)


@pytest.mark.parametrize("scale", FAR_SCALES)
@pytest.mark.parametrize("cfg", CONFIGS[:2] + CONFIGS[3:4], ids=["flat", "heightmap", "heightmap-merge-dist"])
def test_wangtile_worker_far_from_origin_bit_exact(tiles, cfg, scale):
    """Flat and HeightMap maps recentred 1e3..1e5 from the origin (pos_to_coord / coord_to_pos and every tile offset out there)."""
    centres = _check_worker(tiles, cfg, _far_cams(scale))
    assert len(set(centres)) == 6 and min(abs(c) for cc in centres for c in cc) >= 0.9 * scale / 4.0, centres


@pytest.mark.parametrize("cfg", SPHERE_CONFIGS[:2])
def test_wangtile_worker_sphere_far_cameras_bit_exact(tiles, cfg):
    """The Sphere map never shifts; cameras 1e3 world units out (inside the 2400 far plane) still see it."""
    _check_worker(tiles, cfg, [((1e3, -2e3, 500.0), (0, 0, 0)), ((-1.9e3, 1.1e3, -700.0), (0, 0, 1.0)), ((3.0, -19.0, 6.0), (0, 0, 0))])


def _check_worker(tiles, cfg, cams):
    verts, _, pp = tiles
    w = host.WangTile(host.TileSet.from_vertices(verts))
    conf = w.configure(host.user_data(**cfg))
    ow = wo.WangTile(pp)
    ou = ow.configure(wo.UserData(**cfg))
    assert tuple(conf.tile_map_wh) == tuple(ou.tile_map_wh)
    assert np.array_equal(np.array(conf.lod_transition_dist[:3], dtype=np.float32), np.array(ou.lod_transition_dist, dtype=np.float32))
    if cfg["surface_type"] == 1:
        assert np.array_equal(w.height_map().ravel(), ou.height_map)
    centres = []
    with np.errstate(all="ignore"):
        for pos, tgt in cams:
            cu, vp = host.camera_uniforms(pos, tgt, (0, 0, 1), 45.0, 0.1, 2400.0, 320, 240)
            upd = w.check_update(pos)
            assert upd == bool(ow.check_update(pos))
            if upd:
                sd, osd = w.build_tiles(pos), ow.build_tiles(pos)
                oids = [ow.tile_map[i][j].tid[1] for i in range(ou.tile_map_wh[0]) for j in range(ou.tile_map_wh[1])]
                assert w.tile_ids().tolist() == oids
                assert tuple(sd.center_coord) == tuple(osd["center_coord"])
                centres.append(tuple(sd.center_coord))
                assert (sd.splat_count, sd.blending_splat_count) == (osd["splat_count"], osd["blending_splat_count"])
                assert list(sd.lod_instance_count[:3]) == osd["lod_instance_count"]
            s, os_ = w.sort_tiles(pos, vp), ow.sort_tiles(pos, vp)
            assert [t.map_index for t in s.tiles] == [t.map_index for t in os_["tile_instance_vec"]]
            for tc, to, (key, val) in zip(s.tiles, os_["tile_instance_vec"], os_["render_data_vec"]):
                assert (tc.lod, tc.tile, tc.view_id) == (to.tid[0], to.tid[1], to.view_id)
                assert tc.transition == _status_code(to.transition_status)
                assert np.array_equal(np.array(tc.tile_center[:], dtype=np.float32), to.tile_center)
                assert np.array_equal(np.array(tc.tile_offset[:], dtype=np.float32), to.tile_offset)
                assert tc.key_len == len(key[1])
                if to.corner_data is not None:
                    assert np.array_equal(np.array(tc.corners[:], dtype=np.float32).reshape(4, 3), np.stack([c[0] for c in to.corner_data]))
                assert bool(tc.merged) == (val is not None)
                if val is not None:
                    n, a = val["splat_count"], tc.merged_offset
                    assert tc.merged_count == n and tc.single_lod_id == val["single_lod_id"]
                    assert np.array_equal(s.merged_gs_index[a:a + n], val["gs_index"])
                    assert np.array_equal(s.merged_map_id[a:a + n], val["gs_map_id"])
                    if val["gs_lod_id"] is not None:
                        assert np.array_equal(s.merged_lod_id[a:a + n], val["gs_lod_id"])
            # draw list (TileUniforms::from_tile + list selection) vs the oracle's render-loop restatement
            odraws_all = {id(t): None for t in os_["tile_instance_vec"]}
            for d, to, (key, val) in zip(s.draws, os_["tile_instance_vec"], os_["render_data_vec"]):
                otu = wo.tile_uniforms_from_tile(to, val)
                assert bytes(d.tile) == bytes(otu)
                if val is None:
                    bl = to.tid[0] - 1 if to.transition_status == ("changing", False) else to.tid[0]
                    assert (d.merged, d.base_lod, d.base_tile, d.base_view) == (0, bl, to.tid[1], to.view_id)
                    assert d.cull_enable == 1
                else:
                    assert d.merged == 1 and d.merged_has_lod == (1 if val["single_lod_id"] == -1 else 0)
            osu = wo.scene_uniforms_from_data(ou, ow.center_coord)
            assert bytes(w.scene_uniforms()) == bytes(osu)
    return centres


def test_wang_constraints_and_graph_order_properties(tiles):
    """Independent of the unpinned RNG / toposort restatements: edge colours of adjacent tiles match
    (wangtile.rs:1737-1753) and the Graph order respects every visibility edge of the DAG."""
    verts, _, pp = tiles
    w = host.WangTile(host.TileSet.from_vertices(verts))
    cfg = dict(tile_map_half_wh=(5, 4), surface_type=0, lod_max_dist=30.0, tile_sort_type=3, merge_type=0)
    w.configure(host.user_data(**cfg))
    pos = (1.0, 2.0, 4.0)
    cu, vp = host.camera_uniforms(pos, (3, 9, 2), (0, 0, 1), 45.0, 0.1, 2400.0, 320, 240)
    w.build_tiles(pos)
    ids = w.tile_ids().reshape(11, 9)
    col = wo.WangTile.tile_id_to_color
    for x in range(11):
        for y in range(9):
            if x + 1 < 11:
                assert col(ids[x, y])[2] == col(ids[x + 1, y])[0]     # my East == neighbour's West
            if y + 1 < 9:
                assert col(ids[x, y])[1] == col(ids[x, y + 1])[3]     # my North == neighbour's South
    s = w.sort_tiles(pos, vp)
    rank = {t.map_index: i for i, t in enumerate(s.tiles)}
    ow = wo.WangTile(pp)
    ow.configure(wo.UserData(**cfg))
    ow.build_tiles(pos)
    cam = np.array(pos, dtype=np.float32)
    checked = 0
    for x in range(11):
        for y in range(9):
            ti = ow.tile_map[x][y]
            for n_i, nb in enumerate(ow.neighbor_map[x][y]):
                if nb is None:
                    continue
                a, b = ow.map_to_index((x, y)), ow.map_to_index(nb[0])
                if a not in rank or b not in rank:
                    continue
                epos, enorm = ti.edge_data[n_i]
                dr = wo.dot3(enorm, (epos - cam).astype(np.float32))
                if dr > 0:      # edge a -> b in the graph; final list is reversed => b is drawn before a
                    assert rank[b] < rank[a]
                    checked += 1
    assert checked > 50


def test_set_tile_ids_roundtrip(tiles):
    verts, _, _ = tiles
    w = host.WangTile(host.TileSet.from_vertices(verts))
    w.configure(host.user_data(tile_map_half_wh=(2, 2), surface_type=0, lod_max_dist=20.0))
    w.build_tiles((0, 0, 5))
    ids = (np.arange(25) * 5 % 16).astype(np.uint32)
    w.set_tile_ids(ids)
    assert w.tile_ids().tolist() == ids.tolist()
    with pytest.raises(host.GSWTHostError):
        w.set_tile_ids(np.full(25, 99, dtype=np.uint32))


def test_reference_panics_become_errors(tiles):
    verts, _, _ = tiles
    w = host.WangTile(host.TileSet.from_vertices(verts))
    with pytest.raises(host.GSWTHostError):      # assert!(n_tiles.1 / 16 >= center_option), wangtile.rs:366
        w.configure(host.user_data(center_option=2))
    w.configure(host.user_data(tile_map_half_wh=(1, 1), surface_type=0, lod_max_dist=20.0, tile_sort_type=0, merge_type=0))
    w.build_tiles((0, 0, 5))
    cu, vp = host.default_camera(64, 48)
    with pytest.raises(host.GSWTHostError):      # corner_data.unwrap() on None, renderer.rs:476
        w.sort_tiles((0, 0, 5), vp)
    bad = [[v.copy() for v in lod] for lod in verts]
    bad[1][0][:, 55:58] -= 5.0                    # LOD1 avg scale below LOD0: assert at wangtile.rs:138-140
    bad = [[bad[1][t] if l == 1 else verts[l][t] for t in range(16)] for l in range(3)]
    for t in range(16):
        bad[1][t] = bad[1][t].copy(); bad[1][t][:, 55:58] -= 5.0
    with pytest.raises(host.GSWTHostError):
        host.WangTile(host.TileSet.from_vertices(bad))


def test_loader_rejects_crafted_counts_without_unwinding():
    """a header count whose byte size wraps size_t, a 30-digit tile index and null rows must come back as
    status codes -- no over-read, no C++ exception through the C ABI."""
    import io
    import zipfile
    lib = host.load()
    ts = host.TileSet.from_vertices([[np.zeros((1, 62), np.float32)]])
    for count in (2 ** 62, 2 ** 64 - 1, 2 ** 70, 74381295208399815):       # 248 * n wraps to a small number for the last one
        ply = (f"ply\nformat binary_little_endian 1.0\nelement vertex {count}\nend_header\n").encode() + b"\0" * 1000
        buf = np.frombuffer(ply, dtype=np.uint8)
        assert lib.gswt_tileset_set_ply(ts._h, 0, 0, buf.ctypes.data, len(ply)) == -5
    assert lib.gswt_tileset_set_rows(ts._h, 0, 0, None, 5) == -1
    good = synth.write_ply(np.zeros((2, 62), np.float32))
    for name in ("lod0_tile_" + "9" * 30 + ".ply", "lod" + "7" * 25 + "_tile_0.ply", "lod0_tile_99999999.ply"):
        bio = io.BytesIO()
        with zipfile.ZipFile(bio, "w") as zf:
            zf.writestr(name, good)
        with pytest.raises(host.GSWTHostError):
            host.TileSet.from_zip(bio.getvalue())


def test_zero_vertex_ply_is_an_empty_scene():
    """`element vertex 0` is a legal header (scene.rs:72-212 reads zero rows): the loader returns an empty scene, touching no body bytes."""
    lib = host.load()
    ts = host.TileSet.from_vertices([[np.zeros((3, 62), np.float32)]])
    ply = b"ply\nformat binary_little_endian 1.0\nelement vertex 0\nend_header\n"
    buf = np.frombuffer(ply, dtype=np.uint8)
    assert lib.gswt_tileset_set_ply(ts._h, 0, 0, buf.ctypes.data, len(ply)) == 0
    assert ts.rows(0, 0).shape == (0, 32)
    assert orc.scene_load(np.zeros((0, 62), np.float32)).shape[0] == 0


def test_mutated_zips_return_a_status():
    """A bounded run of tools/fuzz_zip_loader.py's mutations (byte flips, truncation, central-directory damage, extreme 32-bit fields):
    every mutated tile zip either loads or raises GSWTHostError -- where the reference's loader panics (scene.rs:1030-1141)."""
    rng = np.random.default_rng(11)
    verts = [[rng.normal(size=(int(rng.integers(1, 6)), 62)).astype(np.float32) for _ in range(4)] for _ in range(2)]
    good = bytearray(synth.tile_zip_bytes(verts))
    seen = set()
    for it in range(300):
        b = bytearray(good)
        kind = it % 4
        if kind == 0:
            for _ in range(int(rng.integers(1, 8))):
                b[int(rng.integers(0, len(b)))] = int(rng.integers(0, 256))
        elif kind == 1:
            b = b[:int(rng.integers(0, len(b)))]
        elif kind == 2:
            for _ in range(int(rng.integers(1, 6))):
                b[len(b) - 1 - int(rng.integers(0, min(200, len(b))))] = int(rng.integers(0, 256))
        else:
            p = int(rng.integers(0, len(b) - 4))
            b[p:p + 4] = int(rng.choice([0, 1, 0x7FFFFFFF, 0xFFFFFFFF, 0xFFFFFFFE, len(b), len(b) + 1])).to_bytes(4, "little")
        try:
            ts = host.TileSet.from_zip(bytes(b))
            l, t = ts.dims()
            for i in range(l):
                for j in range(t):
                    assert ts.rows(i, j).shape[1] == 32
            seen.add("loaded")
        except host.GSWTHostError:
            seen.add("rejected")
    assert seen == {"loaded", "rejected"}
