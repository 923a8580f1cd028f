"""The device sort event (gswt_worker_*) at the map sizes where its code paths change, byte for byte against libgswt_host's
gswt_wang_sort_tiles: BASELINE c5's 129x129 map, the reference's default 97x97 map, both sides of k_w_merge's 48 KB dynamic-LDS
line and of its LDS limit, both sides of the graph tables' LDS / global-memory switch, the largest map gswt_worker_create accepts,
and the refusals one step past each limit.

Every boundary shape below is derived here from the sizes the kernels' tables take, written out again rather than imported:
  k_w_merge       (3 * cells + 3 * (cells // 2 + 1)) * 2 bytes of dynamic LDS; above 48 KB the worker raises the kernel's limit,
                  above 156 KB Edge merging is refused
  k_w_order_seq   52 * cells + 64 bytes of graph tables; in LDS up to 140 KB, in global memory beyond
  u16 ids         edge ids run up to 2 * cells - 1 and 0xFFFF is the empty link: at most 32 767 cells
The map of half size (hw, hh) is (2 hw + 1) x (2 hh + 1) cells."""
import ctypes as C
import time

import numpy as np
import pytest

from tests.test_worker_gpu import _cam, _compare, _pipe

pytestmark = pytest.mark.gpu

KB = 1024


def merge_lds(cells):
    return (3 * cells + 3 * (cells // 2 + 1)) * 2


def graph_bytes(cells):
    return 52 * cells + 64


MERGE_LDS_DEFAULT = 48 * KB          # what a kernel may use without hipFuncSetAttribute
MERGE_LDS_MAX = 156 * KB
GRAPH_LDS_MAX = 140 * KB
MAX_CELLS = 32767                     # 2 * cells - 1 < 0xFFFF


def _half(w, h):
    assert w % 2 == 1 and h % 2 == 1
    return ((w - 1) // 2, (h - 1) // 2)


def _graph_user(**kw):
    from gswt_renderer_amd import host
    u = dict(surface_type=host.SURFACE_NONE, tile_sort_type=host.SORT_GRAPH, merge_type=host.MERGE_EDGE, lod_blending=True,
             lod_transition_width_ratio=0.05, merge_topk=100, merge_dot_threshold=0.2)
    u.update(kw)
    return u


def _event_ms(dw, pos, vp, reps=3):
    """Median wall time of a whole device sort event (sort_tiles + fetch of its records), after the one _compare ran."""
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        dw.sort_tiles(pos, vp)
        dw.fetch()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def _cyclic_nodes(pipe, state, pos):
    """Nodes on a cycle of the Graph order's DiGraph (wangtile.rs:1128-1170) as built from the exported cells: the sort event must
    have taken nodes out with remove_node when this is nonzero.  (The orientation signs are recomputed in f32 here, so this only
    counts; the byte comparison is _compare's.)"""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    cells, n, _ = pipe.wang.export_cells()
    a = np.frombuffer(bytes(cells), dtype=np.float32).reshape(n, C.sizeof(cells) // (4 * n))
    mw, mh = pipe.wang.conf.tile_map_wh
    idx = np.arange(n)
    x, y = idx // mh, idx % mh
    node = np.where(state[:, 3] == 2, state[:, 4], idx)
    epos, enor = a[:, 41:53].reshape(n, 4, 3), a[:, 53:65].reshape(n, 4, 3)
    cam = np.asarray(pos, np.float32)
    src, dst = [], []
    for s, (dx, dy) in ((0, (-1, 0)), (1, (0, 1)), (2, (1, 0)), (3, (0, -1))):
        nx, ny = x + dx, y + dy
        ok = (nx >= 0) & (nx < mw) & (ny >= 0) & (ny < mh)
        nb = np.where(ok, nx * mh + ny, 0)
        ok &= nb > idx
        dr = ((epos[:, s] - cam) * enor[:, s]).sum(axis=1, dtype=np.float32)
        a_, b_ = node[idx], node[nb]
        ok &= (a_ != b_) & (dr != 0)
        src.append(np.where(dr > 0, a_, b_)[ok])
        dst.append(np.where(dr > 0, b_, a_)[ok])
    src, dst = np.concatenate(src), np.concatenate(dst)
    g = coo_matrix((np.ones(len(src)), (src, dst)), shape=(n, n)).tocsr()
    _, lab = connected_components(g, directed=True, connection="strong")
    size = np.bincount(lab)
    return int((size[lab] > 1).sum())


def _run(half, user, cams, lod0=24, height_tex=None, seed=3, tag=""):
    """One pipeline and device worker; _compare at every camera (rebuild where asked).  -> (pipe, dw, last ref)"""
    from gswt_renderer_amd.worker import DeviceWorker
    pipe, _ = _pipe(half, user, lod0=lod0, height_tex=height_tex, seed=seed)
    dw = DeviceWorker(pipe.renderer, pipe.wang)
    ref = None
    for k, (pos, tgt, rebuild) in enumerate(cams):
        cu, vp = _cam(pos, tgt)
        ref = _compare(pipe, dw, pos, vp, rebuild=rebuild, tag=f"{tag} cam {k}")
        assert ref["n"][0] > 0, tag
    return pipe, dw, ref


def test_boundary_shapes_follow_from_the_table_sizes():
    """The shapes used below sit where this file says they do (no GPU work)."""
    assert merge_lds(43 * 127) == MERGE_LDS_DEFAULT                        # 5 461 cells: exactly 48 KB
    assert merge_lds(71 * 77) > MERGE_LDS_DEFAULT                          # 5 467: the first odd-by-odd map above it
    assert all(merge_lds(w * h) <= MERGE_LDS_DEFAULT for w in range(1, 200, 2) for h in range(1, 200, 2) if w * h < 5467)
    assert merge_lds(97 * 97) == 84684 and merge_lds(129 * 129) == 149772
    assert merge_lds(133 * 133) == 159204 <= MERGE_LDS_MAX < merge_lds(133 * 135)
    assert max(c for c in range(20000) if merge_lds(c) <= MERGE_LDS_MAX) == 17749
    assert graph_bytes(19 * 145) <= GRAPH_LDS_MAX < graph_bytes(31 * 89)  # 2 755 / 2 759 cells
    assert max(c for c in range(5000) if graph_bytes(c) <= GRAPH_LDS_MAX) == 2755
    assert 151 * 217 == MAX_CELLS and 2 * MAX_CELLS - 1 < 0xFFFF <= 2 * (MAX_CELLS + 1) - 1
    assert 3 * 10923 == MAX_CELLS + 2                                      # the smallest odd-by-odd map above the limit
    assert merge_lds(121 * 49) > MERGE_LDS_DEFAULT                         # the Sphere map of k = 12


def test_c5_map_sort_event_and_swapped_in_frame_match_host():
    """BASELINE c5's map and worker settings (129x129, Graph order, Edge merge, merge_topk 100, LOD blending): k_w_merge runs with
    146 KB of dynamic LDS.  Three cameras, the first and last with a rebuild; then the device event is swapped in and its frame equals
    the frame of the host's event bit for bit."""
    from gswt_renderer_amd import host, workloads
    w = workloads.WORKLOADS["c5"]
    assert w["half"] == (64, 64) and merge_lds(129 * 129) > MERGE_LDS_DEFAULT
    cam0 = workloads.camera_for("c5")
    cams = [(cam0["pos"], cam0["target"], True), ((30.0, -20.0, 12.0), (60.0, 40.0, 0.0), False),
            ((-90.0, 75.0, 25.0), (0.0, 0.0, 0.0), True)]
    pipe, dw, ref = _run(w["half"], dict(w["user"]), cams, tag="c5")
    assert ref["n"][0] > 10000 and ref["n"][1] > 0, ref["n"]
    pos, tgt, _ = cams[-1]
    ms = _event_ms(dw, pos, _cam(pos, tgt)[1])
    print(f"c5 129x129: device sort event {ms:.2f} ms, {ref['n']} (tiles, groups, members, merged)")
    W, H = 480, 272
    cu, vp = host.camera_uniforms(pos, tgt, (0, 0, 1), 45.0, 0.1, 2400.0, W, H)
    ref = _compare(pipe, dw, pos, vp, rebuild=False, tag="c5 frame")
    pipe.update(pos, vp, force_sort=True)
    img_host = pipe.render(cu, W, H)
    dw.swap_in()
    img_dev = pipe.render(cu, W, H)
    assert float(np.abs(img_host).max()) > 0
    assert np.array_equal(img_host.view(np.uint32), img_dev.view(np.uint32))
    dw.close()


@pytest.mark.parametrize("surface", ["flat", "heightmap", "steep"])
def test_reference_default_map(surface):
    """The reference's default 97x97 map (host.user_data's tile_map_half_wh = (48, 48)): 83 KB of merge tables.  The steep
    HeightMap makes the Graph order's edge orientations cyclic, so remove_node renumbers node ids in the thousands."""
    from gswt_renderer_amd import host
    extra = {"flat": dict(surface_type=host.SURFACE_NONE),
             "heightmap": dict(surface_type=host.SURFACE_HEIGHTMAP, height_map_wh=(10, 10), height_map_scale=(1.0, 1.0, 1.0)),
             "steep": dict(surface_type=host.SURFACE_HEIGHTMAP, height_map_wh=(24, 24), height_map_scale=(1.0, 1.0, 6.0))}[surface]
    assert host.user_data().tile_map_half_wh[:] == [48, 48]
    cams = [((3.0, -2.0, 10.0), (40.0, 60.0, 0.0), True), ((-70.0, 35.0, 18.0), (0.0, 0.0, 0.0), True),
            ((-68.0, 36.0, 18.0), (10.0, -30.0, 2.0), False)]
    pipe, dw, ref = _run((48, 48), _graph_user(lod_max_dist=384.0, **extra), cams, tag=f"97x97 {surface}")
    pos, tgt, _ = cams[-1]
    cyc = _cyclic_nodes(pipe, ref["state"], pos)
    ms = _event_ms(dw, pos, _cam(pos, tgt)[1])
    print(f"97x97 {surface}: device sort event {ms:.2f} ms, {ref['n']}, {cyc} nodes on cycles")
    if surface == "steep":
        assert cyc > 0
    dw.close()


@pytest.mark.parametrize("wh", [(43, 127), (71, 77)], ids=["5461-cells-48KB", "5467-cells"])
def test_edge_merge_at_the_48kb_line(wh):
    """43x127 needs exactly 48 KB (no attribute call); 71x77 is the first odd-by-odd map that needs hipFuncSetAttribute."""
    cells = wh[0] * wh[1]
    assert (merge_lds(cells) > MERGE_LDS_DEFAULT) == (cells > 5461)
    cams = [((5.0, -3.0, 9.0), (40.0, 80.0, 0.0), True), ((-60.0, 150.0, 14.0), (0.0, 0.0, 0.0), True)]
    _, dw, ref = _run(_half(*wh), _graph_user(lod_max_dist=300.0, merge_topk=400), cams, tag=f"{wh}")
    assert ref["n"][1] > 0
    dw.close()


@pytest.mark.parametrize("sort_type", [3, 2], ids=["graph", "object"])
def test_largest_edge_merge_map(sort_type):
    """133x133 = 17 689 cells, 159 204 B of merge tables: the largest square map with Edge merging, in the Graph and Object orders."""
    cams = [((2.0, -1.0, 12.0), (60.0, 90.0, 0.0), True), ((-200.0, 180.0, 30.0), (0.0, 0.0, 0.0), True)]
    _, dw, ref = _run((66, 66), _graph_user(tile_sort_type=sort_type, lod_max_dist=600.0, merge_topk=2000), cams,
                      tag=f"133x133 sort {sort_type}")
    assert ref["n"][1] > 100
    pos, tgt, _ = cams[-1]
    print(f"133x133 sort {sort_type}: device sort event {_event_ms(dw, pos, _cam(pos, tgt)[1]):.2f} ms, {ref['n']}")
    dw.close()


def test_edge_merge_on_a_large_sphere():
    """A Sphere map above 5 461 cells (half (5k, 2k) with k = 12: 121x49), whose neighbours come from the host's table."""
    from gswt_renderer_amd import host
    k = 12
    r = 6.0 * k
    cams = [((1.8 * r, 0.3 * r, 0.5 * r), (0.0, 0.0, 0.0), True), ((-0.4 * r, 1.5 * r, -1.1 * r), (0.0, 0.0, 0.0), False),
            ((0.2 * r, -0.3 * r, 1.9 * r), (0.0, 0.0, 0.0), False)]
    _, dw, ref = _run((5 * k, 2 * k), _graph_user(surface_type=host.SURFACE_SPHERE, sphere_radius=r, lod_max_dist=4.0 * r,
                                                 merge_topk=300, merge_dot_threshold=0.5), cams, tag="sphere k=12")
    dw.close()


@pytest.mark.parametrize("wh", [(19, 145), (31, 89)], ids=["2755-cells-lds", "2759-cells-global"])
def test_graph_tables_at_the_lds_switch(wh):
    """19x145 = 2 755 cells keeps the graph tables in LDS (143 324 B); 31x89 = 2 759 is the first odd-by-odd map in global memory."""
    cells = wh[0] * wh[1]
    assert (graph_bytes(cells) <= GRAPH_LDS_MAX) == (cells <= 2755)
    from gswt_renderer_amd import host
    for surface, extra in ((host.SURFACE_NONE, {}), (host.SURFACE_HEIGHTMAP, dict(height_map_wh=(12, 12), height_map_scale=(1.0, 1.0, 4.0)))):
        cams = [((4.0, -6.0, 8.0), (30.0, 60.0, 0.0), True), ((-30.0, 100.0, 12.0), (0.0, 0.0, 0.0), True)]
        _, dw, _ = _run(_half(*wh), _graph_user(surface_type=surface, lod_max_dist=200.0, **extra), cams, tag=f"{wh} surface {surface}")
        dw.close()


@pytest.mark.parametrize("wh", [(151, 217), (181, 181)], ids=["32767-cells", "32761-cells"])
@pytest.mark.parametrize("merge", ["axis", "none"])
def test_largest_maps(wh, merge):
    """The cell limit itself (151x217 = 32 767 cells: edge ids up to 65 165, node ids up to 32 766, all below the 0xFFFF link) and
    181x181, in the Graph order with Axis merging and with none.  (Another order needs Edge merging for its corner data -- the
    reference panics without it, renderer.rs:476 -- and Edge merging stops at 17 749 cells: see test_largest_edge_merge_map.)"""
    from gswt_renderer_amd import host
    mt = host.MERGE_AXIS if merge == "axis" else host.MERGE_NONE
    cams = [((3.0, -2.0, 10.0), (100.0, 200.0, 0.0), True), ((-250.0, 300.0, 40.0), (0.0, 0.0, 0.0), True)]
    _, dw, ref = _run(_half(*wh), _graph_user(merge_type=mt, lod_max_dist=800.0), cams, tag=f"{wh} merge {merge}")
    assert ref["n"][0] > 30000, ref["n"]
    pos, tgt, _ = cams[-1]
    print(f"{wh[0]}x{wh[1]} merge {merge}: device sort event {_event_ms(dw, pos, _cam(pos, tgt)[1]):.2f} ms, {ref['n']}")
    dw.close()


def _create_rc(pipe):
    from gswt_renderer_amd import _lib as L
    lib = L.load()
    cfg = pipe.wang.worker_config()
    h = C.c_void_p()
    rc = lib.gswt_worker_create(pipe.renderer._h, C.byref(cfg), C.byref(h))
    if h.value:
        lib.gswt_worker_destroy(h)
    return rc, cfg.map_w * cfg.map_h


@pytest.mark.parametrize("case", ["edge-merge", "cells"])
def test_one_step_past_each_limit_is_refused(case):
    """133x135 with Edge merging (161 598 B of merge tables) and 3x10923 = 32 769 cells (the smallest odd-by-odd map above
    32 767) return GSWT_ERR_CAPACITY; then a worker on the same ctx, reconfigured within the limits, still matches the host."""
    from gswt_renderer_amd import _lib as L
    from gswt_renderer_amd import host
    from gswt_renderer_amd.worker import DeviceWorker
    if case == "edge-merge":
        half, user, ok_user = (66, 67), _graph_user(lod_max_dist=600.0), _graph_user(lod_max_dist=600.0, merge_type=host.MERGE_NONE)
        assert merge_lds(133 * 135) > MERGE_LDS_MAX
    else:
        half, user = (1, 5461), _graph_user(merge_type=host.MERGE_NONE, lod_max_dist=600.0)
        ok_user = dict(user, tile_map_half_wh=(1, 5460))
    pipe, _ = _pipe(half, user, lod0=24)
    rc, cells = _create_rc(pipe)
    assert rc == L.GSWT_ERR_CAPACITY, (case, cells, rc)
    with pytest.raises(RuntimeError, match="gswt_worker_create"):
        DeviceWorker(pipe.renderer, pipe.wang)
    pipe.configure(host.user_data(**({"tile_map_half_wh": half} | ok_user)))
    rc, cells = _create_rc(pipe)
    assert rc == L.GSWT_OK and cells <= MAX_CELLS
    dw = DeviceWorker(pipe.renderer, pipe.wang)
    for k, (pos, tgt) in enumerate([((1.0, -3.0, 8.0), (4.0, 60.0, 0.0)), ((2.0, 2000.0, 15.0), (0.0, 1900.0, 0.0))]):
        cu, vp = _cam(pos, tgt)
        ref = _compare(pipe, dw, pos, vp, rebuild=True, tag=f"{case} after refusal cam {k}")
        assert ref["n"][0] > 0
    dw.close()
