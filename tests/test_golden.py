"""Committed golden vectors (tests/golden/*.npz, made by tests/golden/make_golden.py).
CPU: the oracle and the host library reproduce them from the stored inputs.
GPU: the HIP path matches the stored image (1e-4 L-inf) and per-splat outputs (bit-exact)."""
import glob
import json
import os

import numpy as np
import pytest

from gswt_renderer_amd import host
from oracle import gswt_oracle as orc
from oracle import wangtile_oracle as wo

GOLD = sorted(glob.glob(os.path.join(os.path.dirname(__file__), "golden", "case_*.npz")))
assert GOLD


def _load(path):
    g = np.load(path, allow_pickle=False)
    cfg = json.loads(str(g["config"]))
    for k, v in list(cfg.items()):
        if isinstance(v, list):
            cfg[k] = tuple(v)
    cfg["__rc"] = json.loads(str(g["render_config"])) if "render_config" in g.files else {}
    counts = g["row_counts"]
    rows, off = [], 0
    for l in range(counts.shape[0]):
        rows.append([])
        for t in range(counts.shape[1]):
            rows[l].append(np.ascontiguousarray(g["rows"][off: off + counts[l, t]]))
            off += counts[l, t]
    return g, cfg, rows


def _host_wang(rows, cfg, ids, pos):
    lib = host.load()
    import ctypes as C
    h = C.c_void_p()
    assert lib.gswt_tileset_create(len(rows), len(rows[0]), C.byref(h)) == 0
    for l, lod in enumerate(rows):
        for t, r in enumerate(lod):
            assert lib.gswt_tileset_set_rows(h, l, t, r.ctypes.data, r.shape[0]) == 0
    w = host.WangTile(host.TileSet(h))
    w.configure(host.user_data(**cfg))
    w.build_tiles(pos)
    w.set_tile_ids(ids)          # tile ids are explicit fixture inputs (RNG restatement is unpinned)
    return w


@pytest.mark.parametrize("path", GOLD, ids=[os.path.basename(p) for p in GOLD])
def test_oracle_reproduces_golden(path):
    g, cfg, rows = _load(path)
    rc = cfg.pop("__rc")
    W, H = [int(x) for x in g["size"]]
    pos, tgt = g["camera"][0], g["camera"][1]
    pp = orc.preprocess(rows)
    ow = wo.WangTile(pp)
    ou = ow.configure(wo.UserData(**cfg))
    cam = orc.Camera(W, H, pos, tgt, [0, 0, 1])
    with np.errstate(all="ignore"):
        osd = ow.build_tiles(pos)
        ids = [ow.tile_map[i][j].tid[1] for i in range(ou.tile_map_wh[0]) for j in range(ou.tile_map_wh[1])]
        assert ids == g["tile_ids"].tolist()
        osort = ow.sort_tiles(pos, cam.view_proj())
        draws = wo.renderer_draws(pp, osort, cam.view_proj())
    assert [t.map_index for t in osort["tile_instance_vec"]] == g["order"].tolist()
    assert [t.view_id for t in osort["tile_instance_vec"]] == g["views"].tolist()
    hm = ou.height_map.reshape(ou.height_map_wh[1], ou.height_map_wh[0]) if ou.surface_type == 1 else None
    su = wo.scene_uniforms_from_data(ou, osd["center_coord"], **rc)
    with orc.v2():           # the rounding sequence v2: arrays byte-identical to the round-2 / round-3 files
        img, st = orc.render(cam.uniforms(), su, pp.tex, draws, W, H, height_map=hm)
        var = orc.project_draws(cam.uniforms(), su, pp.tex, draws, height_map=hm)
    assert [st["n_instanced"], st["n_visible"], st["n_pairs16"]] == g["stats"].tolist()
    assert np.max(np.abs(img - g["image"])) <= 1e-6      # expf may differ in the last ulp across libm builds
    assert var.tobytes() == g["varyings"].tobytes()
    # the default (round 4): strict vertex stage + the fragment sequence F1..F4
    img, st = orc.render(cam.uniforms(), su, pp.tex, draws, W, H, height_map=hm)
    var = orc.project_draws(cam.uniforms(), su, pp.tex, draws, height_map=hm)
    assert [st["n_instanced"], st["n_visible"], st["n_pairs16"]] == g["stats_default"].tolist()
    assert np.max(np.abs(img - g["image_default"])) <= 1e-6
    assert var.tobytes() == g["varyings_strict"].tobytes()


@pytest.mark.parametrize("path", GOLD, ids=[os.path.basename(p) for p in GOLD])
def test_host_library_reproduces_golden_order(path):
    g, cfg, rows = _load(path)
    cfg.pop("__rc")
    W, H = [int(x) for x in g["size"]]
    pos, tgt = g["camera"][0], g["camera"][1]
    w = _host_wang(rows, cfg, g["tile_ids"], pos)
    cu, vp = host.camera_uniforms(pos, tgt, (0, 0, 1), 45.0, 0.1, 2400.0, W, H)
    s = w.sort_tiles(pos, vp)
    assert [t.map_index for t in s.tiles] == g["order"].tolist()
    assert [t.view_id for t in s.tiles] == g["views"].tolist()
    assert [t.lod for t in s.tiles] == g["lods"].tolist()


@pytest.mark.gpu
@pytest.mark.parametrize("path", GOLD, ids=[os.path.basename(p) for p in GOLD])
def test_gpu_matches_golden_image(renderer, path):
    g, cfg, rows = _load(path)
    rc = cfg.pop("__rc")
    W, H = [int(x) for x in g["size"]]
    pos, tgt = g["camera"][0], g["camera"][1]
    w = _host_wang(rows, cfg, g["tile_ids"], pos)
    cu, vp = host.camera_uniforms(pos, tgt, (0, 0, 1), 45.0, 0.1, 2400.0, W, H)
    s = w.sort_tiles(pos, vp)
    w.upload_to(renderer)
    renderer.configure(w.height_map() if cfg["surface_type"] == 1 else None)
    renderer.set_draws(s.draws, s.merged_gs_index, s.merged_map_id, s.merged_lod_id)
    su = w.scene_uniforms()
    su.draw_mode = int(rc.get("draw_mode", 0))
    img = renderer.render(cu, su, W, H)
    assert np.max(np.abs(img.astype(np.float64) - g["image_default"].astype(np.float64))) <= 1e-4
    t = renderer.timings()
    assert [t["n_visible"], t["n_pairs"]] == g["stats_default"].tolist()[1:]
    with renderer.options(STRICT_VS=0):    # the rounding sequence v2
        img2 = renderer.render(cu, su, W, H)
    assert np.max(np.abs(img2.astype(np.float64) - g["image"].astype(np.float64))) <= 1e-4
    t = renderer.timings()
    assert [t["n_visible"], t["n_pairs"]] == g["stats"].tolist()[1:]


PASSES = os.path.join(os.path.dirname(__file__), "golden", "passes_small.npz")


def _passes_inputs():
    g = np.load(PASSES, allow_pickle=False)
    ts = int(g["tex_size"])
    mips, off, n = [], 0, ts
    while n >= 1:
        mips.append(np.ascontiguousarray(g["mips"][off: off + n * n * 4].reshape(n, n, 4)))
        off += n * n * 4
        n //= 2
    W, H = [int(x) for x in g["size"]]
    cam = orc.Camera(W, H, g["camera"][0], g["camera"][1], [0, 0, 1])
    us = [orc.Proxy224.from_buffer_copy(bytes(u)) for u in g["uniforms"]]
    return g, mips, W, H, cam, us


def test_oracle_reproduces_golden_passes():
    """skybox + two proxy draws (GRID grid then map grid) on a HeightMap surface"""
    g, mips, W, H, cam, us = _passes_inputs()
    sky = orc.skybox_render(cam, g["faces"], W, H)
    assert np.max(np.abs(sky - g["sky"])) <= 1e-6
    rgba, depth = sky.copy(), np.ones((H, W), np.float32)
    for u in us:
        orc.proxy_render(u, W, H, rgba, depth, mips, height_map=g["hm"], grid_dim=int(g["grid_dim"]))
    assert depth.tobytes() == g["depth"].tobytes()
    assert np.max(np.abs(rgba - g["rgba"])) <= 1e-6


@pytest.mark.gpu
def test_gpu_matches_golden_passes(renderer):
    import torch
    g, mips, W, H, cam, us = _passes_inputs()
    renderer.configure(g["hm"])
    renderer.skybox_configure(g["faces"])
    renderer.proxy_configure(mips, grid_dim=int(g["grid_dim"]))
    rgba = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
    depth = torch.zeros((H, W), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    renderer.skybox_render(cam.uniforms(), W, H, rgba.data_ptr())
    renderer.synchronize()
    assert np.max(np.abs(rgba.cpu().numpy() - g["sky"])) <= 1e-5
    for k, u in enumerate(us):
        renderer.proxy_render(u, W, H, rgba.data_ptr(), depth.data_ptr(), clear_depth=(k == 0))
    renderer.synchronize()
    assert depth.cpu().numpy().tobytes() == g["depth"].tobytes()
    assert np.max(np.abs(rgba.cpu().numpy() - g["rgba"])) <= 1e-4
    renderer.configure(None)
