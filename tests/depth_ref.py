"""CPU reference of the composited depth image (gswt_render_depth, include/gswt_hip.h), in numpy.

Composites the projected instances of orc.project_draws -- `visible`, `ndc`, `depth`, `major`, `minor`, `rgba` -- in the
oracle's blend order (reference order: draw order, list position; depth order: stably by descending depth), with the oracle's
fragment sequence F1..F4 (oracle/gswt_oracle.c frag_setup / raster_over) and its depth test against bg_depth (1.0 without one).
Depth rides along as one more colour channel of the "over" blend, starting from the background depth z_bg:

    z <- B z_i + (1 - B) z            (back to front)   ==   Z = T z_bg + sum_i w_i z_i   (front to back, w_i = T_i e_i)

It is only trusted because its colour reproduces orc.render (tests/test_depth_out_cpu.py)."""
from __future__ import annotations

import numpy as np

F32 = np.float32


def _fma(a, b, c):
    """binary32 fma(a, b, c): the product of two binary32 is exact in binary64; one more rounding to binary32 at the end."""
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(F32)


def _frag_setup(sp, splat_scale: float, W: int, H: int):
    """F1, F2 and the conservative pixel box of every instance (frag_setup of the oracle), as float32 arrays."""
    ndc = sp["ndc"].astype(F32)
    major, minor = sp["major"].astype(F32), sp["minor"].astype(F32)
    with np.errstate(all="ignore"):
        cxp = _fma(F32(0.5), ndc[:, 0], F32(0.5)) * F32(W)
        cyp = _fma(F32(-0.5), ndc[:, 1], F32(0.5)) * F32(H)
        hs = F32(0.5) * F32(splat_scale)
        ux, uy = hs * major[:, 0], -(hs * major[:, 1])
        vx, vy = hs * minor[:, 0], -(hs * minor[:, 1])
        uu = _fma(uy, uy, ux * ux)
        vv = _fma(vy, vy, vx * vx)
        ok = (uu > 0) & (vv > 0) & (uu < np.inf) & (vv < np.inf)
        ruu, rvv = F32(1.0) / uu, F32(1.0) / vv
        iux, iuy, ivx, ivy = ux * ruu, uy * ruu, vx * rvv, vy * rvv
        hx = _fma(F32(2.0) * np.sqrt(_fma(vx, vx, ux * ux)), F32(1.00001), F32(0.001))
        hy = _fma(F32(2.0) * np.sqrt(_fma(vy, vy, uy * uy)), F32(1.00001), F32(0.001))
        fx0, fx1 = np.ceil(cxp - hx - F32(0.5)), np.floor(cxp + hx - F32(0.5))
        fy0, fy1 = np.ceil(cyp - hy - F32(0.5)), np.floor(cyp + hy - F32(0.5))
    return dict(ok=ok, iux=iux, iuy=iuy, ivx=ivx, ivy=ivy, fx0=fx0, fx1=fx1, fy0=fy0, fy1=fy1)


def composite(sp, W: int, H: int, *, splat_scale: float = 1.0, order_mode: int = 0, bg_rgba=None, bg_depth=None, with_cover=False):
    """Returns (image [H, W, 4] f32, depth [H, W] f32) of the instances `sp` (orc.SPLAT_DTYPE, draw order); with_cover: also the
    number of splats that cover each pixel (pass its coverage and depth test), [H, W] int."""
    fs = _frag_setup(sp, splat_scale, W, H)
    vis = (sp["visible"] == 1) & fs["ok"]
    idx = np.nonzero(vis)[0]
    if order_mode == 1:
        idx = idx[np.argsort(-sp["depth"][idx].astype(np.float64), kind="stable")]
    img = np.zeros((H, W, 4), F32) if bg_rgba is None else np.array(bg_rgba, F32).reshape(H, W, 4)
    zbg = np.ones((H, W), F32) if bg_depth is None else np.array(bg_depth, F32).reshape(H, W)
    z = zbg.copy()
    n_cover = np.zeros((H, W), np.int64)
    hW, hH = F32(0.5) * F32(W), F32(0.5) * F32(H)
    for k in idx:
        fx0, fx1, fy0, fy1 = fs["fx0"][k], fs["fx1"][k], fs["fy0"][k], fs["fy1"][k]
        if not (fx1 >= fx0 and fy1 >= fy0 and fx1 >= 0 and fy1 >= 0 and fx0 <= W - 1 and fy0 <= H - 1):
            continue
        x0, x1 = (0 if fx0 < 0 else int(fx0)), (W - 1 if fx1 > W - 1 else int(fx1))
        y0, y1 = (0 if fy0 < 0 else int(fy0)), (H - 1 if fy1 > H - 1 else int(fy1))
        xs = np.arange(x0, x1 + 1, dtype=np.int64)[None, :]
        ys = np.arange(y0, y1 + 1, dtype=np.int64)[:, None]
        bx, by = (xs & ~15).astype(F32), (ys & ~15).astype(F32)
        iux, iuy, ivx, ivy = fs["iux"][k], fs["iuy"][k], fs["ivx"][k], fs["ivy"][k]
        # F3: per 16 x 16 block (the block origin of every pixel), F4: per pixel
        ox = _fma(hW, sp["ndc"][k, 0], hW - bx)
        oy = _fma(-hH, sp["ndc"][k, 1], hH - by)
        nku = -_fma(iux, ox, iuy * oy)
        nkv = -_fma(ivx, ox, ivy * oy)
        ly = (ys.astype(F32) - by) + F32(0.5)
        lx = (xs.astype(F32) - bx) + F32(0.5)
        px = _fma(iux, lx, _fma(iuy, ly, nku))
        py = _fma(ivx, lx, _fma(ivy, ly, nkv))
        r2 = _fma(py, py, px * px)
        dk = F32(sp["depth"][k])
        cover = (r2 <= F32(4.0)) & (dk < zbg[y0:y1 + 1, x0:x1 + 1])
        if not cover.any():
            continue
        cy, cx = np.nonzero(cover)
        cy, cx = cy + y0, cx + x0
        B = np.exp(-r2[cover]).astype(F32) * F32(sp["rgba"][k, 3])
        om = F32(1.0) - B
        d = img[cy, cx]
        rgba = sp["rgba"][k].astype(F32)
        d[:, 0] = B * rgba[0] + d[:, 0] * om
        d[:, 1] = B * rgba[1] + d[:, 1] * om
        d[:, 2] = B * rgba[2] + d[:, 2] * om
        d[:, 3] = B + d[:, 3] * om
        img[cy, cx] = d
        z[cy, cx] = B * dk + z[cy, cx] * om
        n_cover[cy, cx] += 1
    return (img, z, n_cover) if with_cover else (img, z)


def golden_case(name: str, *, W: int | None = None, H: int | None = None, verts=None):
    """One of tests/golden/make_golden.py's CASES built the way that script builds it (not read from its .npz): the tile set, the
    oracle's draws, camera and scene uniforms, and the projected instances.  W, H: another frame size for the same view.
    verts: another tile set ([lod][tile] [n, 62], the case's n_lod LODs of 16 tiles) in the place of synth.make_tileset's, under the
    same configuration, camera and sort event (tests/hostile_cases.py)."""
    import importlib.util
    import os

    from gswt_renderer_amd import synth
    from oracle import gswt_oracle as orc
    from oracle import wangtile_oracle as wo

    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "make_golden.py")
    spec = importlib.util.spec_from_file_location("_make_golden", path)
    mg = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mg)
    c = mg.CASES[name]
    W, H = W or c["W"], H or c["H"]
    if verts is None:
        verts = synth.make_tileset(n_lod=c["n_lod"], n_tile=16, lod0_count=c["lod0"])
    assert len(verts) == c["n_lod"] and all(len(lod) == 16 for lod in verts)
    pp = orc.preprocess([[orc.scene_load(v) for v in lod] for lod in verts])
    ow = wo.WangTile(pp)
    ou = ow.configure(wo.UserData(**c["cfg"]))
    cam = orc.Camera(W, H, c["pos"], c["tgt"], [0, 0, 1])
    with np.errstate(all="ignore"):
        osd = ow.build_tiles(c["pos"])
        osort = ow.sort_tiles(c["pos"], cam.view_proj())
        draws = wo.renderer_draws(pp, osort, cam.view_proj())
    su = wo.scene_uniforms_from_data(ou, osd["center_coord"], **c.get("render_config", {}))
    hm = ou.height_map.reshape(ou.height_map_wh[1], ou.height_map_wh[0]) if ou.surface_type == 1 else None
    sp = orc.project_draws(cam.uniforms(), su, pp.tex, draws, height_map=hm)
    return dict(cfg=c["cfg"], pos=c["pos"], tgt=c["tgt"], W=W, H=H, verts=verts, pp=pp, cam=cam, su=su, draws=draws, hm=hm, sp=sp)


def bg_images(W: int, H: int, seed: int = 5):
    """A background colour and a proxy depth buffer in the range the splats' depths fall in (some splats in front, some behind)."""
    rng = np.random.default_rng(seed)
    return rng.uniform(0, 1, size=(H, W, 4)).astype(F32), rng.uniform(0.97, 1.0, size=(H, W)).astype(F32)
