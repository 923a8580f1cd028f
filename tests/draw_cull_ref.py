"""A plain restatement of the per-draw viewport cull and LOD skip of renderer.rs:472-497, independent of the HIP kernel
(k_cull / draw_is_culled) and of the oracle's draw loop (wangtile_oracle.renderer_draws): the three cull terms of one draw in
binary32, one rounded operation at a time, the same in float64, the keep rule and the LOD-enable bit.  Also the one scene the
cull tests share (the oracle's side of it), built once per session."""
from __future__ import annotations

import functools
import struct

import numpy as np

f32 = np.float32
FLT_MAX = f32(np.finfo(np.float32).max)


def _terms(vp16, corners12, t):
    """min |x/w|, min |y/w|, max z/w over the four corners in number type t: each clip coordinate is
    ((VP[r] x + VP[4+r] y) + VP[8+r] z) + VP[12+r] 1, every product, sum and quotient rounded to t on its own.  The minima
    start from FLT_MAX and are replaced on a strict <, the maximum from -FLT_MAX on a strict >: a NaN never replaces the
    running value."""
    vp = [t(x) for x in np.asarray(vp16, dtype=np.float32).reshape(16)]
    p = [t(x) for x in np.asarray(corners12, dtype=np.float32).reshape(12)]
    one = t(1.0)
    mx, my, mz = t(FLT_MAX), t(FLT_MAX), t(-FLT_MAX)
    with np.errstate(all="ignore"):
        for ci in range(4):
            x, y, z = p[3 * ci], p[3 * ci + 1], p[3 * ci + 2]
            c = []
            for r in range(4):
                a = t(vp[r] * x)
                a = t(a + t(vp[4 + r] * y))
                a = t(a + t(vp[8 + r] * z))
                a = t(a + t(vp[12 + r] * one))
                c.append(a)
            cx, cy, cz = t(c[0] / c[3]), t(c[1] / c[3]), t(c[2] / c[3])
            if abs(cx) < mx:
                mx = t(abs(cx))
            if abs(cy) < my:
                my = t(abs(cy))
            if cz > mz:
                mz = cz
    return mx, my, mz


def cull_terms(vp16, corners12):
    """(mx, my, mz) in binary32."""
    return _terms(vp16, corners12, np.float32)


def cull_terms64(vp16, corners12):
    """(mx, my, mz) in float64 from the same binary32 inputs."""
    return _terms(vp16, corners12, np.float64)


def keeps(terms, culling_dist) -> bool:
    """renderer.rs:490: the draw is dropped when mz < -clip || mx > clip || my > clip, clip = culling_dist as f32.  Every
    comparison with a NaN is false, so a NaN clip keeps everything."""
    mx, my, mz = terms
    clip = f32(culling_dist)
    return not (mz < -clip or mx > clip or my > clip)


def lod_kept(mask: int, lod: int) -> bool:
    """Bit lod & 31 of the u32 lod_enable_mask."""
    return bool(((int(mask) & 0xFFFFFFFF) >> (int(lod) & 31)) & 1)


def margin(terms, culling_dist) -> float:
    """Smallest relative distance of a term from the bound it is compared with (|t - b| / max(|t|, |b|); inf where they
    cannot meet: a NaN on either side, or both zero / equal infinities count as distance 0)."""
    clip = np.float64(f32(culling_dist))
    if np.isnan(clip):
        return float("inf")
    m = float("inf")
    for t, b in ((terms[0], clip), (terms[1], clip), (terms[2], -clip)):
        t = np.float64(t)
        if np.isnan(t):
            continue
        if t == b:
            return 0.0
        if np.isinf(t) or np.isinf(b):
            continue
        m = min(m, float(abs(t - b) / max(abs(t), abs(b))))
    return m


def f32_bits(x) -> int:
    return struct.unpack("<I", struct.pack("<f", f32(x)))[0]


def next_toward_zero(x):
    """nextafter(x, 0) in binary32."""
    return np.nextafter(f32(x), f32(0.0))


# ---------------------------------------------------------------------------------------------------------------------
# The scene of the cull tests: 7 x 7 map, plain surface, Graph order, Edge merge -- 46 tile instances (23 plain, 20 blending,
# 3 merged; 43 with corner data).
# ---------------------------------------------------------------------------------------------------------------------
CFG = dict(tile_map_half_wh=(3, 3), surface_type=0, lod_max_dist=20.0, tile_sort_type=3, merge_type=2)
CAM = ((4.2, 1.0, 3.0), (5.0, 3.0, 2.5))
W, H = 272, 176
TILESET = dict(n_lod=3, n_tile=16, lod0_count=300)
INF, NAN = float("inf"), float("nan")
# draws kept per culling_dist with every LOD enabled, and per LOD mask at culling_dist 1 (walked with the oracle)
CULL_DISTS = [(0.0, 3), (0.25, 7), (0.5, 9), (0.75, 11), (1.0, 13), (1.5, 25), (3.0, 37), (10.0, 46), (INF, 46), (NAN, 46), (-1.0, 3)]
LOD_MASKS = [(0, 0), (1, 2), (2, 5), (3, 7), (4, 6), (5, 8), (6, 11), (7, 13)]


class Scene:
    """The oracle's side of the scene: tile set, sorted instances, every draw (culling_dist = inf) and the f32 terms of each."""

    def __init__(self):
        from gswt_renderer_amd import synth
        from oracle import gswt_oracle as orc
        from oracle import wangtile_oracle as wo
        self.verts = synth.make_tileset(**TILESET)
        self.pp = orc.preprocess([[orc.scene_load(v) for v in lod] for lod in self.verts])
        ow = wo.WangTile(self.pp)
        self.user = ow.configure(wo.UserData(**CFG))
        self.cam = orc.Camera(W, H, CAM[0], CAM[1], [0, 0, 1])
        self.vp = self.cam.view_proj()
        sd = ow.build_tiles(CAM[0])
        self.sort = ow.sort_tiles(CAM[0], self.vp)
        self.su = wo.scene_uniforms_from_data(self.user, sd["center_coord"])
        self.insts = list(self.sort["tile_instance_vec"])
        self.cull_enable = [len(key[1]) == 1 for key, _ in self.sort["render_data_vec"]]
        self.corners = [np.stack([ti.corner_data[ci][0] for ci in range(4)]).astype(np.float32) if ti.corner_data is not None else None
                        for ti in self.insts]
        self.lod = [int(ti.tid[0]) for ti in self.insts]
        self.map_index = [int(ti.map_index) for ti in self.insts]
        self.terms = [cull_terms(self.vp, c) if ce else None for ce, c in zip(self.cull_enable, self.corners)]
        self.all_draws = wo.renderer_draws(self.pp, self.sort, self.vp, culling_dist=INF)
        assert [int(d.tile.map_index) for d in self.all_draws] == self.map_index
        self.kind = ["merged" if d.tile.single_draw else ("blend" if d.tile.changing else "plain") for d in self.all_draws]

    def oracle_draws(self, culling_dist=1.0, mask=0xFFFFFFFF):
        from oracle import wangtile_oracle as wo
        n_lod = TILESET["n_lod"]
        return wo.renderer_draws(self.pp, self.sort, self.vp, culling_dist=culling_dist,
                                 lod_enable=[lod_kept(mask, l) for l in range(n_lod)])

    def ref_keep(self, culling_dist=1.0, mask=0xFFFFFFFF):
        """Per instance: does draw_cull_ref keep it?"""
        return [(not ce or keeps(t, culling_dist)) and lod_kept(mask, l)
                for ce, t, l in zip(self.cull_enable, self.terms, self.lod)]

    def g(self, i):
        """The governing term max(mx, my) of instance i (binary32)."""
        mx, my, _ = self.terms[i]
        return mx if mx >= my else my


@functools.lru_cache(maxsize=1)
def scene() -> Scene:
    return Scene()
