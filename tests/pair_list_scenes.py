"""The scenes of the pair-list tests (tests/test_pair_list_cpu.py, tests/test_pair_list_gpu.py; no tests here): small frames whose
per-tile lists the oracle can enumerate, each built once per session in both representations (tests.helpers.Case)."""
from __future__ import annotations

import dataclasses
import functools

import numpy as np

from oracle import gswt_oracle as orc
from tests import helpers as H
from tests import pair_list_ref as PL
from tests import special_splats as SP


@dataclasses.dataclass
class Scene:
    name: str
    W: int
    H: int
    cam: orc.Camera176
    su: orc.Scene160
    case: H.Case
    hm: np.ndarray | None = None
    wall_entries: np.ndarray | None = None      # occlusion scene: the oracle entry indices of the wall's splats

    @property
    def tiles(self):
        return (self.W + 15) // 16, (self.H + 15) // 16

    def rects(self, bg_depth=None):
        return orc.pair_rects(self.cam, self.su, self.case.pp.tex, self.case.orc_draws, self.W, self.H, height_map=self.hm,
                              bg_depth=bg_depth)

    def render(self, order_mode=0, **kw):
        return orc.render(self.cam, self.su, self.case.pp.tex, self.case.orc_draws, self.W, self.H, height_map=self.hm,
                          order_mode=order_mode, **kw)

    def expected(self, order_mode, bg_depth=None) -> PL.PairLists:
        return PL.expected_lists(self.rects(bg_depth), order_mode, *self.tiles)


def grid_merged_case(pp, *, half=(1, 2), tile_width=4.0, view=2, merged_cells=((0, 3), (1, 3)), merged_at=5, repeat=1, n_tile=None):
    """H.grid_case's plain class-A draws, except that `merged_cells` ((mx, my) map cells) form one merged (single_draw) draw with
    per-splat map ids, submitted as draw number `merged_at`.  repeat = 2: the whole draw list once more behind itself."""
    case = H.Case(pp)
    n_tile = pp.n_tile if n_tile is None else n_tile
    hx, hy = half
    wy = 2 * hy + 1
    for _ in range(repeat):
        n = 0
        for my in range(2 * hy, -1, -1):
            for mx in range(2 * hx + 1):
                if n == merged_at and merged_cells:
                    members = [(cx * wy + cy, 0, (cx * 7 + cy * 3) % n_tile, None) for cx, cy in merged_cells]
                    case.add_merged(members=members, view=view, head_lod=0, head_tile=members[0][2], head_map_index=members[0][0])
                n += 1
                if (mx, my) in merged_cells:
                    continue
                case.add_static(lod=0, tile=(mx * 7 + my * 3) % n_tile, view=view,
                                offset=((mx - hx) * tile_width, (my - hy) * tile_width, 0.0), valid_lod_id=0,
                                map_index=mx * wy + my, map_coord=(mx, my))
    return case


# the 3 x 5 map of 4-unit cells spans x in [-4, 8], y in [-8, 12]: seen from above its middle, nearly every screen tile has a list
DOWN_CAMERA = ((2.0, -3.0, 9.0), (2.0, 2.0, 0.0))


def _camera(W, Hh, pos_tgt=DOWN_CAMERA):
    return orc.Camera(W, Hh, pos_tgt[0], pos_tgt[1], [0, 0, 1]).uniforms()


@functools.lru_cache(maxsize=None)
def plane() -> Scene:
    """17 x 11 tiles: a frame whose width and height are no multiple of anything the kernels tile by but 16."""
    pp = H.tileset()
    W, Hh = 272, 176
    return Scene("plane", W, Hh, _camera(W, Hh), orc.scene_uniforms(num_lod=pp.n_lod, map_half_wh=(1, 2)), grid_merged_case(pp))


@functools.lru_cache(maxsize=None)
def hmap() -> Scene:
    pp = H.tileset()
    W, Hh = 320, 240
    hm = np.random.default_rng(5).random((16, 16), dtype=np.float32)
    su = orc.scene_uniforms(num_lod=pp.n_lod, map_half_wh=(1, 2), surface_type=1, height_map_scale=(1.0, 1.0, 0.4))
    return Scene("hmap", W, Hh, _camera(W, Hh), su, grid_merged_case(pp), hm=hm)


@functools.lru_cache(maxsize=None)
def sphere() -> Scene:
    from tests.test_render_parity_gpu import _sphere_case
    pp = H.tileset()
    W, Hh = 320, 240
    su = orc.scene_uniforms(num_lod=pp.n_lod, map_half_wh=(5, 2), surface_type=2, sphere_radius=6.5)
    cam = orc.Camera(W, Hh, (3.0, -19.0, 6.0), (0.0, 0.0, 0.0), [0, 0, 1]).uniforms()
    return Scene("sphere", W, Hh, cam, su, _sphere_case(pp))


SURFACES = {"plane": plane, "hmap": hmap, "sphere": sphere}


@functools.lru_cache(maxsize=None)
def dense() -> Scene:
    """Many splats on few tiles, seen at a grazing angle: the horizon tiles' lists pass 4096 pairs and many pass 512 (asserted on the
    oracle's lists by the tests), so a tile has several compositor segments and the tile-local depth sort meets its three size classes."""
    pp = H.tileset(lod0_count=12000, base_scale=0.05)
    W, Hh = 272, 176
    return Scene("dense", W, Hh, _camera(W, Hh, ((2.0, -9.5, 0.9), (2.0, 4.0, 0.0))), orc.scene_uniforms(num_lod=pp.n_lod, map_half_wh=(1, 2)),
                 grid_merged_case(pp))


TWIN_CAMERAS = tuple(((2.0 + dx, -3.0 + dy, 9.0 + dz), (2.0 + dx, 2.0 + dy, 0.0))
                     for dx, dy, dz in ((0, 0, 0), (-1.5, 0, 0), (1.5, 1, 0), (0, 2, -1)))


@functools.lru_cache(maxsize=None)
def twins(k: int = 0) -> Scene:
    """The plane scene's draw list submitted twice: every splat has a twin of identical depth bits in a later draw.  A 320 x 240
    frame has 300 tile lists; the TWIN_CAMERAS frames together have more than 1000 that hold such a tie (asserted by the tests)."""
    pp = H.tileset()
    W, Hh = 320, 240
    return Scene(f"twins{k}", W, Hh, _camera(W, Hh, TWIN_CAMERAS[k]), orc.scene_uniforms(num_lod=pp.n_lod, map_half_wh=(1, 2)),
                 grid_merged_case(pp, repeat=2))


WALL_Z = 6.0                            # the wall's plane, 3 units under DOWN_CAMERA, which looks down along (0, 5, -9)
WALL_X, WALL_Y = (1.0, 3.0), (-2.2, -0.6)
WALL_STEP, WALL_SIGMA = 0.05, 0.06


@functools.lru_cache(maxsize=None)
def wall() -> Scene:
    """The plane scene behind a wall of opaque splats (alpha byte 255, spaced closer than their sigma) that covers the middle of the
    frame: drawn last, so in front of everything in reference order, and nearest in depth order too."""
    pp0 = H.tileset()
    xs = np.arange(WALL_X[0], WALL_X[1] + 1e-6, WALL_STEP)
    ys = np.arange(WALL_Y[0], WALL_Y[1] + 1e-6, WALL_STEP)
    halves = SP.diag_halves((WALL_SIGMA, WALL_SIGMA, WALL_SIGMA))
    rows = np.stack([SP.tex_row((x, y, WALL_Z), halves, rgba=(40 + (i * 37) % 200, 40 + (j * 53) % 200, 90, 255))
                     for i, x in enumerate(xs) for j, y in enumerate(ys)])
    first = pp0.tex.reshape(-1, 8).shape[0]
    idx = np.arange(first, first + rows.shape[0], dtype=np.uint32)
    zero = np.zeros(rows.shape[0], dtype=np.uint32)
    # one more tile of the scene's static lists holds the wall, the same list for every view and LOD
    pp = dataclasses.replace(pp0, n_tile=pp0.n_tile + 1, tex=np.concatenate([pp0.tex.reshape(-1, 8), rows]),
                             gs_index=[lod + [[idx] * pp0.n_view] for lod in pp0.gs_index],
                             gs_lod_id=[lod + [[zero] * pp0.n_view] for lod in pp0.gs_lod_id])
    case = grid_merged_case(pp, n_tile=pp0.n_tile)
    n_before = sum(int(np.asarray(d.gs_index).shape[0]) for d in case.orc_draws)
    case.add_static(lod=0, tile=pp0.n_tile, view=2, offset=(0.0, 0.0, 0.0), valid_lod_id=0)
    W, Hh = 272, 176
    return Scene("wall", W, Hh, _camera(W, Hh), orc.scene_uniforms(num_lod=pp.n_lod, map_half_wh=(1, 2)), case,
                 wall_entries=np.arange(n_before, n_before + rows.shape[0]))


def twin_tie_tiles(sc):
    """Tile lists of the depth-ordered frame in which two neighbours have the same depth bits."""
    e = sc.expected(PL.ORDER_DEPTH)
    d = sc.rects()["depth"].view(np.uint32)
    return sum(1 for t in range(e.n_tiles) if (np.diff(d[e.tile(t)].astype(np.int64)) == 0).any())


def wall_hidden_tiles(sc, mode):
    """Tiles whose list holds at least 4 wall splats with at least 50 pairs behind the last of them."""
    e = sc.expected(mode)
    w0 = int(sc.wall_entries[0])
    n = 0
    for t in range(e.n_tiles):
        l = e.tile(t)
        iw = np.nonzero(l >= w0)[0]
        n += int(iw.size >= 4 and l.shape[0] - int(iw[-1]) - 1 >= 50)
    return n


ALL = {"plane": plane, "hmap": hmap, "sphere": sphere, "dense": dense, "wall": wall,
       **{f"twins{k}": functools.partial(twins, k) for k in range(len(TWIN_CAMERAS))}}
