"""The scenes of the pair-list tests (tests/test_pair_list_cpu.py, tests/test_pair_list_gpu.py and their _modes siblings; no tests
here): small frames whose per-tile lists the oracle can enumerate, each built once per session in both representations
(tests.helpers.Case), and the same scenes as orthographic, anti-aliased and faded frames (framed)."""
from __future__ import annotations

import dataclasses
import functools
import math

import numpy as np

from oracle import gswt_oracle as orc
from tests import antialias_ref as AA
from tests import atmosphere_ref as AT
from tests import helpers as H
from tests import ortho_ref as OR
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
    mode: "Mode | None" = None                  # a frame of framed(): orthographic camera, pixel filter, far fade (None: all off)
    aa_s: float = 0.0                           # the filter's s as the host computes it (tests/antialias_ref.py: aa_s)
    ramp: tuple | None = None                   # the far fade's (fade_start, fade_end), binary32 numbers
    ortho_args: dict | None = None              # tests/ortho_ref.py camera arguments of an orthographic frame (cam is their block)

    @property
    def tiles(self):
        return (self.W + 15) // 16, (self.H + 15) // 16

    def oracle_mode(self):
        """The oracle's switches of this frame (a context manager; the plain scenes': everything off)."""
        fade = None
        if self.ramp is not None:
            p = AT.params(self.atmosphere())
            fade = (float(p["fade_end"]), float(p["fade_inv"]))
        return orc.frame_mode(ortho=int(self.ortho_args is not None), aa_s=self.aa_s, fade=fade)

    def atmosphere(self):
        from gswt_renderer_amd import atmosphere
        return atmosphere.Atmosphere(fade=self.ramp) if self.ramp is not None else atmosphere.OFF

    def rects(self, bg_depth=None):
        with self.oracle_mode():
            return orc.pair_rects(self.cam, self.su, self.case.pp.tex, self.case.orc_draws, self.W, self.H, height_map=self.hm,
                                  bg_depth=bg_depth)

    def records(self):
        with self.oracle_mode():
            return orc.project_draws(self.cam, self.su, self.case.pp.tex, self.case.orc_draws, height_map=self.hm)

    def render(self, order_mode=0, **kw):
        with self.oracle_mode():
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


# ---- frames with the orthographic projection, the pixel filter and the far fade -----------------------------------------------------------
@dataclasses.dataclass(frozen=True)
class Mode:
    """What a frame has beside vs_main: ortho = the name of one of the scene's ORTHO_CAMERAS (None: the scene's perspective camera),
    aa = GSWT_OPT_ANTIALIAS' value (0: off), fade = the far fade over the scene's own ramp."""
    ortho: str | None = None
    aa: int = 0
    fade: bool = False

    @property
    def id(self):
        return "-".join(([f"ortho_{self.ortho}"] if self.ortho else []) + ([f"aa{self.aa}"] if self.aa else []) + (["fade"] if self.fade else [])) or "plain"


_EL35 = math.radians(35.0)
# The orthographic cameras (tests/ortho_ref.py: camera_args' form), lod_pos = the scene's perspective eye.  "top" looks straight down on the
# middle of the map, "oblique" from the south at 35 degrees elevation, 30 units away.  The depth ranges (z_top 500 above a scene a few
# units high; near = -2000) are far wider than the scenes: orthographic depth is linear, so the splats' depths crowd into the few tens of
# thousands of binary32 numbers just below 1.0, and lists in depth order hold ties between different splats (asserted by
# tests/test_pair_list_modes_cpu.py).  Faded frames use the oblique camera on the plane: under "top" a quarter fewer splats leave
# fewer than the 10 000 pairs that test asks of a plane frame.
ORTHO_CAMERAS = {
    "plane": dict(
        top=dict(kind="top_down", center_xy=(2.0, 2.0), half_extent=4.0, z_top=500.0, z_bottom=-1.0, lod_pos=DOWN_CAMERA[0]),
        oblique=dict(kind="look_at", eye=(2.0, 2.0 - 30.0 * math.cos(_EL35), 30.0 * math.sin(_EL35)), target=(2.0, 2.0, 0.0), up=(0.0, 0.0, 1.0),
                     half_height=4.0, near=-2000.0, far=40.0, lod_pos=DOWN_CAMERA[0])),
    "sphere": dict(
        top=dict(kind="top_down", center_xy=(0.0, 0.0), half_extent=8.0, z_top=500.0, z_bottom=-8.0, lod_pos=(3.0, -19.0, 6.0)),
        oblique=dict(kind="look_at", eye=(3.0, -19.0, 6.0), target=(0.0, 0.0, 0.0), up=(0.0, 0.0, 1.0), half_height=8.0, near=-2000.0, far=35.0,
                     lod_pos=(3.0, -19.0, 6.0))),
}
ORTHO_CAMERAS["hmap"] = ORTHO_CAMERAS["plane"]
ORTHO_CAMERAS["dense"] = ORTHO_CAMERAS["plane"]

BANDS_SPLAT_SCALE = 0.03
BANDS_EYE = (1.87, 2.0, 40.0)


@functools.lru_cache(maxsize=None)
def bands() -> Scene:
    """The plane scene for column bands with the filter on, built so that a band cull whose pad forgets the filter loses pairs.  The
    filter's reach is sqrt(8 v) px whatever the splat scale (5.7 px at 4096), while the unfiltered pad of k_cull's band bound, 1.25 * 2
    splat_scale sqrt(bound of lambda) + 2 px, shrinks with the scale: 3.1 px at splat_scale 0.03.  The camera looks straight down from
    far away through a narrow angle (the same 23.6 px per world unit as from 9 units at 45 degrees, but the +-0.6 units of height in a
    cell's box now move its projection by 0.7 px, not 3), so the map's cell edges are vertical screen lines, and the eye's x puts the edge
    x = 0 four pixels left of the boundary between the first two of three 96-pixel bands: the cells left of it miss band 1 by the
    unfiltered pad, and their grown splats still reach it (pairs_lost_by_an_unfiltered_band_pad, asserted by
    tests/test_pair_list_modes_cpu.py)."""
    base = plane()
    su = orc.Scene160.from_buffer_copy(bytes(base.su))
    su.splat_scale = BANDS_SPLAT_SCALE
    fovy = 2.0 * math.degrees(math.atan(math.tan(math.radians(22.5)) * 9.0 / BANDS_EYE[2]))
    cam = orc.Camera(base.W, base.H, BANDS_EYE, (BANDS_EYE[0], BANDS_EYE[1], 0.0), [0, 1, 0], fovy_deg=fovy).uniforms()
    return dataclasses.replace(base, name="bands", cam=cam, su=su)


def _band_misses(cam, su, lo, hi, max_trace, aa_s, col0, col1, W):
    """k_cull's band_misses on the plain surface, in float64: the box's eight corners projected, padded by the bound of a splat's reach."""
    VP = np.array(cam.projection, np.float64).reshape(4, 4).T @ np.array(cam.view, np.float64).reshape(4, 4).T
    xs, ws = [], []
    for k in range(8):
        c = VP @ np.array([hi[0] if k & 1 else lo[0], hi[1] if k & 2 else lo[1], hi[2] if k & 4 else lo[2], 1.0])
        xs.append((0.5 * c[0] / c[3] + 0.5) * W)
        ws.append(c[3])
    if not min(ws) > 1e-6:
        return False
    hx, hy = 1.3 * cam.htan_fov[0], 1.3 * cam.htan_fov[1]
    jn2 = (cam.focal[0] ** 2 * (1.0 + hx * hx) + cam.focal[1] ** 2 * (1.0 + hy * hy)) / min(ws) ** 2
    ss = abs(su.splat_scale)
    rad = min(2.0 * ss * math.sqrt(jn2 * max(max_trace, 0.0) + aa_s), 1448.2 * ss) * 1.25 + 2.0
    return max(xs) + rad < col0 * 16 or min(xs) - rad >= col1 * 16


def pairs_lost_by_an_unfiltered_band_pad(sc, count, with_filter_term=False):
    """A model of the column-band cull (k_cull: a static draw, or a merged draw's cell, is dropped for a band when the box of its splat
    centres, padded by a bound of their reach, misses the band's pixel columns) whose pad leaves out the filter's s: the pairs of sc's
    filtered frame, from the oracle's rectangles, that lie in a band for which their draw or cell would be dropped.  Plain surface.
    with_filter_term: the pad as the kernel has it -- no pair may be lost then."""
    assert sc.su.surface_type == 0
    pp, su = sc.case.pp, sc.su
    pos = np.concatenate([orc.rows_positions(r) for lod in pp.rows for r in lod]).astype(np.float64)
    lo, hi = pos.min(0), pos.max(0)
    hf = OR._half_table().astype(np.float64)
    t = np.ascontiguousarray(pp.tex, dtype=np.uint32).reshape(-1, 8)
    max_trace = float((hf[t[:, 4] & 0xFFFF] + hf[t[:, 5] >> 16] + hf[t[:, 6] >> 16]).max())
    r = sc.rects()
    tx = sc.tiles[0]
    bt = -(-tx // count)
    wy = 2 * su.map_half_wh[1] + 1
    lost, base = 0, 0
    for d in sc.case.orc_draws:
        n = int(np.asarray(d.gs_index).shape[0])
        rr = r[base:base + n]
        base += n
        if d.tile.single_draw == 1:
            mid = np.asarray(d.map_id)
            groups = [((((int(m) // wy) - su.map_half_wh[0] + su.center_coord[0]) * su.tile_width,
                        ((int(m) % wy) - su.map_half_wh[1] + su.center_coord[1]) * su.tile_width, 0.0), mid == m) for m in np.unique(mid)]
        else:
            groups = [(tuple(d.tile.offset[:3]), np.ones(n, bool))]
        for off, sel in groups:
            q = rr[sel & (rr["visible"] == 1)]
            rows = np.maximum(q["ty1"].astype(np.int64) - q["ty0"] + 1, 0)
            for b in range(count):
                c0, c1 = b * bt, min(tx, (b + 1) * bt)
                if _band_misses(sc.cam, su, lo + off, hi + off, max_trace, sc.aa_s if with_filter_term else 0.0, c0, c1, sc.W):
                    cols = np.maximum(np.minimum(q["tx1"], c1 - 1).astype(np.int64) - np.maximum(q["tx0"], c0) + 1, 0)
                    lost += int((cols * rows).sum())
    return lost


@functools.lru_cache(maxsize=None)
def framed(name: str, mode: Mode) -> Scene:
    """Scene `name` as a frame in `mode`: the camera block, the filter's s and the fade's ramp are inputs worked out here once; every
    oracle call of the returned Scene runs under them (Scene.oracle_mode).  The ramp is the 30th .. 75th percentile of the distances of
    the frame's otherwise visible splats from cam_pos (float64, from the unfaded records; the ramp is an input, not a result)."""
    base = (bands if name == "bands" else ALL[name])()
    cam, args = base.cam, None
    if mode.ortho:
        args = ORTHO_CAMERAS[name][mode.ortho]
        cam = OR.block_of(args, base.W, base.H)
    aa_s = float(AA.aa_s(mode.aa, base.su.splat_scale)) if mode.aa else 0.0
    sc = dataclasses.replace(base, name=f"{name}-{mode.id}", cam=cam, mode=mode, aa_s=aa_s, ortho_args=args)
    if mode.fade:
        sp = sc.records()
        vis = sc.rects()["visible"] == 1
        dist, _ = AT.dist_f64(cam, sp["ndc"][vis], sp["depth"][vis])
        sc = dataclasses.replace(sc, ramp=AT.ramp_from_percentiles(dist))
    return sc


def ortho_camera(sc):
    """The product's camera object of an orthographic frame (gswt_renderer_amd/ortho.py); its block must be sc.cam byte for byte."""
    return OR.ortho_camera_of(sc.ortho_args, sc.W, sc.H)


def rect_areas(r):
    w = np.maximum(r["tx1"].astype(np.int64) - r["tx0"] + 1, 0)
    h = np.maximum(r["ty1"].astype(np.int64) - r["ty0"] + 1, 0)
    return w * h


# The frames of tests/test_pair_list_modes_gpu.py; tests/test_pair_list_modes_cpu.py asserts on the oracle's lists that each of them
# exercises what it is there for.  Plane: all seven non-trivial combinations, the filter at both values and both cameras.
PLANE_MODES = tuple(Mode(o, a, f) for o in (None, "top", "oblique") for a in (0, 307, 4096) for f in (False, True)
                    if (o or a or f) and not (o == "top" and f))
SURFACE_MODES = (Mode(aa=4096), Mode(fade=True), Mode(aa=307, fade=True), Mode("top"), Mode("oblique"), Mode("top", 4096), Mode("oblique", 307))
FRAMES = tuple(("plane", m) for m in PLANE_MODES) + tuple((s, m) for s in ("hmap", "sphere") for m in SURFACE_MODES)


ALL = {"plane": plane, "hmap": hmap, "sphere": sphere, "dense": dense, "wall": wall,
       **{f"twins{k}": functools.partial(twins, k) for k in range(len(TWIN_CAMERAS))}}
