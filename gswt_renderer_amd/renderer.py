"""Host-side mirror of the reference's ``renderer::GSWTRenderer`` over the C ABI.

``GSWTRenderer.new / configure / render`` keep the reference's names and argument
meaning (renderer.rs:31,351,407); device work is done by libgswt_hip.so.  There is no
CPU fallback: constructing a renderer without the HIP library or a GPU raises.
"""
from __future__ import annotations

import contextlib
import ctypes as C

import numpy as np

from . import _lib as L
from . import clip as _clip


# one record of the pick image (gswt_pick, include/gswt_hip.h): the splat with the largest blend weight at the pixel.  entry is the list
# word gs_index | lod_id << 28; a pixel no splat covers has map_index = entry = PICK_NONE, weight 0 and the background depth.
PICK_DTYPE = np.dtype([("map_index", "<u4"), ("entry", "<u4"), ("depth", "<f4"), ("weight", "<f4")])
PICK_NONE = L.PICK_NONE
assert PICK_DTYPE.itemsize == C.sizeof(L.Pick)


class GSWTError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"gswt error {code}: {msg}")
        self.code = code


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def _shard_mode(mode) -> int:
    """"cols", "columns" or GSWT_SHARD_COLUMNS -> contiguous tile-column bands; anything else -> interleaved tile rows."""
    return L.GSWT_SHARD_COLUMNS if mode in ("cols", "columns", L.GSWT_SHARD_COLUMNS) and mode != 0 else L.GSWT_SHARD_ROWS


def _shard_args(shard):
    """shard = (index, count) -> interleaved tile rows; (index, count, "cols") -> contiguous tile-column bands."""
    return int(shard[0]), int(shard[1]), _shard_mode(shard[2]) if len(shard) > 2 else L.GSWT_SHARD_ROWS


def _frame_blocks(camera, scene, culling_dist, lod_enable_mask, order_mode, transmittance_eps, shard, out_format):
    """(camera block, scene block, RenderConfig) of a frame, as the gswt_render* entry points take them."""
    cam = (C.c_char * 176).from_buffer_copy(bytes(camera))
    sc = (C.c_char * 160).from_buffer_copy(bytes(scene))
    cfg = L.RenderConfig()
    cfg.culling_dist, cfg.lod_enable_mask, cfg.order_mode = culling_dist, lod_enable_mask & 0xFFFFFFFF, order_mode
    cfg.transmittance_eps = transmittance_eps
    cfg.shard_index, cfg.shard_count, cfg.shard_mode = _shard_args(shard)
    cfg.out_format = out_format & 0xFFFFFFFF
    return cam, sc, cfg


def _out_dtype(out_format: int):
    """numpy dtype of one channel of an image in out_format (GSWT_OUT_*)."""
    if out_format in (L.GSWT_OUT_RGBA8_UNORM, L.GSWT_OUT_BGRA8_UNORM):
        return np.uint8
    return np.float32          # (an unknown format is refused by the library, GSWT_ERR_BAD_ARG, before anything is written)


def video_planes(buf: np.ndarray, out_format: int, rows: int, out_w: int):
    """The planes of a GSWT_VIDEO_* image of rows x out_w pixels held in the flat uint8 array buf (views, no copy):
    (y, cbcr) with shapes [rows, out_w], [rows / 2, out_w / 2, 2] for NV12, (y, cb, cr) with [rows / 2, out_w / 2] chroma for I420."""
    n, hr, hw = rows * out_w, rows // 2, out_w // 2
    y = buf[:n].reshape(rows, out_w)
    if out_format == L.GSWT_VIDEO_NV12:
        return y, buf[n:n + 2 * hr * hw].reshape(hr, hw, 2)
    return y, buf[n:n + hr * hw].reshape(hr, hw), buf[n + hr * hw:n + 2 * hr * hw].reshape(hr, hw)


def make_draw(tile: L.TileUniforms, *, base=None, merged_range=None, merged_has_lod=False, corners=None,
              lod=None) -> L.Draw:
    """One draw of the loop renderer.rs:466-591.  base = (lod, tile, view) of a static list or
    merged_range = (offset, count) into the merged arrays."""
    d = L.Draw()
    d.tile = tile
    if merged_range is not None:
        d.merged = 1
        d.merged_offset, d.merged_count = int(merged_range[0]), int(merged_range[1])
        d.merged_has_lod = 1 if merged_has_lod else 0
    else:
        d.merged = 0
        d.base_lod, d.base_tile, d.base_view = int(base[0]), int(base[1]), int(base[2])
    if corners is not None:
        d.cull_enable = 1
        d.corners[:] = [float(x) for x in np.asarray(corners, dtype=np.float32).reshape(12)]
    d.lod = int(tile.tile_id[0] if lod is None else lod)
    return d


class GSWTRenderer:
    """renderer.rs:10-29.  Owns the device context and all HBM buffers."""

    def __init__(self, device_id: int = 0):
        self._lib = L.load()
        h = C.c_void_p()
        rc = self._lib.gswt_create(device_id, C.byref(h))
        if rc != L.GSWT_OK:
            raise GSWTError(rc, "gswt_create failed (no HIP device?)")
        self._h = h
        self.n_lists = (0, 0, 0)
        self._options = dict(L.OPTION_DEFAULTS)      # the value last set through set_option, per plain option

    # -- lifecycle ---------------------------------------------------------------
    def close(self):
        if getattr(self, "_h", None):
            self._lib.gswt_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc: int):
        if rc != L.GSWT_OK:
            raise GSWTError(rc, self._lib.gswt_last_error(self._h).decode())

    def set_option(self, key: int, value: int):
        self._check(self._lib.gswt_set_option(self._h, key, value))
        if key in self._options:
            self._options[key] = value

    @contextlib.contextmanager
    def options(self, **by_name):
        """``with r.options(GRAPH=1, TIMING=0):`` sets the named plain options (GSWT_OPT_<name>, the keys of _lib.OPTION_DEFAULTS) in
        the order given and on the way out, also when the body raises, puts back in reverse order what set_option had last set when
        the block was entered: blocks nest.  An unknown name raises KeyError before anything is set.  The body may call set_option on
        the same keys (GSWT_OPT_PAIR_CAP clears itself inside the library once a frame overflows it); the exit restores all the same."""
        keys = [getattr(L, "GSWT_OPT_" + name, None) for name in by_name]
        for name, key in zip(by_name, keys):
            if key not in L.OPTION_DEFAULTS:
                raise KeyError(name)
        before = [self._options[key] for key in keys]
        try:
            for key, value in zip(keys, by_name.values()):
                self.set_option(key, value)
            yield self
        finally:
            for key, value in zip(reversed(keys), reversed(before)):
                self.set_option(key, value)

    def set_atmosphere(self, a):
        """gswt_set_atmosphere: a is an atmosphere.Atmosphere (or 32 bytes of that layout); atmosphere.OFF or None switches the far
        fade and the fog off.  Read by the frames submitted and the proxy passes called afterwards."""
        if a is None:
            self._check(self._lib.gswt_set_atmosphere(self._h, None))
            return
        blk = (C.c_char * 32).from_buffer_copy(bytes(a))
        self._check(self._lib.gswt_set_atmosphere(self._h, blk))

    def set_tile_styles(self, table):
        """gswt_set_tile_styles: table is the packed table of a styles.TileStyles (``.table(...)``), bytes of 8-byte gswt_tile_style
        entries indexed by map cell, or a sequence of styles.TileStyle; None, empty or all neutral switches styles off.  The library
        copies it inside the call; the frames submitted afterwards use it, frames in flight keep theirs."""
        if table is None:
            self._check(self._lib.gswt_set_tile_styles(self._h, None, 0))
            return
        if not isinstance(table, (bytes, bytearray, memoryview)):
            table = b"".join(bytes(e) for e in table)
        raw = bytes(table)
        if len(raw) % 8:
            raise ValueError("set_tile_styles: the table is a whole number of 8-byte entries")
        if not raw:
            self._check(self._lib.gswt_set_tile_styles(self._h, None, 0))
            return
        buf = (C.c_char * len(raw)).from_buffer_copy(raw)
        self._check(self._lib.gswt_set_tile_styles(self._h, buf, len(raw) // 8))

    def set_shadow_map(self, m):
        """gswt_set_shadow_map: m is a shadows.ShadowMap (shadows.from_ortho_camera makes one from the light's orthographic frame);
        shadows.OFF or None switches shadows off.  The library copies the image inside the call (a device image on the context's
        stream); the frames submitted and the proxy passes called afterwards use it, frames in flight keep theirs."""
        if m is None or m.is_off:
            self._check(self._lib.gswt_set_shadow_map(self._h, None, None, 0, 0, 0))
            return
        blk = (C.c_char * 96).from_buffer_copy(bytes(m))
        self._check(self._lib.gswt_set_shadow_map(self._h, blk, C.c_void_p(m.depth_ptr()), m.width, m.height, 1 if m.on_device else 0))

    def set_clip_volumes(self, volumes):
        """gswt_set_clip_volumes: volumes is a sequence of clip.ClipVolume (at most clip.MAX_VOLUMES) or the bytes of clip.pack;
        None or empty switches the mode off.  The set travels by value: the frames submitted and the proxy passes called afterwards
        use it, frames in flight keep theirs, and nothing is waited for."""
        if volumes is None:
            self._check(self._lib.gswt_set_clip_volumes(self._h, None, 0))
            return
        raw = bytes(volumes) if isinstance(volumes, (bytes, bytearray, memoryview)) else _clip.pack(volumes)
        if len(raw) % _clip.VOLUME_BYTES:
            raise ValueError("set_clip_volumes: the array is a whole number of 64-byte gswt_clip_volume records")
        if not raw:
            self._check(self._lib.gswt_set_clip_volumes(self._h, None, 0))
            return
        buf = (C.c_char * len(raw)).from_buffer_copy(raw)
        self._check(self._lib.gswt_set_clip_volumes(self._h, buf, len(raw) // _clip.VOLUME_BYTES))

    def set_stream(self, hip_stream: int):
        self._check(self._lib.gswt_set_stream(self._h, C.c_void_p(hip_stream)))

    # -- GSWTRenderer::new (renderer.rs:31): PreloadData upload ------------------------
    def upload_scene(self, tex_data: np.ndarray, gs_index, gs_lod_id):
        """tex_data [U, 8] u32 (Scene.tex_data); gs_index / gs_lod_id nested [lod][tile][view]."""
        tex = np.ascontiguousarray(tex_data, dtype=np.uint32).reshape(-1, 8)
        n_lod, n_tile, n_view = len(gs_index), len(gs_index[0]), len(gs_index[0][0])
        arr = (L.BaseList * (n_lod * n_tile * n_view))()
        keep = []
        i = 0
        for l in range(n_lod):
            for t in range(n_tile):
                for v in range(n_view):
                    gi = np.ascontiguousarray(gs_index[l][t][v], dtype=np.uint32)
                    li = np.ascontiguousarray(gs_lod_id[l][t][v], dtype=np.uint32)
                    keep += [gi, li]
                    arr[i].gs_index, arr[i].gs_lod_id, arr[i].splat_count = gi.ctypes.data, li.ctypes.data, gi.shape[0]
                    i += 1
        self._check(self._lib.gswt_upload_scene(self._h, _ptr(tex), tex.shape[0], arr, n_lod, n_tile, n_view))
        self.n_lists = (n_lod, n_tile, n_view)

    def upload_scene_rows(self, wang):
        """GSWTRenderer::new from a rows-only WangTile: the texture, raw depths, base lists and static arena are built on the
        device from the normalised rows (gswt_upload_scene_rows); device-side merged lists work right after it."""
        rows, cnts, _ = wang.rows_tables()
        n_lod, n_tile, n_view = wang.n_tiles
        vp = np.ascontiguousarray(wang.presort_view_proj(), dtype=np.float32)
        self._check(self._lib.gswt_upload_scene_rows(self._h, rows, cnts, n_lod, n_tile, _ptr(vp), n_view))
        self.n_lists = (n_lod, n_tile, n_view)

    def read_scene(self, what: int) -> bytes:
        """gswt_debug_read_scene: one item of the device's scene state (L.GSWT_SCENE_*) as raw bytes."""
        n = C.c_size_t()
        self._check(self._lib.gswt_debug_read_scene(self._h, what, None, 0, C.byref(n)))
        buf = (C.c_uint8 * max(1, n.value))()
        self._check(self._lib.gswt_debug_read_scene(self._h, what, buf, n.value, C.byref(n)))
        return bytes(buf[:n.value])

    # -- GSWTRenderer::configure (renderer.rs:351) -----------------------------------
    def configure(self, height_map: np.ndarray | None):
        if height_map is None:
            self._check(self._lib.gswt_configure(self._h, None, 0, 0))
        else:
            hm = np.ascontiguousarray(height_map, dtype=np.float32)
            self._check(self._lib.gswt_configure(self._h, _ptr(hm), hm.shape[1], hm.shape[0]))

    # -- SortData swap-in (state.rs:361-376) -------------------------------------------
    def set_draws(self, draws, merged_gs_index=None, merged_map_id=None, merged_lod_id=None):
        arr = (L.Draw * max(1, len(draws)))(*draws)
        gi = np.ascontiguousarray(merged_gs_index, dtype=np.uint32) if merged_gs_index is not None else None
        mi = np.ascontiguousarray(merged_map_id, dtype=np.uint32) if merged_map_id is not None else None
        li = np.ascontiguousarray(merged_lod_id, dtype=np.uint32) if merged_lod_id is not None else None
        n = 0 if gi is None else gi.shape[0]
        self._check(self._lib.gswt_set_draws(self._h, arr, len(draws), _ptr(gi), _ptr(mi), _ptr(li), n))

    def set_draws_merge_groups(self, draws, groups_ptr, n_groups: int, members_ptr, n_members: int):
        """SortData swap-in with the merged lists built on the device (groups / members: C arrays of
        gswt_merge_group / gswt_merge_member, e.g. straight from libgswt_host's sort data)."""
        arr = (L.Draw * max(1, len(draws)))(*draws)
        self._check(self._lib.gswt_set_draws_merge_groups(self._h, arr, len(draws), groups_ptr, n_groups, members_ptr, n_members))

    def set_draws_merge_groups_raw(self, draws_arr, n_draws: int, groups_arr, n_groups: int, members_arr, n_members: int):
        """The same from C arrays (WangTile.sort_tiles_raw): no per-draw Python work on the render thread."""
        self._check(self._lib.gswt_set_draws_merge_groups(self._h, draws_arr, n_draws, groups_arr, n_groups, members_arr, n_members))

    def graph_stats(self):
        """GSWT_OPT_GRAPH bookkeeping: [frames replayed through hipGraphLaunch, graphs (re)built, kernel nodes updated]."""
        a = (C.c_ulonglong * 3)()
        self._check(self._lib.gswt_debug_graph_stats(self._h, a))
        return [int(x) for x in a]

    def merge_stats(self):
        """(merged groups sorted, merged groups copied from the previous sort event) since the ctx was created."""
        out = (C.c_ulonglong * 2)()
        self._check(self._lib.gswt_debug_merge_stats(self._h, out))
        return int(out[0]), int(out[1])

    def merge_stats_deep(self):
        """Of the copied groups, how many came from a sort event older than the previous one (the lists of the last 9 events are kept)."""
        out = C.c_ulonglong(0)
        self._check(self._lib.gswt_debug_merge_stats_deep(self._h, C.byref(out)))
        return int(out.value)

    def read_merged(self):
        n = C.c_size_t(0)
        self._check(self._lib.gswt_debug_read_merged(self._h, None, None, 0, C.byref(n)))
        a = np.zeros(max(1, n.value), dtype=np.uint32)
        b = np.zeros(max(1, n.value), dtype=np.uint32)
        self._check(self._lib.gswt_debug_read_merged(self._h, _ptr(a), _ptr(b), a.shape[0], C.byref(n)))
        return a[:n.value], b[:n.value]

    def _set_frame_modes(self, projection, antialias, atmosphere, tile_styles, shadow=None, clip_volumes=None):
        """The per-frame modes that render and render_async take as keywords: each one given is set on the context, in this order."""
        if projection is not None:
            self.set_option(L.GSWT_OPT_PROJECTION, int(projection))
        if antialias is not None:
            self.set_option(L.GSWT_OPT_ANTIALIAS, int(round(float(antialias) * 1024)))
        if atmosphere is not None:
            self.set_atmosphere(atmosphere)
        if tile_styles is not None:
            self.set_tile_styles(tile_styles)
        if shadow is not None:
            self.set_shadow_map(shadow)
        if clip_volumes is not None:
            self.set_clip_volumes(clip_volumes)

    # -- GSWTRenderer::render (renderer.rs:407) ---------------------------------------
    def render(self, camera, scene, width: int, height: int, *, culling_dist: float = 1.0,
               lod_enable_mask: int = 0xFFFFFFFF, order_mode: int = L.GSWT_ORDER_REFERENCE,
               transmittance_eps: float = 0.0, shard=(0, 1), bg_rgba=None, bg_depth=None,
               out_device_ptr: int | None = None, bg_on_device: bool = False, out_format: int = L.GSWT_OUT_RGBA32F,
               depth: bool = False, out_depth_device_ptr: int | None = None, pick: bool = False,
               out_pick_device_ptr: int | None = None, projection: int | None = None, antialias: float | None = None,
               atmosphere=None, tile_styles=None, shadow=None, clip_volumes=None):
        """camera / scene: 176 / 160-byte uniform blocks (any ctypes struct or bytes of that layout).
        Returns the image [rows, W, 4] on the host -- f32 for GSWT_OUT_RGBA32F, uint8 in the channel order of
        GSWT_OUT_RGBA8_UNORM / GSWT_OUT_BGRA8_UNORM --, or None when out_device_ptr is given.
        out_format GSWT_VIDEO_NV12 / GSWT_VIDEO_I420 (4:2:0, BT.709 limited range; width and height even): returns the planes as
        uint8 arrays instead of one image, (y, cbcr) with shapes [rows, W], [rows / 2, W / 2, 2] for NV12 and (y, cb, cr) with
        [rows / 2, W / 2] chroma planes for I420; out_device_ptr then addresses gswt_out_image_bytes(out_format, rows, W) bytes.
        With depth=True the depth image follows the planes: (y, cbcr, depth) / (y, cb, cr, depth).
        depth=True: returns (image, depth), depth the composited depth image [rows, W] f32 of gswt_render_depth (NDC depth
        blended like a colour channel over bg_depth, or 1.0 without one).  With out_device_ptr the depth goes to
        out_depth_device_ptr (rows x out_w f32 on the device) when that is given.
        pick=True: the pick image of gswt_render_pick, [rows, W] records of PICK_DTYPE (per pixel the tile instance and list word
        of the splat with the largest blend weight, its depth and that weight), follows as the last element: (image, pick),
        (image, depth, pick), or behind the planes and the depth of a video format.  With out_device_ptr it goes to
        out_pick_device_ptr (rows x out_w x 16 bytes on the device) when that is given.
        projection: when given, sets GSWT_OPT_PROJECTION first (0 perspective, 1 orthographic: `camera` is then the block of an
        ortho.OrthoCamera); omitted, the context keeps the projection it has.
        antialias: when given, sets GSWT_OPT_ANTIALIAS first: the variance of the screen-space pixel filter in px^2 (0.3 is the
        usual 3DGS constant, 0.1 Mip-Splatting's, 0 switches it off; rounded to 1/1024 px^2); omitted, the context keeps its value.
        atmosphere: when given, an atmosphere.Atmosphere set first with set_atmosphere (atmosphere.OFF switches the far fade and the
        fog off); omitted, the context keeps the block it has.
        tile_styles: when given, a table set first with set_tile_styles (b"" switches styles off); omitted, the context keeps the
        table it has.
        shadow: when given, a shadows.ShadowMap set first with set_shadow_map (shadows.OFF switches shadows off); omitted, the
        context keeps the map it has.
        clip_volumes: when given, a list of clip.ClipVolume set first with set_clip_volumes ([] switches the mode off); omitted, the
        context keeps the set it has."""
        self._set_frame_modes(projection, antialias, atmosphere, tile_styles, shadow, clip_volumes)
        cam, sc, cfg = _frame_blocks(camera, scene, culling_dist, lod_enable_mask, order_mode, transmittance_eps, shard, out_format)
        rows, out_w = height, width
        if cfg.shard_count > 1 and cfg.shard_mode == L.GSWT_SHARD_COLUMNS:
            out_w = self._lib.gswt_shard_cols_padded(width, cfg.shard_count)
        elif cfg.shard_count > 1:
            rows = self._lib.gswt_shard_rows_padded(height, cfg.shard_count)
        if bg_on_device:
            bgc = C.c_void_p(bg_rgba) if bg_rgba else None
            bgd = C.c_void_p(bg_depth) if bg_depth else None
        else:
            bgc_a = np.ascontiguousarray(bg_rgba, dtype=np.float32) if bg_rgba is not None else None
            bgd_a = np.ascontiguousarray(bg_depth, dtype=np.float32) if bg_depth is not None else None
            bgc, bgd = _ptr(bgc_a), _ptr(bgd_a)
        if out_device_ptr is not None:
            zd = C.c_void_p(out_depth_device_ptr) if out_depth_device_ptr else None
            pd = C.c_void_p(out_pick_device_ptr) if out_pick_device_ptr else None
            self._check(self._lib.gswt_render_pick(self._h, cam, sc, C.byref(cfg), width, height, bgc, bgd,
                                                   1 if bg_on_device else 0, C.c_void_p(out_device_ptr), zd, pd, 1))
            return None
        video = out_format in (L.GSWT_VIDEO_NV12, L.GSWT_VIDEO_I420)
        if video:       # (an odd size has no plane layout, 0 bytes: the library refuses the call before it writes anything)
            out = np.empty(max(int(self._lib.gswt_out_image_bytes(out_format, rows, out_w)), 16), dtype=np.uint8)
            planes = lambda: video_planes(out, out_format, rows, out_w)
        else:
            out = np.empty((rows, out_w, 4), dtype=_out_dtype(out_format))
        if depth or pick:
            z = np.empty((rows, out_w), dtype=np.float32) if depth else None
            pk = np.empty((rows, out_w), dtype=PICK_DTYPE) if pick else None
            self._check(self._lib.gswt_render_pick(self._h, cam, sc, C.byref(cfg), width, height, bgc, bgd,
                                                   1 if bg_on_device else 0, _ptr(out), _ptr(z), _ptr(pk), 0))
            extra = tuple(a for a in (z, pk) if a is not None)
            return (planes() if video else (out,)) + extra
        self._check(self._lib.gswt_render(self._h, cam, sc, C.byref(cfg), width, height, bgc, bgd,
                                          1 if bg_on_device else 0, _ptr(out), 0))
        return planes() if video else out

    def render_async(self, camera, scene, width: int, height: int, out_device_ptr: int, *, culling_dist: float = 1.0,
                     lod_enable_mask: int = 0xFFFFFFFF, order_mode: int = L.GSWT_ORDER_REFERENCE,
                     transmittance_eps: float = 0.0, shard=(0, 1), bg_rgba_ptr: int = 0, bg_depth_ptr: int = 0,
                     out_format: int = L.GSWT_OUT_RGBA32F, out_depth_ptr: int = 0, out_pick_ptr: int = 0,
                     projection: int | None = None, antialias: float | None = None, atmosphere=None,
                     tile_styles=None, shadow=None, clip_volumes=None) -> int:
        """Queues a frame (device pointers only) and returns a ticket for render_wait.  out_device_ptr holds rows x out_w x 4
        f32, or bytes for the 8-bit out_format values, or the planes of a GSWT_VIDEO_* format (gswt_out_image_bytes(out_format,
        rows, out_w) bytes, width and height even; see video_planes); out_depth_ptr (optional) receives the depth image, rows x out_w f32
        (gswt_render_async_depth); out_pick_ptr (optional) the pick image, rows x out_w records of PICK_DTYPE (gswt_render_async_pick).
        projection, antialias, atmosphere, tile_styles, shadow, clip_volumes: as in render (the frame keeps the values it was submitted with, whatever is set afterwards)."""
        self._set_frame_modes(projection, antialias, atmosphere, tile_styles, shadow, clip_volumes)
        cam, sc, cfg = _frame_blocks(camera, scene, culling_dist, lod_enable_mask, order_mode, transmittance_eps, shard, out_format)
        ticket = C.c_int(-1)
        self._check(self._lib.gswt_render_async_pick(self._h, cam, sc, C.byref(cfg), width, height,
                                                     C.c_void_p(bg_rgba_ptr) if bg_rgba_ptr else None,
                                                     C.c_void_p(bg_depth_ptr) if bg_depth_ptr else None,
                                                     C.c_void_p(out_device_ptr), C.c_void_p(out_depth_ptr) if out_depth_ptr else None,
                                                     C.c_void_p(out_pick_ptr) if out_pick_ptr else None, C.byref(ticket)))
        return ticket.value

    def frame_slots(self) -> int:
        """Frames that may be in flight at once (render_async tickets)."""
        return int(self._lib.gswt_frame_slots())

    def render_wait(self, ticket: int):
        self._check(self._lib.gswt_render_wait(self._h, ticket))

    def render_fence(self, ticket: int):
        """Device-side: work submitted to the ctx stream afterwards waits for this frame."""
        self._check(self._lib.gswt_render_fence(self._h, ticket))

    # -- background passes (state.rs:384-392) ------------------------------------------
    def skybox_configure(self, faces: np.ndarray, equirectangular: bool = False):
        """Skybox::configure (skybox.rs:341): faces [6, n, n, 4] f32, +X -X +Y -Y +Z -Z."""
        f = np.ascontiguousarray(faces, dtype=np.float32)
        assert f.ndim == 4 and f.shape[0] == 6 and f.shape[1] == f.shape[2] and f.shape[3] == 4
        self._check(self._lib.gswt_skybox_configure(self._h, _ptr(f), f.shape[1], 1 if equirectangular else 0))
        self._sky_size = f.shape[1]

    def skybox_configure_equirect(self, equi: np.ndarray, face_size: int = 2048):
        """Skybox::configure with an HDR panorama (skybox.rs:490-668): equi [h, w, 4] f32, linear, row 0 at the top, baked
        on the device into a face_size^2 x 6 cube map that is then sampled as is_equi."""
        e = np.ascontiguousarray(equi, dtype=np.float32)
        assert e.ndim == 3 and e.shape[2] == 4
        self._check(self._lib.gswt_skybox_configure_equirect(self._h, _ptr(e), e.shape[1], e.shape[0], int(face_size)))
        self._sky_size = int(face_size)

    def skybox_download(self) -> np.ndarray:
        """The current cube map, [6, n, n, 4] f32 (+X -X +Y -Y +Z -Z)."""
        n = getattr(self, "_sky_size", 0)
        out = np.empty((6, n, n, 4) if n else (1,), np.float32)       # (before any configure the call fails before writing)
        self._check(self._lib.gswt_skybox_download(self._h, _ptr(out)))
        return out

    def skybox_render(self, camera, width: int, height: int, out_device_ptr: int):
        """Skybox::render (skybox.rs:457) into a device RGBA f32 buffer."""
        cam = (C.c_char * 176).from_buffer_copy(bytes(camera))
        self._check(self._lib.gswt_skybox_render(self._h, cam, width, height, C.c_void_p(out_device_ptr)))

    def proxy_configure(self, mips, grid_dim: int = 2048):
        """Proxy::configure (proxy.rs:208): mip chain [level][n >> level, n >> level, 4] f32."""
        ms = [np.ascontiguousarray(m, dtype=np.float32) for m in mips]
        arr = (C.c_void_p * len(ms))(*[m.ctypes.data for m in ms])
        self._check(self._lib.gswt_proxy_configure(self._h, arr, ms[0].shape[0], len(ms), grid_dim))
        self._proxy_chain = (ms[0].shape[0], len(ms))

    def proxy_configure_image(self, img: np.ndarray, tex_size: int | None = None, grid_dim: int = 2048):
        """upload_proxy_texture + Proxy::configure (proxy.rs:513-554) from the decoded image: the Lanczos3 mip chain
        tex_size, tex_size / 2, ..., 1 is built on the device from img, [h, w, 4], [h, w, 3] or [h, w] uint8 or uint16 (row 0
        first).  Missing channels are expanded as image's to_rgba8 / to_rgba16 do: grey -> (g, g, g, MAX), RGB -> (r, g, b, MAX).

        tex_size defaults to the largest power of two <= w, computed exactly.  The reference computes it as
        2^floor(ln(w) / ln(2)) in f32, which at w = 8192 gives 4096 or 8192 depending on how its logf rounds; a host that
        must match it passes its own value."""
        a = np.asarray(img)
        if a.dtype not in (np.uint8, np.uint16):
            raise TypeError(f"proxy image must be uint8 or uint16, not {a.dtype}")
        if a.ndim == 2:
            a = a[..., None]
        if a.ndim != 3 or a.shape[2] not in (1, 3, 4):
            raise ValueError(f"proxy image must be [h, w], [h, w, 3] or [h, w, 4], not {tuple(np.shape(img))}")
        if a.shape[2] != 4:
            rgba = np.empty(a.shape[:2] + (4,), a.dtype)
            rgba[..., :3] = a[..., :3] if a.shape[2] == 3 else a
            rgba[..., 3] = np.iinfo(a.dtype).max
            a = rgba
        a = np.ascontiguousarray(a)
        h, w = a.shape[:2]
        n = (1 << (int(w).bit_length() - 1)) if tex_size is None else int(tex_size)
        fmt = L.GSWT_PROXY_SRC_RGBA16 if a.dtype == np.uint16 else L.GSWT_PROXY_SRC_RGBA8
        self._check(self._lib.gswt_proxy_configure_image(self._h, _ptr(a), w, h, fmt, n, int(grid_dim)))
        self._proxy_chain = (n, n.bit_length())

    def proxy_download(self) -> list:
        """The current proxy mip chain: [n >> level, n >> level, 4] f32 arrays, level 0 first."""
        n, levels = getattr(self, "_proxy_chain", (0, 0))
        sizes = [n >> l for l in range(levels)]
        flat = np.empty((sum(s * s for s in sizes), 4) if n else (1,), np.float32)   # (no proxy: the call fails before writing)
        self._check(self._lib.gswt_proxy_download(self._h, _ptr(flat)))
        out, off = [], 0
        for s in sizes:
            out.append(flat[off:off + s * s].reshape(s, s, 4))
            off += s * s
        return out

    def proxy_render(self, uniforms, width: int, height: int, rgba_device_ptr: int, depth_device_ptr: int, clear_depth: bool,
                     projection: int = 0):
        """One draw of Proxy::render (proxy.rs:366); uniforms: 224-byte proxy.wgsl Uniforms block.  projection = 1: the orthographic
        pass, gswt_proxy_render_ortho, over a block of `ortho.OrthoCamera.proxy_uniforms` (the context's GSWT_OPT_PROJECTION plays
        no part either way)."""
        if projection not in (0, 1):
            raise ValueError(f"proxy_render: projection must be 0 (perspective) or 1 (orthographic), not {projection!r}")
        u = (C.c_char * 224).from_buffer_copy(bytes(uniforms))
        fn = self._lib.gswt_proxy_render_ortho if projection == 1 else self._lib.gswt_proxy_render
        self._check(fn(self._h, u, width, height, C.c_void_p(rgba_device_ptr), C.c_void_p(depth_device_ptr), 1 if clear_depth else 0))

    def proxy_render_sphere(self, uniforms, sphere_radius: float, width: int, height: int, rgba_device_ptr: int, depth_device_ptr: int,
                            clear_depth: bool, projection: int = 0):
        """The ground under the Sphere surface (gswt_proxy_render_sphere): the sphere of radius sphere_radius + height_offset about the
        world origin, textured through the inverse of the sphere unfolding; uniforms: the 224-byte proxy block (map_proxy, width_scale,
        surface_type and height_map_scale are not read).  projection = 1: an orthographic block, as `proxy_render(..., projection=1)`."""
        if projection not in (0, 1):
            raise ValueError(f"proxy_render_sphere: projection must be 0 (perspective) or 1 (orthographic), not {projection!r}")
        u = (C.c_char * 224).from_buffer_copy(bytes(uniforms))
        self._check(self._lib.gswt_proxy_render_sphere(self._h, u, float(sphere_radius), int(projection), width, height, C.c_void_p(rgba_device_ptr),
                                                       C.c_void_p(depth_device_ptr), 1 if clear_depth else 0))

    def shard_rows_padded(self, height: int, shard_count: int) -> int:
        return int(self._lib.gswt_shard_rows_padded(height, shard_count))

    def shard_cols_padded(self, width: int, shard_count: int) -> int:
        return int(self._lib.gswt_shard_cols_padded(width, shard_count))

    def unshard_mode(self, gathered_device_ptr: int, width: int, height: int, shard_count: int, mode, out_device_ptr: int):
        self._check(self._lib.gswt_unshard_mode(self._h, C.c_void_p(gathered_device_ptr), width, height, shard_count, _shard_mode(mode),
                                                C.c_void_p(out_device_ptr)))

    def unshard_format(self, gathered_device_ptr: int, width: int, height: int, shard_count: int, mode, out_format: int,
                       out_device_ptr: int):
        """unshard_mode for any output format (GSWT_OUT_*: 16- or 4-byte pixels; GSWT_VIDEO_*: every gathered shard is a complete
        image of planes, the frame is reassembled plane by plane)."""
        self._check(self._lib.gswt_unshard_format(self._h, C.c_void_p(gathered_device_ptr), width, height, shard_count, _shard_mode(mode), out_format,
                                                  C.c_void_p(out_device_ptr)))

    def unshard(self, gathered_device_ptr: int, width: int, height: int, shard_count: int, out_device_ptr: int):
        self._check(self._lib.gswt_unshard(self._h, C.c_void_p(gathered_device_ptr), width, height, shard_count,
                                           C.c_void_p(out_device_ptr)))

    # -- multi-GPU gather behind the ABI -------------------------------------------------------
    @staticmethod
    def comm_unique_id() -> bytes:
        """Rank 0: the 128-byte RCCL id every rank passes to comm_init (ship it by any means)."""
        buf = (C.c_char * L.GSWT_COMM_ID_BYTES)()
        rc = L.load().gswt_comm_unique_id(buf)
        if rc != 0:
            raise GSWTError(rc, "gswt_comm_unique_id: RCCL is not available")
        return bytes(buf)

    def comm_init(self, unique_id: bytes, rank: int, world: int):
        self._check(self._lib.gswt_comm_init(self._h, C.c_char_p(unique_id), rank, world))

    def comm_destroy(self):
        self._check(self._lib.gswt_comm_destroy(self._h))

    def render_gather(self, ticket: int, frame_device_ptr: int):
        """Overflow-safe fence + ncclAllGather of the shard images + re-assembly, on the ctx stream."""
        self._check(self._lib.gswt_render_gather(self._h, ticket, C.c_void_p(frame_device_ptr)))

    @staticmethod
    def group_init(renderers):
        """All ranks in one process (peer copies instead of RCCL): rank r = renderers[r]."""
        arr = (C.c_void_p * len(renderers))(*[r._h for r in renderers])
        rc = L.load().gswt_group_init(arr, len(renderers))
        if rc != 0:
            raise GSWTError(rc, "gswt_group_init failed")

    @staticmethod
    def group_render_gather(renderers, tickets, frame_device_ptrs):
        n = len(renderers)
        arr = (C.c_void_p * n)(*[r._h for r in renderers])
        tk = (C.c_int * n)(*tickets)
        fr = (C.c_void_p * n)(*frame_device_ptrs)
        rc = L.load().gswt_group_render_gather(arr, tk, fr, n)
        if rc != 0:
            raise GSWTError(rc, renderers[0]._lib.gswt_last_error(renderers[0]._h).decode())

    def synchronize(self):
        self._check(self._lib.gswt_synchronize(self._h))

    def timings(self) -> dict:
        t = L.Timings()
        self._check(self._lib.gswt_last_timings(self._h, C.byref(t)))
        return {k: getattr(t, k) for k, _ in L.Timings._fields_ if not k.startswith("_pad")}

    VARYINGS_DTYPE = np.dtype([("visible", "<i4"), ("ndc", "<f4", 2), ("depth", "<f4"), ("major", "<f4", 2),
                               ("minor", "<f4", 2), ("rgba", "<f4", 4)])

    def read_projected(self) -> np.ndarray:
        n = C.c_size_t(0)
        self._check(self._lib.gswt_debug_read_projected(self._h, None, 0, C.byref(n)))
        out = np.zeros(max(1, n.value), dtype=self.VARYINGS_DTYPE)
        self._check(self._lib.gswt_debug_read_projected(self._h, _ptr(out), out.shape[0], C.byref(n)))
        return out[:n.value]

    def depth_stats(self):
        """GSWT_ORDER_DEPTH: (frames on the tile-local path, frames on the global depth passes, longest tile list of the last depth-ordered frame)."""
        a = (C.c_ulonglong * 3)()
        self._check(self._lib.gswt_debug_depth_stats(self._h, a))
        return int(a[0]), int(a[1]), int(a[2])

    def frame_times(self, ticket_ref: int, ticket: int):
        """(start, end, gather end) of slot `ticket`'s frame in ms after the start of slot `ticket_ref`'s frame (device timeline)."""
        out = (C.c_float * 3)()
        self._check(self._lib.gswt_debug_frame_times(self._h, ticket_ref, ticket, out))
        return float(out[0]), float(out[1]), float(out[2])

    def read_ranges(self) -> np.ndarray:
        """[n_tiles, 2] (start, end) of each screen tile's slice of the sorted pair list."""
        n = C.c_size_t(0)
        self._check(self._lib.gswt_debug_read_ranges(self._h, None, 0, C.byref(n)))
        out = np.zeros((max(1, n.value), 2), dtype=np.uint32)
        self._check(self._lib.gswt_debug_read_ranges(self._h, _ptr(out), out.shape[0], C.byref(n)))
        return out[:n.value]

    def read_pairs(self) -> np.ndarray:
        """The sorted pair list the last frame's compositor walked (read_ranges' slices index it): per pair its list entry in draw
        order (read_projected's index; 0xFFFFFFFF for a slot that names none).  Works without GSWT_OPT_DEBUG_VARYINGS."""
        n = C.c_size_t(0)
        self._check(self._lib.gswt_debug_read_pairs(self._h, None, 0, C.byref(n)))
        out = np.zeros(max(1, n.value), dtype=np.uint32)
        self._check(self._lib.gswt_debug_read_pairs(self._h, _ptr(out), out.shape[0], C.byref(n)))
        return out[:n.value]

    def debug_sort_ex(self, keys, vals, aux=None, *, n=None, overflow=False, key_bits=32, krange=None, n_range_keys=0, threads=0,
                      aux_form=0):
        """gswt_debug_sort_ex: the frame's radix sort as frames drive it.  keys / vals / aux: n_cap words each (copies are sorted);
        n: the device-side item count (default n_cap); krange: (min, max); n_range_keys > 0: the last pass writes the range table
        and no keys.  Returns (keys or None, vals, aux or None, ranges [n_range_keys, 2] or None), each of all n_cap words."""
        k = np.array(keys, dtype=np.uint32, copy=True)
        v = np.array(vals, dtype=np.uint32, copy=True)
        x = np.array(aux, dtype=np.uint32, copy=True) if aux is not None else None
        n_cap = k.shape[0]
        assert k.ndim == 1 and v.shape == k.shape and (x is None or x.shape == k.shape)
        rg = np.full((n_range_keys, 2), 0xDEADBEEF, dtype=np.uint32) if n_range_keys else None
        kmin, kmax = (int(krange[0]), int(krange[1])) if krange is not None else (0, 0)
        self._check(self._lib.gswt_debug_sort_ex(self._h, _ptr(k), _ptr(v), _ptr(x) if x is not None else None, n_cap,
                                                 n_cap if n is None else int(n), 1 if overflow else 0, key_bits,
                                                 1 if krange is not None else 0, kmin, kmax, _ptr(rg) if rg is not None else None,
                                                 n_range_keys, threads, aux_form))
        return (None if rg is not None else k), v, x, rg
