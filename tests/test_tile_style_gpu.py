"""Tile-instance styles (gswt_set_tile_styles, include/gswt_hip.h) on the GPU: hide, dim and tint map cells per splat.
Frames are 72 x 40 (tests/ortho_ref.py) on the golden cases with the draws of their own perspective sort event.

The styled vertex stage bit for bit against tests/tile_style_ref.py (perspective and orthographic, with and without the pixel filter,
on the three surfaces); tint then fog against the float64 fog reference; known answers; image, depth and pick against the CPU references
over the GPU's own styled records; the same bits through graphs, frames in flight, a pair-buffer overflow, the chunk cull off,
output formats and shards; styles off leaves every output as it was; the refusals; the pipeline's world-keyed styles across a build
event."""
import ctypes as C

import numpy as np
import pytest

from gswt_renderer_amd import _lib as L
from gswt_renderer_amd import atmosphere as A
from gswt_renderer_amd import styles as ST
from gswt_renderer_amd.renderer import GSWTError
from oracle import gswt_oracle as orc
from tests import atmosphere_ref as AR
from tests import frame_modes as FM
from tests import ortho_ref as OR
from tests import pick_ref as PR
from tests import special_splats as S
from tests import tile_style_ref as TR

pytestmark = pytest.mark.gpu
W, Hh = OR.W, OR.H
F32 = np.float32
ORTHO, PERSP = L.GSWT_PROJECTION_ORTHO, L.GSWT_PROJECTION_PERSPECTIVE
AA = 307 / 1024.0
FOG = (0.15, 2.0, 0.9, (0.62, 0.71, 0.80))
MAIN = TR.entries(TR.MAIN, TR.MAIN_N)
TABLES = {"off": None, "main": TR.pack(MAIN),
          "hide_only": TR.pack(TR.entries({8: TR.HIDE, 9: TR.HIDE, 13: TR.HIDE}, TR.MAIN_N)),
          "tint_only": TR.pack(TR.entries({14: TR.entry((0, 255, 64), 160), 19: TR.entry((255, 64, 0), 160), 24: TR.entry((10, 20, 250), 255)}, TR.MAIN_N))}
# the surfaces' own cells: in each, one member of a merged draw is hidden and the other tinted, one member of another is dimmed
SURFACE_TABLES = {"case_hmap": ({9: TR.HIDE, 14: TR.entry((20, 200, 90), 180), 13: TR.entry(dim=100), 19: TR.entry((250, 30, 30), 255, 40)}, 20),
                  "case_sphere": ({27: TR.HIDE, 31: TR.entry((20, 200, 90), 180), 25: TR.entry(dim=77), 26: TR.entry((250, 30, 30), 255, 40),
                                   30: TR.HIDE, 3: TR.entry((0, 0, 255), 90)}, 32)}


@pytest.fixture(autouse=True)
def _defaults(renderer):
    yield
    FM.restore_defaults(renderer)


def _varyings(renderer, cu, su, projection, table, antialias=0.0, atmosphere=A.OFF):
    return FM.varyings(renderer, cu, su, projection=projection, antialias=antialias, atmosphere=atmosphere, tile_styles=table if table is not None else b"")


def _view(name, cam, splat_scale=OR.SPLAT_SCALE):
    """FM.view with the per-instance cell ids in the place of the reference records."""
    g, cu, su, proj, _ = FM.view(name, cam, splat_scale)
    return g, cu, su, proj, PR.identities(g["draws"])[0]


def _check_records(got, tm, base, sty, label):
    """The styled records `got` against the reference over the unstyled records `base`: visibility, geometry, alpha and colour bits."""
    want_vis, want_rgba = TR.apply(base["rgba"], base["visible"], sty)
    assert np.array_equal(got["visible"] == 1, want_vis), label
    assert tm["n_visible"] == int(want_vis.sum()), label
    for fld in ("ndc", "depth", "major", "minor"):
        assert FM.bits_equal(np.ascontiguousarray(got[fld][want_vis]), np.ascontiguousarray(base[fld][want_vis])), (label, fld)
    assert FM.bits_equal(np.ascontiguousarray(got["rgba"][want_vis]), np.ascontiguousarray(want_rgba[want_vis])), label
    neutral = want_vis & TR.classes(sty)[3]
    for fld in ("ndc", "depth", "major", "minor", "rgba"):
        assert FM.bits_equal(np.ascontiguousarray(got[fld][neutral]), np.ascontiguousarray(base[fld][neutral])), (label, fld, "neutral")
    return want_vis


# ---- 1. records, bit for bit ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("aa", [0.0, AA], ids=["plain", "antialias"])
@pytest.mark.parametrize("cam", ["persp", "oblique"])
def test_records_are_bit_exact_on_the_plain_surface(renderer, cam, aa):
    g, cu, su, proj, ids = _view("case_plane", cam)
    FM.bind(renderer, g)
    sty = TR.lookup(MAIN, ids)
    base, tm0 = _varyings(renderer, cu, su, proj, None, aa)
    if aa == 0.0:                               # the unstyled records are the oracle's / the orthographic restatement's, bit for bit
        ref = orc.project_draws(orc.Camera176.from_buffer_copy(bytes(cu)), su, g["pp"].tex, g["draws"], height_map=g["hm"]) if cam == "persp" \
            else OR.plane_records(cam)[2]
        assert np.array_equal(base["visible"], ref["visible"])
        for fld in ("ndc", "depth", "major", "minor", "rgba"):
            assert FM.bits_equal(np.ascontiguousarray(base[fld][ref["visible"] == 1]), np.ascontiguousarray(ref[fld][ref["visible"] == 1])), fld
    got, tm = _varyings(renderer, cu, su, proj, TABLES["main"], aa)
    assert got.shape == base.shape == (510,)
    vis0 = base["visible"] == 1
    hidden, dimmed, tinted, neutral = TR.classes(sty)
    counts = (int(vis0.sum()), int((vis0 & hidden).sum()), int((vis0 & dimmed).sum()), int((vis0 & tinted).sum()), int((vis0 & neutral).sum()))
    print(f"{cam} aa={aa:.3f}: visible, hidden, dimmed only, tinted, neutral = {counts}")
    if aa == 0.0:
        assert counts == ((189, 42, 27, 45, 75) if cam == "persp" else (367, 59, 27, 45, 236))
    assert min(counts) > 0
    want_vis = _check_records(got, tm, base, sty, (cam, aa))
    m = want_vis & tinted
    changed = (AR.bytes_of(got["rgba"][m]) != AR.bytes_of(base["rgba"][m])).mean()
    assert changed >= 0.98, changed
    c24 = want_vis & (ids == 24)
    assert c24.sum() > 0 and (AR.bytes_of(got["rgba"][c24]) == np.array([10.0, 20.0, 250.0])).all()
    dm = want_vis & (dimmed | (ids == 14)) & (base["rgba"][:, 3] > 0)
    assert dm.sum() > 20 and (got["rgba"][dm][:, 3] < base["rgba"][dm][:, 3]).all()
    assert tm["n_pairs"] < tm0["n_pairs"]


# ---- 2. the surfaces (FULL instantiations) ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["case_hmap", "case_sphere"])
def test_records_on_the_surfaces(renderer, name):
    g, cu, su, proj, ids = _view(name, "persp")
    FM.bind(renderer, g)
    cells, n = SURFACE_TABLES[name]
    e = TR.entries(cells, n)
    sty = TR.lookup(e, ids)
    merged = [sorted(set(np.asarray(d.map_id).tolist())) for d in g["draws"] if d.tile.single_draw == 1]
    assert any(len(m) == 2 and cells.get(m[0]) != cells.get(m[1]) and m[0] in cells and m[1] in cells for m in merged)
    base, _ = _varyings(renderer, cu, su, proj, None)
    got, tm = _varyings(renderer, cu, su, proj, TR.pack(e))
    vis0 = base["visible"] == 1
    hidden, dimmed, tinted, neutral = TR.classes(sty)
    counts = tuple(int((vis0 & c).sum()) for c in (hidden, dimmed, tinted, neutral))
    print(f"{name}: {int(vis0.sum())} visible; hidden, dimmed only, tinted, neutral = {counts}")
    assert min(counts) > 0
    _check_records(got, tm, base, sty, name)


# ---- 3. tint, then fog ------------------------------------------------------------------------------------------------------------------
def test_tint_then_fog(renderer):
    g, cu, su, proj, ids = _view("case_plane", "persp")
    FM.bind(renderer, g)
    atm = A.Atmosphere(fog=FOG)
    sty = TR.lookup(MAIN, ids)
    base, _ = _varyings(renderer, cu, su, proj, None)
    got, tm = _varyings(renderer, cu, su, proj, TABLES["main"], atmosphere=atm)
    keep = (base["visible"] == 1) & ~TR.classes(sty)[0]
    assert np.array_equal(got["visible"] == 1, keep) and tm["n_visible"] == int(keep.sum()) == 147
    for fld in ("ndc", "depth", "major", "minor"):
        assert FM.bits_equal(np.ascontiguousarray(got[fld][keep]), np.ascontiguousarray(base[fld][keep])), fld
    # alpha: the dim-only reference, nothing else
    assert FM.bits_equal(got["rgba"][keep][:, 3].copy(), TR.dimmed_alpha(base["rgba"][:, 3], sty)[keep].copy())
    dist = AR.dist_f32(orc.Camera176.from_buffer_copy(bytes(cu)).cam_pos, su, g["pp"].tex, g["draws"]).astype(np.float64)[keep]
    ct = TR.tinted_rgb(base["rgba"][:, :3], sty)[keep]
    want, near_half = AR.fog_bytes(AR.fog_codes_f64(ct, dist, AR.params(atm)))
    codes = got["rgba"][keep][:, :3].astype(np.float64) * 255.0
    have = np.rint(codes)
    assert np.abs(codes - have).max() < 1e-4
    print(f"tint then fog: {int(keep.sum())} splats, {int(near_half.sum())} channels inside the margin, {int((have != want).sum())} bytes off the float64 rint")
    assert near_half.mean() <= AR.MAX_MASKED
    assert np.abs(have - want).max() <= 1.0
    assert np.array_equal(have[~near_half], want[~near_half])
    # ... and it is neither the fog alone nor the tint alone
    fog_only, _ = _varyings(renderer, cu, su, proj, None, atmosphere=atm)
    tinted = keep & TR.classes(sty)[2]
    assert (AR.bytes_of(got["rgba"][tinted]) != AR.bytes_of(fog_only["rgba"][tinted])).mean() > 0.5


# ---- 4. known answers ---------------------------------------------------------------------------------------------------------------------
def test_known_answers(renderer):
    """Three one-splat draws, map_index 3, 4 and 5, opaque, colour (200, 100, 50)."""
    from gswt_renderer_amd import host
    pos = [(3.0, 4.0, 0.0), (4.5, 6.0, 0.0), (0.0, 2.5, 0.0)]
    halves = S.diag_halves((0.03, 0.03, 0.06))
    rows = [(p, halves, (200, 100, 50, 255)) for p in pos]
    scene = S.raw_scene(rows, lists=[(np.array([k]), np.zeros(1)) for k in range(3)])
    pd = []
    for k in range(3):
        pd += scene.draws(view=k, map_index=3 + k)[1]
    renderer.configure(None)
    scene.upload(renderer)
    renderer.set_draws(pd)
    su = orc.scene_uniforms(num_lod=1)
    cu = host.camera_uniforms((0.0, 0.0, 0.0), (2.0, 4.0, 0.0), (0, 0, 1), 45.0, 0.1, 2400.0, W, Hh)[0]
    base, tm = _varyings(renderer, cu, su, PERSP, None)
    assert list(base["visible"]) == [1, 1, 1] and tm["n_visible"] == 3 and (base["rgba"][:, 3] == 1.0).all()
    assert (AR.bytes_of(base["rgba"]) == np.array([200.0, 100.0, 50.0])).all()
    table = TR.pack(TR.entries({3: TR.HIDE, 4: TR.entry(dim=128)}, 6))
    got, tm = _varyings(renderer, cu, su, PERSP, table)
    assert list(got["visible"]) == [0, 1, 1] and tm["n_visible"] == 2
    assert got["rgba"][1, 3] == (F32(127) / F32(255)) * base["rgba"][1, 3]
    assert FM.bits_equal(got["rgba"][1, :3].copy(), base["rgba"][1, :3].copy())
    for fld in ("ndc", "depth", "major", "minor", "rgba"):
        assert FM.bits_equal(np.ascontiguousarray(got[fld][2]), np.ascontiguousarray(base[fld][2])), fld
    got, tm = _varyings(renderer, cu, su, PERSP, TR.pack(TR.entries({5: TR.entry((10, 20, 250), 255)}, 6)))
    assert tm["n_visible"] == 3 and (AR.bytes_of(got["rgba"][2:3]) == np.array([10.0, 20.0, 250.0])).all()
    assert FM.bits_equal(got["rgba"][:, 3].copy(), base["rgba"][:, 3].copy()) and FM.bits_equal(got["rgba"][:2].copy(), base["rgba"][:2].copy())
    # a table of length 4 does not reach cells 4 and 5
    got, tm = _varyings(renderer, cu, su, PERSP, TR.pack(TR.entries({3: TR.HIDE}, 6))[:32])
    assert list(got["visible"]) == [0, 1, 1] and tm["n_visible"] == 2
    short = TR.pack(TR.entries({3: TR.HIDE, 4: TR.entry(dim=128), 5: TR.entry((10, 20, 250), 255)}, 6))[:32]
    got, tm = _varyings(renderer, cu, su, PERSP, short)
    assert list(got["visible"]) == [0, 1, 1]
    for fld in ("ndc", "depth", "major", "minor", "rgba"):
        assert FM.bits_equal(np.ascontiguousarray(got[fld][1:]), np.ascontiguousarray(base[fld][1:])), fld


# ---- 5. image, depth and pick over the GPU's own styled records ---------------------------------------------------------------------------
def _image_case(renderer, cam, order_mode, bg, splat_scale):
    c = FM.image_case(renderer, cam, order_mode, bg, splat_scale, dict(antialias=0.0, atmosphere=A.OFF, tile_styles=TABLES["main"]), "styles")
    t, pick = c["t"], c["pick"]
    hit = pick["weight"] > 0
    assert hit.mean() > 0.3 and not np.isin(pick["map_index"][hit], [8, 9]).any()
    off = c["again"](tile_styles=b"", depth=True, pick=True)
    assert not FM.same(c["img"], off[0]) and renderer.timings()["n_pairs"] > t["n_pairs"] > 0
    assert np.isin(off[2]["map_index"][off[2]["weight"] > 0], [8, 9]).any()           # (the hidden cells are on screen without the table)
    return t


@pytest.mark.parametrize("bg", [False, True], ids=["clear", "bg"])
@pytest.mark.parametrize("order_mode", [0, 1], ids=["reference", "depth"])
def test_image_depth_and_pick_match_the_references(renderer, order_mode, bg):
    _image_case(renderer, "persp", order_mode, bg, OR.SPLAT_SCALE)


def test_image_depth_and_pick_with_several_segments_per_tile(renderer):
    renderer.set_option(L.GSWT_OPT_SEGMENT, 256)
    t = _image_case(renderer, "oblique", L.GSWT_ORDER_DEPTH, True, OR.SPLAT_SCALE_DENSE)
    lens = renderer.read_ranges().astype(np.int64)
    assert ((lens[:, 1] - lens[:, 0]) > 256).sum() >= 1 and t["n_pairs"] > 256


# ---- 6. the same bits every way -------------------------------------------------------------------------------------------------------------
def _styles_arg(name):
    return TABLES[name] if TABLES[name] is not None else b""


def _set_table(renderer, name):
    renderer.set_tile_styles(_styles_arg(name))


MODE = FM.Mode({name: (None, dict(tile_styles=_styles_arg(name))) for name in TABLES}, _set_table, on="main")


@pytest.fixture()
def plain(renderer):
    """The plane case bound under its perspective camera, depth order over a background, and the plain synchronous frames (colour,
    depth, pick) under each table of TABLES."""
    g, cu, su, proj, _ = _view("case_plane", "persp")
    s = FM.plain_frames(renderer, MODE, g, su, cu)
    renderer.set_tile_styles(None)
    pairs = s["pairs"]
    assert len({bytes(np.ascontiguousarray(f[0])) for f in s["frames"].values()}) == len(TABLES)
    assert pairs["tint_only"] == pairs["off"] and pairs["main"] < pairs["off"] and pairs["hide_only"] < pairs["off"]
    return s


def test_graph_replay_with_alternating_tables(renderer, plain):
    seq1 = ["off", "main", "hide_only", "main", "off", "tint_only"]
    seq2 = ["main", "off", "tint_only", "hide_only", "off", "main"]
    _, rebuilds, _ = FM.check_graph_replay(renderer, plain, MODE, seq1, seq2)
    assert rebuilds >= 4                                   # on <-> off is another k_project instantiation: the slot's graph is rebuilt


def test_async_frames_in_flight_keep_their_table(renderer, plain):
    assert renderer.frame_slots() >= 4
    seq = ["main", "off", "tint_only", "hide_only"]          # four frames in flight, each with a table of its own
    FM.check_in_flight(renderer, plain, MODE, seq, waves=4, then="tint_only")
    seq = ["hide_only", "main", "main", "tint_only"]
    FM.check_in_flight(renderer, plain, MODE, seq, waves=4, then="off", what="async, then off")


@pytest.mark.parametrize("opt", [L.GSWT_OPT_NO_CHUNK_CULL], ids=["no_chunk_cull"])
def test_compositor_and_cull_variants(renderer, plain, opt):
    FM.check_with_option_on(renderer, plain, MODE, opt, [MODE.on])


def test_pair_buffer_overflow_rerun_keeps_the_table(renderer, plain):
    FM.check_overflow_rerun(renderer, plain, MODE, MODE.on, then="hide_only")


def test_output_formats(renderer, plain):
    FM.check_output_formats(renderer, plain, MODE, [MODE.on])


@pytest.mark.parametrize("n", [2, 3])
def test_row_shards_tile_the_frame(renderer, plain, n):
    FM.check_row_shards(renderer, plain, MODE, n, [MODE.on])


@pytest.mark.parametrize("n", [2, 3, 5])
def test_column_bands_unite_to_the_frame(renderer, plain, n):
    FM.check_column_bands(renderer, plain, MODE, n, [MODE.on])


# ---- 7. off is untouched ----------------------------------------------------------------------------------------------------------------------
def _null_table(r):
    r.set_tile_styles(TABLES["main"])
    r.set_tile_styles(None)
    return {}


def test_off_is_untouched():
    """A context on which no table was ever set; then NULL, an all-neutral table, and a table that is on (one hidden cell) but too short
    to reach any drawn cell, so that the STY instantiation runs: byte-identical colour, depth, pick and counts every time, and the vertex
    stage is still the oracle's, bit for bit."""
    n_short = int(_view("case_plane", "persp")[4].min())
    assert n_short >= 1
    neutral = TR.pack(TR.entries({3: TR.entry((9, 9, 9), 0, 0)}, TR.MAIN_N))           # a tint colour without strength is neutral
    short = TR.pack(TR.entries({0: TR.HIDE}, n_short))
    FM.check_off_is_untouched("persp", dict(tile_styles=TABLES["main"]), [("NULL", _null_table), ("all neutral", lambda r: dict(tile_styles=neutral)),
                                                                        ("too short", lambda r: dict(tile_styles=short))])


# ---- 8. refusals --------------------------------------------------------------------------------------------------------------------------------
def test_refused_tables_leave_the_table_in_force(renderer, plain):
    lib, h = renderer._lib, renderer._h
    renderer.set_tile_styles(TABLES["main"])
    one = (C.c_char * 8).from_buffer_copy(ST.HIDE.pack())
    assert lib.gswt_set_tile_styles(h, None, 3) == L.GSWT_ERR_BAD_ARG and b"NULL" in lib.gswt_last_error(h)
    big = np.zeros(((1 << 20) + 1, 8), np.uint8)
    big[5, 4] = 255
    assert lib.gswt_set_tile_styles(h, big.ctypes.data_as(C.c_void_p), big.shape[0]) == L.GSWT_ERR_BAD_ARG and b"1 << 20" in lib.gswt_last_error(h)
    for k in (5, 6, 7):
        bad = np.frombuffer(TABLES["main"], np.uint8).reshape(-1, 8).copy()
        bad[17, k] = 1
        assert lib.gswt_set_tile_styles(h, bad.ctypes.data_as(C.c_void_p), bad.shape[0]) == L.GSWT_ERR_BAD_ARG, k
        assert b"styles[17]" in lib.gswt_last_error(h) and b"_pad" in lib.gswt_last_error(h)
    with pytest.raises(GSWTError):
        renderer.set_tile_styles(bytes([0, 0, 0, 0, 9, 0, 0, 1]))
    with pytest.raises(ValueError):
        renderer.set_tile_styles(b"\0" * 12)
    got = renderer.render(plain["cu"], plain["su"], W, Hh, depth=True, pick=True, **plain["kw"])
    FM.assert_frames([got], ["main"], plain, "after refused tables")
    # the largest table is accepted; a table and n_styles = 0 switches styles off
    assert lib.gswt_set_tile_styles(h, big.ctypes.data_as(C.c_void_p), 1 << 20) == L.GSWT_OK
    got = renderer.render(plain["cu"], plain["su"], W, Hh, depth=True, pick=True, **plain["kw"])
    FM.assert_frames([got], ["off"], plain, "a hidden cell no draw names")
    renderer.set_tile_styles(TABLES["main"])
    assert lib.gswt_set_tile_styles(h, one, 0) == L.GSWT_OK
    got = renderer.render(plain["cu"], plain["su"], W, Hh, depth=True, pick=True, **plain["kw"])
    FM.assert_frames([got], ["off"], plain, "after n_styles = 0")


def test_sequence_v2_is_refused_at_submit(renderer, plain):
    FM.check_v2_refused_at_submit(renderer, plain, MODE, ("main",), (b"GSWT_OPT_STRICT_VS", b"gswt_set_tile_styles"))


# ---- 9. through the frame harness: world-keyed styles across a build event ---------------------------------------------------------------------
def test_pipeline_keeps_a_world_cell_styled_across_a_build_event(renderer):
    from gswt_renderer_amd import host, synth
    from gswt_renderer_amd.pipeline import GSWTPipeline
    cfg = dict(tile_map_half_wh=(3, 3), surface_type=0, lod_max_dist=20.0, tile_sort_type=3, merge_type=2)
    pipe = GSWTPipeline(synth.make_tileset(n_lod=3, n_tile=16, lod0_count=800), host.user_data(**cfg), renderer=renderer)

    def window():
        su = pipe.wang.scene_uniforms()
        return tuple(su.center_coord), tuple(su.map_half_wh), int(su.surface_type), float(su.tile_width)

    def visit(pos):
        """A frame's worker half at `pos`; every comparison below is between frames of one visit (no update in between)."""
        cu, vp = host.camera_uniforms(pos, (pos[0] + 0.8, pos[1] + 2.0, pos[2] - 0.5), (0, 0, 1), 45.0, 0.1, 2400.0, W, Hh)
        return cu, pipe.update(pos, vp)

    def owners(pick, win):
        hit = pick["weight"] > 0
        ids, n = np.unique(pick["map_index"][hit], return_counts=True)
        return {ST.cell_of(int(i), win[0], win[1], win[2]): int(c) for i, c in zip(ids, n)}

    pos1 = (4.2, 1.0, 2.0)
    cu1, _ = visit(pos1)
    win1 = window()
    assert len(pipe.sort.groups) > 0                                                   # merged groups are in the draw list
    own1 = owners(pipe.render(cu1, W, Hh, pick=True)[1], win1)
    pos2 = (pos1[0] + win1[3], pos1[1], pos1[2])                                       # one tile over: a build event
    cu2, swapped = visit(pos2)
    win2 = window()
    assert swapped and win2[0] != win1[0]
    off2, pick2 = pipe.render(cu2, W, Hh, pick=True)
    own2 = owners(pick2, win2)
    cell = max(set(own1) & set(own2), key=lambda c: min(own1[c], own2[c]))
    i1, i2 = ST.index_of(cell, *win1[:3]), ST.index_of(cell, *win2[:3])
    assert i1 is not None and i2 is not None and i1 != i2 and min(own1[cell], own2[cell]) > 0
    # hidden through the pipeline: no pixel picks it, and the frame differs
    pipe.set_tile_styles(ST.TileStyles({cell: ST.HIDE}))
    on2, pk = pipe.render(cu2, W, Hh, pick=True)
    assert not FM.same(on2, off2) and cell not in owners(pk, win2) and (pk["weight"] > 0).any()
    # the camera goes back one tile: another build event, the map index of the cell changes, the cell stays hidden
    cu1, swapped = visit(pos1)
    assert swapped and window()[0] == win1[0]
    on1, pk = pipe.render(cu1, W, Hh, pick=True)
    assert cell not in owners(pk, win1) and (pk["weight"] > 0).any()
    # with None the frame is the unstyled one again, and the cell is back
    pipe.set_tile_styles(None)
    off1, pk = pipe.render(cu1, W, Hh, pick=True)
    assert cell in owners(pk, win1) and not FM.same(on1, off1)
    assert FM.same(renderer.render(cu1, pipe.wang.scene_uniforms(), W, Hh, tile_styles=ST.TileStyles({cell: ST.HIDE}).table(*win1[:3])), on1)
    assert FM.same(pipe.render(cu1, W, Hh, tile_styles=b""), off1)
