"""tests/test_pair_list_gpu.py's comparison -- every screen tile's slice of the sorted pair list against lists derived from the oracle alone
-- for the frames that file leaves out: orthographic (GSWT_OPT_PROJECTION = 1), anti-aliased (GSWT_OPT_ANTIALIAS) and faded
(gswt_set_atmosphere's far fade), alone and combined.  Each of the three changes what goes into the lists: the Jacobian behind every
rectangle, s on both eigenvalues (every rectangle grows, and k_cull's band bound with it), the splats discarded before the fragment setup.
The expected lists come from the oracle's strict vertex stage under oracle.frame_mode (tests/pair_list_scenes.py: framed);
tests/test_pair_list_modes_cpu.py pins those oracle lines to the numpy references and shows that every frame here exercises its path.

Every frame asserts: the lists pair by pair and their total against n_pairs, n_visible against the oracle's count, and the image within
the 1e-4 of the other file against orc.render under the same mode.  Debug-varyings frames also compare the projected records with the
oracle's bit for bit: for the filter the first such check of comp, for the HeightMap and Sphere surfaces the first of orthographic axes."""
import contextlib

import numpy as np
import pytest

from gswt_renderer_amd import _lib as L
from oracle import gswt_oracle as orc
from tests import helpers as H
from tests import pair_list_ref as PL
from tests import pair_list_scenes as S
from tests.test_pair_list_gpu import ORDERS, TOL, _check, _frame, _options

pytestmark = pytest.mark.gpu
ORTHO, PERSP = L.GSWT_PROJECTION_ORTHO, L.GSWT_PROJECTION_PERSPECTIVE
Mode = S.Mode


def _restore(renderer):
    renderer.set_option(L.GSWT_OPT_PROJECTION, PERSP)
    renderer.set_option(L.GSWT_OPT_ANTIALIAS, 0)
    renderer.set_atmosphere(None)


@pytest.fixture(autouse=True)
def _defaults(renderer):
    """No test leaves the shared context in another mode, whatever way it ends."""
    yield
    _restore(renderer)
    assert orc.frame_mode_is_default()


@contextlib.contextmanager
def _mode(renderer, sc, **opts):
    """_options(**opts) around a frame of sc's mode: yields the keyword arguments that make renderer.render set the projection, the filter
    and the atmosphere block of sc; perspective, no filter and no atmosphere afterwards."""
    if sc.ortho_args is not None:
        assert bytes(S.ortho_camera(sc).uniforms()) == bytes(sc.cam)          # the product's camera object gives the oracle's block
    try:
        with _options(renderer, **opts):
            yield dict(projection=ORTHO if sc.ortho_args is not None else PERSP, antialias=sc.mode.aa / 1024.0, atmosphere=sc.atmosphere())
    finally:
        _restore(renderer)


def _check_image(sc, order, img, t):
    ref, st = sc.render(ORDERS[order][0])
    assert t["n_visible"] == st["n_visible"]
    d = H.max_abs_diff(img, ref)
    assert d <= TOL, d


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _check_records(sc, var):
    """gswt_debug_read_projected against the oracle's records, entry by entry (the frame kept the unfiltered static lists)."""
    want, r = sc.records(), sc.rects()
    assert var.shape == want.shape
    assert np.array_equal(var["visible"], r["visible"])                       # (the product's `visible`: the fragment setup passed too)
    vis = r["visible"] == 1
    assert vis.sum() > 5000
    for fld in ("depth", "ndc", "major", "minor", "rgba"):
        assert np.array_equal(_bits(var[fld][vis]), _bits(want[fld][vis])), (sc.name, fld)


# ---- the plane scene: every combination, every order ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", list(ORDERS))
@pytest.mark.parametrize("mode", S.PLANE_MODES, ids=lambda m: m.id)
def test_plane_every_combination(renderer, mode, order):
    """The live-chunk table over the LOD-prefiltered lists."""
    sc = S.framed("plane", mode)
    want = sc.expected(ORDERS[order][0])
    with _mode(renderer, sc) as kw:
        img, got, t = _frame(renderer, sc, order, **kw)
    _check(want, got, t)
    _check_image(sc, order, img, t)


DEBUG_PLANE = (Mode("oblique", 4096, True), Mode("top", 307), Mode("top"), Mode("oblique"), Mode(aa=307), Mode(aa=4096), Mode(fade=True))
DEBUG_SURFACE = (Mode("top"), Mode("oblique"), Mode("top", 4096), Mode("oblique", 307), Mode(aa=307, fade=True))


@pytest.mark.parametrize("name,mode", [("plane", m) for m in DEBUG_PLANE] + [(s, m) for s in ("hmap", "sphere") for m in DEBUG_SURFACE],
                         ids=lambda v: v.id if isinstance(v, Mode) else v)
def test_debug_varyings_records_and_lists(renderer, name, mode):
    """GSWT_OPT_DEBUG_VARYINGS with GSWT_OPT_NO_LOD_PREFILTER: k_project<DEBUG> of the same instantiations, every chunk emitted; the
    projected records are the oracle's bit for bit -- `visible`, depth, ndc, both axes, colour and alpha (comp and the fade's factor in it)."""
    sc = S.framed(name, mode)
    order = "depth-local"
    want = sc.expected(ORDERS[order][0])
    with _mode(renderer, sc, DEBUG_VARYINGS=1, NO_LOD_PREFILTER=1) as kw:
        img, got, t = _frame(renderer, sc, order, prefilter=False, **kw)
        var = renderer.read_projected()
    _check_records(sc, var)
    _check(want, got, t)
    _check_image(sc, order, img, t)


# ---- HeightMap and Sphere (the FULL instantiations) ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ["reference", "depth-local"])
@pytest.mark.parametrize("mode", S.SURFACE_MODES, ids=lambda m: m.id)
@pytest.mark.parametrize("surface", ["hmap", "sphere"])
def test_mapped_surfaces(renderer, surface, mode, order):
    sc = S.framed(surface, mode)
    want = sc.expected(ORDERS[order][0])
    with _mode(renderer, sc) as kw:
        img, got, t = _frame(renderer, sc, order, **kw)
    _check(want, got, t)
    _check_image(sc, order, img, t)


# ---- shards --------------------------------------------------------------------------------------------------------------------------------
def _paste(canvas, part, sc, shard, band):
    """One shard's image into its place of the frame."""
    if len(shard) > 2:
        x0 = shard[0] * band
        x1 = min(sc.W, x0 + band)
        canvas[:, x0:x1] = part[:, :x1 - x0]
    else:
        for k, ty in enumerate(range(shard[0], sc.tiles[1], shard[1])):
            y0, y1 = ty * 16, min(sc.H, ty * 16 + 16)
            canvas[y0:y1] = part[k * 16:k * 16 + (y1 - y0)]


SHARD_FRAMES = [("bands", Mode(aa=4096), 3, "cols"), ("plane", Mode(aa=4096), 3, "cols"), ("hmap", Mode(aa=4096), 3, "cols"),
                ("plane", Mode("oblique", 4096), 3, "rows"), ("plane", Mode(fade=True), 2, "cols")]


@pytest.mark.parametrize("order", ["reference", "depth-local"])
@pytest.mark.parametrize("name,mode,count,kind", SHARD_FRAMES, ids=[f"{n}-{m.id}-{c}{k}" for n, m, c, k in SHARD_FRAMES])
def test_shard_local_lists(renderer, name, mode, count, kind, order):
    """Column bands with the filter on (k_cull's band bound carries + aa_s: a cell whose grown splats reach the band must stay; the "bands"
    scene is built so that a bound without the term loses pairs, tests/pair_list_scenes.py), row shards of an orthographic filtered frame
    (orthographic frames have no column form), column bands of a faded frame: each shard's lists, in its local tile numbering, are the
    frame's, and the shards' images tile the oracle's."""
    sc = S.framed(name, mode)
    tx, ty = sc.tiles
    full = sc.expected(ORDERS[order][0])
    ref, st = sc.render(ORDERS[order][0])
    band = renderer.shard_cols_padded(sc.W, count) if kind == "cols" else 0
    canvas = np.zeros_like(ref)
    total = 0
    with _mode(renderer, sc) as kw:
        for index in range(count):
            shard = (index, count, "cols") if kind == "cols" else (index, count)
            want = PL.shard_lists(full, tx, ty, shard, band_px=band)
            assert want.total() > 1000
            img, got, t = _frame(renderer, sc, order, shard=shard, **kw)
            msg = PL.compare(want, got)
            assert msg is None, (shard, msg)
            assert got.total() == t["n_pairs"]
            # a shard projects what can reach it: never more visible splats than the frame has, all of them when nothing is culled by band
            assert t["n_visible"] <= st["n_visible"] and (kind == "cols" or t["n_visible"] == st["n_visible"])
            _paste(canvas, img, sc, shard, band)
            total += got.total()
    assert total == full.total()
    d = H.max_abs_diff(canvas, ref)
    assert d <= TOL, d


# ---- long lists, and the re-run after a pair overflow --------------------------------------------------------------------------------------
def test_dense_scene_filtered_long_lists(renderer):
    """The dense scene with every rectangle grown by the filter at 4096: lists far beyond 4096 pairs in depth order -- k_tile_depth_sort's
    long classes, several compositor segments per tile."""
    sc = S.framed("dense", Mode(aa=4096))
    order = "depth-local"
    want = sc.expected(ORDERS[order][0])
    n = want.lengths()
    assert n.max() > 4096 and int((n > 512).sum()) >= 20
    with _mode(renderer, sc) as kw:
        img, got, t = _frame(renderer, sc, order, **kw)
    _check(want, got, t)
    _check_image(sc, order, img, t)


@pytest.mark.parametrize("order", list(ORDERS))
def test_lists_after_a_pair_overflow(renderer, order):
    """GSWT_OPT_PAIR_CAP = 4096 on an orthographic, filtered and faded frame of many more pairs: the re-run keeps the frame's own aa_s,
    projection and atmosphere -- its lists and its image are the frame's."""
    sc = S.framed("plane", Mode("oblique", 4096, True))
    want = sc.expected(ORDERS[order][0])
    assert want.total() > 2 * 4096
    with _mode(renderer, sc, PAIR_CAP=4096) as kw:
        img, got, t = _frame(renderer, sc, order, **kw)
    _check(want, got, t)
    _check_image(sc, order, img, t)
    if order != "reference":
        assert t["depth_frames_enqueued"] >= 2                      # the frame really ran twice
