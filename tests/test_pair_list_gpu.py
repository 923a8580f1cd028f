"""What lies between the vertex stage and the image: the sorted pair list a finished frame's compositor walked (read_pairs) and every
screen tile's slice of it (read_ranges), against lists derived from the oracle alone (tests/pair_list_ref.py: the oracle's blend
sequence reversed, restricted to the entries whose rectangle holds the tile).  k_emit, the pair sort, the tile ranges and both depth
paths of GSWT_ORDER_DEPTH are checked pair by pair: a pair filed under the neighbouring tile, two neighbours swapped, a pair behind
opaque content lost -- none of which the total pair count or the 1e-4 image can see.  All comparisons are between integers.

The frames here are perspective ones with the pixel filter and the atmosphere off.  Orthographic, anti-aliased and faded frames, alone
and combined, are in tests/test_pair_list_modes_gpu.py, which reuses _options / _frame / _check.  Not covered by either file: the fog's
colours (a colour byte, no list), the sequence v2 in those modes (it has no form of them) and orthographic column bands (the API refuses
them)."""
import contextlib

import numpy as np
import pytest

from gswt_renderer_amd import _lib as L
from oracle import gswt_oracle as orc
from tests import helpers as H
from tests import pair_list_ref as PL
from tests import pair_list_scenes as S

pytestmark = pytest.mark.gpu
TOL = 1e-4

# (order mode, GSWT_OPT_DEPTH_SORT): the reference order, depth order through the tile-local sort, through the global depth passes
ORDERS = {"reference": (L.GSWT_ORDER_REFERENCE, 0), "depth-local": (L.GSWT_ORDER_DEPTH, 0), "depth-global": (L.GSWT_ORDER_DEPTH, 1)}


@contextlib.contextmanager
def _options(renderer, **opts):
    """renderer.options(**opts) for the block, and no height map afterwards."""
    try:
        with renderer.options(**opts):
            yield
    finally:
        renderer.configure(None)


def _frame(renderer, sc, order, *, shard=None, prefilter=True, **render_kw):
    """Uploads the scene, renders one frame and reads its lists back, the pairs translated to the oracle's entry numbers.
    Returns (image, PairLists, timings).  Call inside _options (the LOD prefilter is read when the draws are set)."""
    order_mode, depth_sort = ORDERS[order]
    with renderer.options(DEPTH_SORT=depth_sort):
        renderer.configure(sc.hm)
        sc.case.upload(renderer)
        l0, g0, _ = renderer.depth_stats()
        img = renderer.render(sc.cam, sc.su, sc.W, sc.H, order_mode=order_mode, **({"shard": shard} if shard else {}), **render_kw)
        l1, g1, _ = renderer.depth_stats()
        t = renderer.timings()
        ranges, pairs = renderer.read_ranges(), renderer.read_pairs()
    # the frame took the path the test names (re-runs count too)
    assert (l1 > l0, g1 > g0) == (order == "depth-local", order == "depth-global")
    emap = PL.product_entry_map(sc.case.draws, sc.case.orc_draws, prefilter=prefilter)
    assert pairs.shape[0] == t["n_pairs"]
    t["depth_frames_enqueued"] = (l1 - l0) + (g1 - g0)              # (a re-run counts again)
    assert pairs.size == 0 or int(pairs.max()) < emap.shape[0], "a pair names no list entry"
    return img, PL.PairLists.from_gpu(ranges, emap[pairs]), t


def _check(want, got, t):
    msg = PL.compare(want, got)
    assert msg is None, msg
    assert got.total() == want.total() == t["n_pairs"]


@pytest.mark.parametrize("debug", [0, 1], ids=["live-table", "debug-varyings"])
@pytest.mark.parametrize("order", list(ORDERS))
@pytest.mark.parametrize("surface", list(S.SURFACES))
def test_surfaces_and_order_modes(renderer, surface, order, debug):
    """Plane (17 x 11 tiles), height map and sphere (20 x 15), each with a merged draw among plain ones.  A debug-varyings frame runs
    k_emit over every chunk and keeps the unfiltered static lists; a normal frame runs the live-chunk table over the LOD-filtered ones."""
    sc = S.SURFACES[surface]()
    want = sc.expected(ORDERS[order][0])
    assert int((want.lengths() > 0).sum()) > 100 and want.total() > 10000
    with _options(renderer, DEBUG_VARYINGS=debug, NO_LOD_PREFILTER=debug):
        img, got, t = _frame(renderer, sc, order, prefilter=not debug)
        var = renderer.read_projected() if debug else None
    _check(want, got, t)
    if debug:
        # the lists rest on the vertex stage the other tests compare: the same visibility and depth bits, entry by entry
        r = sc.rects()
        vis = r["visible"] == 1
        assert not (vis & (var["visible"] == 0)).any()
        assert np.array_equal(var["depth"][vis].view(np.uint32), r["depth"][vis].view(np.uint32))
    ref, st = sc.render(ORDERS[order][0])
    assert t["n_visible"] == st["n_visible"] and H.max_abs_diff(img, ref) <= TOL


@pytest.mark.parametrize("order", list(ORDERS))
def test_rounding_sequence_v2(renderer, order):
    """GSWT_OPT_STRICT_VS = 0 against the oracle's v2() mode: rectangles and depths come from the other vertex stage."""
    sc = S.hmap()
    with orc.v2():
        want = sc.expected(ORDERS[order][0])
        r2 = sc.rects()
    r = sc.rects()
    assert not np.array_equal(r2["depth"].view(np.uint32), r["depth"].view(np.uint32))      # the two sequences differ
    with _options(renderer, STRICT_VS=0):
        _, got, t = _frame(renderer, sc, order)
    _check(want, got, t)


@pytest.mark.parametrize("order", list(ORDERS))
def test_dense_scene_long_lists(renderer, order):
    """The longest tile list exceeds 4096 pairs and many exceed 512 (on the reference's lists): several compositor segments per tile,
    three size classes of k_tile_depth_sort, runs of one tile over many sort blocks."""
    sc = S.dense()
    want = sc.expected(ORDERS[order][0])
    n = want.lengths()
    assert n.max() > 4096 and int((n > 512).sum()) >= 20 and int(((n > 0) & (n <= 512)).sum()) >= 20
    with _options(renderer):
        img, got, t = _frame(renderer, sc, order)
    _check(want, got, t)
    ref, _ = sc.render(ORDERS[order][0])
    assert H.max_abs_diff(img, ref) <= TOL


@pytest.mark.parametrize("order", ["depth-local", "depth-global"])
def test_twin_draws_stand_in_slot_order(renderer, order):
    """The same draw list twice at the same offsets: every splat has a twin with identical depth bits, entries apart.  In depth order the
    twins are neighbours in every list they share, and the contract is "equal depths in composite order": the later draw's twin -- the
    lower slot, the higher entry number -- first.  The frames are 320 x 240, 300 tile lists each; over the TWIN_CAMERAS more than 1000
    lists hold such a tie (asserted on the reference)."""
    ties = 0
    for k in range(len(S.TWIN_CAMERAS)):
        sc = S.twins(k)
        want = sc.expected(L.GSWT_ORDER_DEPTH)
        ties += S.twin_tie_tiles(sc)
        with _options(renderer):
            _, got, t = _frame(renderer, sc, order)
        _check(want, got, t)
        # the contract read off the GPU's own list: inside a depth tie the entry numbers fall
        d = sc.rects()["depth"].view(np.uint32).astype(np.int64)
        for tile in range(got.n_tiles):
            l = got.tile(tile)
            tie = np.diff(d[l]) == 0
            assert (np.diff(l)[tie] < 0).all(), (k, tile)
    assert ties >= 1000


@pytest.mark.parametrize("order", list(ORDERS))
def test_lists_behind_an_opaque_wall(renderer, order):
    """A wall of opaque splats in front of the plane scene, early-out at transmittance_eps = 1e-4: the pairs behind the wall contribute
    nothing to the image, and their lists must still be complete and ordered."""
    sc = S.wall()
    want = sc.expected(ORDERS[order][0])
    assert S.wall_hidden_tiles(sc, ORDERS[order][0]) >= 50
    ref, st = sc.render(ORDERS[order][0])
    assert int((ref[..., 3] >= 1.0 - 1e-4).sum()) > 5000
    with _options(renderer):
        img, got, t = _frame(renderer, sc, order, transmittance_eps=1e-4)
    _check(want, got, t)
    assert t["n_visible"] == st["n_visible"] and H.max_abs_diff(img, ref) <= TOL


@pytest.mark.parametrize("order", list(ORDERS))
def test_shard_local_lists(renderer, order):
    """Three row shards (tile row ty is row ty // 3 of shard ty % 3) and two column bands (gswt_shard_cols_padded): each shard's lists, in
    its local tile numbering, are the frame's."""
    sc = S.plane()
    tx, ty = sc.tiles
    full = sc.expected(ORDERS[order][0])
    band = renderer.shard_cols_padded(sc.W, 2)
    assert band % 16 == 0 and band < sc.W
    total = {"rows": 0, "cols": 0}
    with _options(renderer):
        for shard in [(r, 3) for r in range(3)] + [(r, 2, "cols") for r in range(2)]:
            want = PL.shard_lists(full, tx, ty, shard, band_px=band)
            assert want.total() > 1000
            _, got, t = _frame(renderer, sc, order, shard=shard)
            msg = PL.compare(want, got)
            assert msg is None, (shard, msg)
            assert got.total() == t["n_pairs"]
            total["cols" if len(shard) > 2 else "rows"] += got.total()
    assert total["rows"] == total["cols"] == full.total()


@pytest.mark.parametrize("order", list(ORDERS))
def test_lists_after_a_pair_overflow(renderer, order):
    """GSWT_OPT_PAIR_CAP = 4096 on a frame of more pairs: the first run overflows and processes nothing, the re-run's lists are the frame's."""
    sc = S.plane()
    want = sc.expected(ORDERS[order][0])
    assert want.total() > 2 * 4096
    with _options(renderer, PAIR_CAP=4096):
        _, got, t = _frame(renderer, sc, order)
    _check(want, got, t)
    if order != "reference":
        assert t["depth_frames_enqueued"] >= 2                      # the frame really ran twice


def test_read_pairs_needs_a_frame():
    from gswt_renderer_amd.renderer import GSWTError, GSWTRenderer
    r = GSWTRenderer(0)
    try:
        with pytest.raises(GSWTError) as e:
            r.read_pairs()
        assert e.value.code == L.GSWT_ERR_STATE
    finally:
        r.close()
