"""The oracle side of the pair-list tests (tests/test_pair_list_gpu.py), checked without a GPU: oracle.pair_rects against orc.render's
own pair count and a rectangle worked out by hand, and the comparison of tests/pair_list_ref.py against planted faults."""
import math

import numpy as np
import pytest

from oracle import gswt_oracle as orc
from oracle import wangtile_oracle as wo
from tests import pair_list_ref as PL
from tests import pair_list_scenes as S
from tests.test_golden import GOLD, _load
from tests.test_oracle_kat import _draw1, _one_splat_tex


def _areas(r):
    w = np.maximum(r["tx1"].astype(np.int64) - r["tx0"] + 1, 0)
    h = np.maximum(r["ty1"].astype(np.int64) - r["ty0"] + 1, 0)
    return w * h


@pytest.mark.parametrize("path", GOLD, ids=[p.rsplit("/", 1)[-1] for p in GOLD])
def test_rect_areas_sum_to_the_pair_count_on_golden_cases(path):
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
        osort = ow.sort_tiles(pos, cam.view_proj())
        draws = wo.renderer_draws(pp, osort, cam.view_proj())
    hm = ou.height_map.reshape(ou.height_map_wh[1], ou.height_map_wh[0]) if ou.surface_type == 1 else None
    su = wo.scene_uniforms_from_data(ou, osd["center_coord"], **rc)
    bgd = np.full((H, W), 1.0, np.float32)
    for ctx, key in ((orc.strict(fragment=False), "stats_default"), (orc.v2(), "stats")):
        with ctx:
            r = orc.pair_rects(cam.uniforms(), su, pp.tex, draws, W, H, height_map=hm)
            var = orc.project_draws(cam.uniforms(), su, pp.tex, draws, height_map=hm)
            _, st_bg = orc.render(cam.uniforms(), su, pp.tex, draws, W, H, height_map=hm, bg_depth=bgd)
            r_bg = orc.pair_rects(cam.uniforms(), su, pp.tex, draws, W, H, height_map=hm, bg_depth=bgd)
        n_inst, n_vis, n_pairs = g[key].tolist()
        assert r.shape[0] == n_inst and int(r["visible"].sum()) == n_vis and int(_areas(r).sum()) == n_pairs, key
        assert n_pairs > 0
        # visible may only drop against the vertex stage (frag_setup refuses degenerate axes); the depth is the vertex stage's
        vis = r["visible"] == 1
        assert not (vis & (var["visible"] == 0)).any()
        assert np.array_equal(r["depth"][vis].view(np.uint32), var["depth"][vis].view(np.uint32))
        # an entry without pairs has the empty rectangle, one with pairs lies inside the frame
        a = _areas(r)
        assert (a[~vis] == 0).all()
        assert (r["tx0"][a > 0] >= 0).all() and (r["tx1"][a > 0] <= (W - 1) >> 4).all()
        assert (r["ty0"][a > 0] >= 0).all() and (r["ty1"][a > 0] <= (H - 1) >> 4).all()
        # with a depth buffer a splat at depth 1.0 makes pairs too: the count follows
        assert int(_areas(r_bg).sum()) == st_bg["n_pairs16"] >= n_pairs
    assert orc.lib().orc_get_strict() == 2                  # the context managers restore the default


@pytest.mark.parametrize("name", sorted(S.ALL))
def test_rect_areas_sum_to_the_pair_count_on_the_gpu_tests_scenes(name):
    sc = S.ALL[name]()
    r = sc.rects()
    for mode in (PL.ORDER_REFERENCE, PL.ORDER_DEPTH):
        _, st = sc.render(mode)
        assert r.shape[0] == st["n_instanced"] and int(r["visible"].sum()) == st["n_visible"]
        assert int(_areas(r).sum()) == st["n_pairs16"] > 1000
        e = sc.expected(mode)
        assert e.n_tiles == sc.tiles[0] * sc.tiles[1] and e.total() == st["n_pairs16"]
        # every list is the blend sequence reversed: in reference order descending entries, in depth order ascending depths
        for t in range(e.n_tiles):
            l = e.tile(t)
            if mode == PL.ORDER_REFERENCE:
                assert (np.diff(l) < 0).all()
            else:
                d = r["depth"][l]
                assert (np.diff(d) >= 0).all()
                tie = np.diff(d) == 0
                assert (np.diff(l)[tie] < 0).all()
    with orc.v2():
        r2 = sc.rects()
        _, st2 = sc.render(0)
    assert int(_areas(r2).sum()) == st2["n_pairs16"]


def test_dense_scene_has_long_lists_on_the_reference():
    L = S.dense().expected(PL.ORDER_DEPTH).lengths()
    assert L.max() > 4096 and int((L > 512).sum()) >= 20 and int(((L > 0) & (L <= 512)).sum()) >= 20


def test_twin_scenes_hold_ties_on_the_reference():
    assert sum(S.twin_tie_tiles(S.twins(k)) for k in range(len(S.TWIN_CAMERAS))) >= 1000


def test_wall_scene_hides_complete_lists_on_the_reference():
    sc = S.wall()
    img, _ = sc.render(PL.ORDER_REFERENCE)
    assert S.wall_hidden_tiles(sc, PL.ORDER_REFERENCE) >= 50 and S.wall_hidden_tiles(sc, PL.ORDER_DEPTH) >= 50
    assert int((img[..., 3] >= 1.0 - 1e-4).sum()) > 5000          # pixels the early-out at 1e-4 can cut behind


def test_one_splat_rectangle_known_answer():
    """The default camera (fovy 45 degrees) at (0, 0, 5) looks along +y; a splat on its axis at distance 4 with sigma (0.25, ., 0.375) --
    both 4 sigma^2 exact in f16, the longer axis upright (the other way round the eigenvector is normalize((0, 0))) -- projects to the
    centre (80, 64) of a 160 x 128 frame with pixel sigmas s = sigma f / 4, f = 64 / tan(22.5 deg) = 154.51: 9.657 and 14.485.
    |p| <= 2 with p = d / (s sqrt 2) reaches 2 sqrt(2) s = 27.31 and 40.97 pixels: pixel centres x + 0.5 in [52.69, 107.31] ->
    x = 53 .. 106, blocks 3 .. 6; y + 0.5 in [23.03, 104.97] -> y = 23 .. 104, blocks 1 .. 6."""
    W, H = 160, 128
    cu = orc.default_camera(W, H).uniforms()
    f = 64.0 / math.tan(math.radians(22.5))
    assert abs(cu.focal[0] - f) < 1e-3 and abs(cu.focal[1] - f) < 1e-3
    tex = _one_splat_tex((0.0, 4.0, 5.0), (0.25, 0.1, 0.375))
    su = orc.scene_uniforms(num_lod=1)
    draws = _draw1(valid_lod_id=0)
    r = orc.pair_rects(cu, su, tex, draws, W, H)
    assert r.shape == (1,) and r["visible"][0] == 1
    assert (int(r["tx0"][0]), int(r["tx1"][0]), int(r["ty0"][0]), int(r["ty1"][0])) == (3, 6, 1, 6)
    img, st = orc.render(cu, su, tex, draws, W, H)
    assert st["n_pairs16"] == 24
    # the rectangle is the smallest: the image has coverage in its outermost block columns and rows
    a = img[..., 3]
    assert a[:, 48:64].max() > 0 and a[:, 96:112].max() > 0 and a[16:32].max() > 0 and a[96:112].max() > 0
    assert a[:, :48].max() == 0 and a[:, 112:].max() == 0 and a[:16].max() == 0 and a[112:].max() == 0
    assert r["depth"][0] == orc.project_draws(cu, su, tex, draws)["depth"][0]
    # lists: one entry in each of the 24 tiles of the 10 x 8 frame
    e = PL.expected_lists(r, PL.ORDER_DEPTH, 10, 8)
    assert [t for t in range(80) if e.lengths()[t]] == [ty * 10 + tx for ty in range(1, 7) for tx in range(3, 7)]
    assert (e.pairs == 0).all()
    # a wrong frame size is refused like orc_render refuses it
    with pytest.raises(RuntimeError):
        orc.pair_rects(cu, su, tex, draws, W + 16, H)


def test_shard_tiles_mapping():
    # 5 x 7 tiles in three row shards: shard 1 owns rows 1, 4 as local rows 0, 1
    assert PL.shard_tiles(5, 7, (1, 3)).tolist() == list(range(5, 10)) + list(range(20, 25))
    assert PL.shard_tiles(5, 7, (0, 3)).tolist() == list(range(0, 5)) + list(range(15, 20)) + list(range(30, 35))
    # two column bands of 48 pixels: columns 0-2 and 3-4
    assert PL.shard_tiles(5, 2, (0, 2, "cols"), band_px=48).tolist() == [0, 1, 2, 5, 6, 7]
    assert PL.shard_tiles(5, 2, (1, 2, "cols"), band_px=48).tolist() == [3, 4, 8, 9]
    assert PL.shard_tiles(5, 2, None).tolist() == list(range(10))
    full = PL.PairLists.from_lists([[t, t + 100] for t in range(35)])
    loc = PL.shard_lists(full, 5, 7, (2, 3))
    assert loc.n_tiles == 10 and loc.tile(0).tolist() == [10, 110] and loc.tile(9).tolist() == [29, 129]
    # every tile belongs to exactly one shard
    for shards, kw in (([(r, 3) for r in range(3)], {}), ([(r, 2, "cols") for r in range(2)], dict(band_px=48))):
        assert sorted(np.concatenate([PL.shard_tiles(5, 7, s, **kw) for s in shards]).tolist()) == list(range(35))


def _planted(sc_lists):
    lists = sc_lists.lists()
    t = next(i for i in range(len(lists) - 1) if len(lists[i]) >= 6 and len(lists[i + 1]) >= 1)
    return lists, t


def test_comparison_reports_planted_faults():
    want = S.plane().expected(PL.ORDER_DEPTH)
    assert PL.compare(want, PL.PairLists.from_lists(want.lists())) is None
    # the GPU's form of the same lists: empty tiles read (0, 0)
    rg = np.stack([np.where(want.lengths() > 0, want.start, 0), np.where(want.lengths() > 0, want.end, 0)], axis=1).astype(np.uint32)
    assert PL.compare(want, PL.PairLists.from_gpu(rg, want.pairs.astype(np.uint32))) is None
    # two neighbours of one tile swapped
    lists, t = _planted(want)
    lists[t][[3, 4]] = lists[t][[4, 3]]
    msg = PL.compare(want, PL.PairLists.from_lists(lists))
    assert msg is not None and msg.startswith(f"tile {t}, position 3:"), msg
    # one pair moved to the neighbouring tile: the total is unchanged
    lists, t = _planted(want)
    moved = lists[t][2]
    lists[t] = np.delete(lists[t], 2)
    lists[t + 1] = np.insert(lists[t + 1], 0, moved)
    got = PL.PairLists.from_lists(lists)
    assert got.total() == want.total()
    msg = PL.compare(want, got)
    assert msg is not None and msg.startswith(f"tile {t}, position 2:"), msg
    # one pair dropped and another duplicated: every length is unchanged
    lists, t = _planted(want)
    lists[t][5] = lists[t][4]
    got = PL.PairLists.from_lists(lists)
    assert np.array_equal(got.lengths(), want.lengths())
    msg = PL.compare(want, got)
    assert msg is not None and msg.startswith(f"tile {t}, position 5:"), msg
    # a shorter list, and a range that is no slice of the list
    lists, t = _planted(want)
    lists[t] = lists[t][:-1]
    msg = PL.compare(want, PL.PairLists.from_lists(lists))
    assert msg is not None and msg.startswith(f"tile {t}, position {len(lists[t])}:"), msg
    bad = rg.copy()
    bad[t, 1] = want.pairs.shape[0] + 1
    assert "not a slice" in PL.compare(want, PL.PairLists.from_gpu(bad, want.pairs))


def test_product_entry_map_follows_the_lod_prefilter():
    sc = S.plane()
    case = sc.case
    n = sum(int(np.asarray(d.gs_index).shape[0]) for d in case.orc_draws)
    ident = PL.product_entry_map(case.draws, case.orc_draws, prefilter=False)
    assert np.array_equal(ident, np.arange(n))
    m = PL.product_entry_map(case.draws, case.orc_draws, prefilter=True)
    assert m.shape[0] < n and (np.diff(m) > 0).all()
    # what the filter leaves out is invisible in the oracle: no list ever names it
    r = sc.rects()
    gone = np.setdiff1d(np.arange(n), m)
    assert gone.size and (r["visible"][gone] == 0).all()
