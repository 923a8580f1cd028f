"""The per-draw viewport cull and LOD skip (renderer.rs:472-497) on the CPU: tests/draw_cull_ref.py against the oracle's draw loop
on the scene tests/test_draw_cull_gpu.py uses.  Anything failing here would make the GPU tests vacuous: the reference must
decide what the oracle decides, the scene must decide differently at every value, the binary32 decisions must be the float64
ones away from the bound, and the single-ulp knife edges must exist."""
import numpy as np
import pytest

from tests import draw_cull_ref as R


@pytest.fixture(scope="module")
def sc():
    return R.scene()


def _kept_ids(draws):
    return [int(d.tile.map_index) for d in draws]


def test_scene_is_the_one_the_counts_were_taken_on(sc):
    assert len(sc.insts) == 46
    assert sorted(set(sc.map_index)) == sorted(sc.map_index)            # map_index identifies an instance
    assert {k: sc.kind.count(k) for k in ("plain", "blend", "merged")} == {"plain": 23, "blend": 20, "merged": 3}
    assert sum(sc.cull_enable) == 43
    assert all(c is not None for ce, c in zip(sc.cull_enable, sc.corners) if ce)
    assert [k == "merged" for k in sc.kind] == [not ce for ce in sc.cull_enable]


@pytest.mark.parametrize("cd,count", R.CULL_DISTS, ids=[repr(c) for c, _ in R.CULL_DISTS])
def test_reference_keeps_what_the_oracle_keeps_per_culling_dist(sc, cd, count):
    want = _kept_ids(sc.oracle_draws(culling_dist=cd))
    keep = sc.ref_keep(culling_dist=cd)
    got = [mi for mi, k in zip(sc.map_index, keep) if k]
    assert got == want
    assert len(got) == count
    assert all(k for k, kind in zip(keep, sc.kind) if kind == "merged")  # cull_enable = 0 survives every value


@pytest.mark.parametrize("mask,count", R.LOD_MASKS)
def test_reference_keeps_what_the_oracle_keeps_per_lod_mask(sc, mask, count):
    want = _kept_ids(sc.oracle_draws(culling_dist=1.0, mask=mask))
    got = [mi for mi, k in zip(sc.map_index, sc.ref_keep(culling_dist=1.0, mask=mask)) if k]
    assert got == want
    assert len(got) == count
    # the bit is that of tile_id[0] (a blending draw's base list may be LOD - 1, a merged draw carries its head's LOD)
    by_mi = dict(zip(sc.map_index, sc.all_draws))
    assert all(R.lod_kept(mask, by_mi[mi].tile.tile_id[0]) for mi in got)


def test_lod_bit_differs_from_base_lod_somewhere(sc):
    """Blending draws that read the list of LOD - 1 exist, so a mask indexed by base_lod decides differently."""
    n = sum(1 for d in sc.all_draws if d.base is not None and d.base[0] != d.tile.tile_id[0])
    assert n >= 3, n


@pytest.mark.parametrize("cd", [c for c, _ in R.CULL_DISTS], ids=[repr(c) for c, _ in R.CULL_DISTS])
def test_f32_and_f64_decisions_agree_away_from_the_bound(sc, cd):
    qualify = 0
    for ce, c, t32 in zip(sc.cull_enable, sc.corners, sc.terms):
        if not ce:
            continue
        t64 = R.cull_terms64(sc.vp, c)
        if min(R.margin(t32, cd), R.margin(t64, cd)) < 1e-5:
            continue
        qualify += 1
        assert R.keeps(t32, cd) == R.keeps(t64, cd), (cd, t32, t64)
    assert qualify >= 40, qualify


def test_knife_edges(sc):
    """culling_dist = g = max(mx, my) keeps the draw, the next binary32 toward zero drops it and touches no draw with another g."""
    idx = [i for i, ce in enumerate(sc.cull_enable) if ce]
    gs = {i: sc.g(i) for i in idx}
    assert all(np.isfinite(g) and g > 0 for g in gs.values())
    assert all(t[2] > 0 for t in sc.terms if t is not None)               # real tiles never reach the z branch
    single = 0
    for i in idx:
        g, lo = gs[i], R.next_toward_zero(gs[i])
        assert R.f32_bits(lo) == R.f32_bits(g) - 1
        at_g, below = sc.ref_keep(culling_dist=g), sc.ref_keep(culling_dist=lo)
        assert at_g[i] and not below[i]
        assert set(_kept_ids(sc.oracle_draws(culling_dist=g))) == {mi for mi, k in zip(sc.map_index, at_g) if k}
        assert set(_kept_ids(sc.oracle_draws(culling_dist=lo))) == {mi for mi, k in zip(sc.map_index, below) if k}
        flipped = [j for j in range(len(at_g)) if at_g[j] != below[j]]
        assert all(R.f32_bits(gs[j]) == R.f32_bits(g) for j in flipped), (i, flipped)
        single += int(flipped == [i])
    assert single >= 38, single
    xg = sum(1 for i in idx if sc.terms[i][0] >= sc.terms[i][1])
    assert (xg, len(idx) - xg) == (27, 16)                                 # x-governed and y-governed draws


def test_reference_special_values():
    """The rule itself on values no real tile produces: NaN terms never replace the running value, w = 0 gives infinite
    quotients, a NaN bound keeps everything."""
    eye = np.eye(4, dtype=np.float32).reshape(16)                          # clip = position, w = 1
    sq = np.array([[0.5, 0.25, 0.1], [0.75, 0.3, 0.2], [0.6, 0.4, -0.3], [0.9, 0.5, 0.0]], dtype=np.float32)
    assert R.cull_terms(eye, sq) == (np.float32(0.5), np.float32(0.25), np.float32(0.2))
    assert R.keeps(R.cull_terms(eye, sq), 0.5) and not R.keeps(R.cull_terms(eye, sq), np.nextafter(np.float32(0.5), np.float32(0)))
    nan_one = sq.copy(); nan_one[0, 0] = np.nan
    # (NaN * 0 is NaN: the whole corner drops out of all three terms)
    assert R.cull_terms(eye, nan_one) == (np.float32(0.6), np.float32(0.3), np.float32(0.2))
    nan_all = np.full((4, 3), np.nan, dtype=np.float32)
    t = R.cull_terms(eye, nan_all)
    assert t == (R.FLT_MAX, R.FLT_MAX, -R.FLT_MAX)
    # (FLT_MAX is not beyond an infinite bound: only there, and at a NaN bound, does a draw without one finite corner stay)
    assert not R.keeps(t, 1.0) and not R.keeps(t, 1e38) and R.keeps(t, float("inf")) and R.keeps(t, float("nan"))
    assert R.keeps(R.cull_terms(eye, sq), float("nan")) and R.keeps(R.cull_terms(eye, sq), float("inf"))
    assert not R.keeps(R.cull_terms(eye, sq), float("-inf"))
    assert [R.lod_kept(1 << 1, l) for l in (1, 33, 32, 31)] == [True, True, False, False]
    assert R.lod_kept(0x80000000, 31) and R.lod_kept(0xFFFFFFF8, 3) and not R.lod_kept(0xFFFFFFF8, 2)
