"""The oracle side of tests/test_pair_list_modes_gpu.py, checked without a GPU.

The C oracle's strict vertex stage has the three stages the HIP path has beside vs_main -- the orthographic Jacobian, the pixel filter,
the far fade (gswt_oracle.c: orc_set_projection / orc_set_antialias / orc_set_fade; oracle.frame_mode) -- and the expected pair lists of
such frames come from it alone.  Here each of the new oracle lines is pinned to a reference that existed before it:
  * orthographic, plane surface: tests/ortho_ref.py's float32 restatement, bit for bit, with and without the filter;
  * the filter under the perspective camera: tests/antialias_ref.py's filter_records of the oracle's own unfiltered records, within the
    tolerances that module records;
  * the fade: tests/atmosphere_ref.py's dist_f32 / fade_f32, which are exact.
And every frame the GPU tests render is shown, on the oracle's lists, to exercise what it is there for (enough tiles and pairs, rectangles
the filter widens, entries the fade removes, depth ties under the orthographic cameras): a scene that stops doing so fails here."""
import dataclasses

import numpy as np
import pytest

from oracle import gswt_oracle as orc
from tests import antialias_ref as AA
from tests import atmosphere_ref as AT
from tests import ortho_ref as OR
from tests import pair_list_ref as PL
from tests import pair_list_scenes as S

FIELDS = ("ndc", "depth", "major", "minor", "rgba")
FRAME_IDS = [f"{n}-{m.id}" for n, m in S.FRAMES]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _assert_records_equal(got, want, where, label):
    for fld in FIELDS:
        assert np.array_equal(_bits(got[fld][where]), _bits(want[fld][where])), (label, fld)


@pytest.fixture(autouse=True)
def _oracle_left_in_its_default_mode():
    yield
    assert orc.frame_mode_is_default() and orc.lib().orc_get_strict() == 2


# ---- the orthographic Jacobian and the filter behind it, bit for bit ---------------------------------------------------------------------
def _ortho_inputs(source, which, value):
    """(camera block, scene block, tex, draws, W, H, aa_s) of the golden plane case / the pair-list plane scene under camera `which`."""
    if source == "golden":
        g = OR.golden()
        cu, su = OR.block_of(OR.camera_args(which, lod_pos=g["pos"])), OR.scene_of(g)
        tex, draws, W, H = g["pp"].tex, g["draws"], OR.W, OR.H
    else:
        sc = S.framed("plane", S.Mode(which))
        cu, su, tex, draws, W, H = sc.cam, sc.su, sc.case.pp.tex, sc.case.orc_draws, sc.W, sc.H
    return cu, su, tex, draws, W, H, (float(AA.aa_s(value, su.splat_scale)) if value else 0.0)


@pytest.mark.parametrize("value", [0, 307, 4096])
@pytest.mark.parametrize("which", ["top", "oblique"])
@pytest.mark.parametrize("source", ["golden", "scene"])
def test_orthographic_plane_records_equal_the_float32_restatement(source, which, value):
    cu, su, tex, draws, W, H, s = _ortho_inputs(source, which, value)
    want = OR.project_ortho_f32(cu, su, tex, draws, aa_s=s if value else None)
    with orc.frame_mode(ortho=1, aa_s=s):
        got = orc.project_draws(cu, su, tex, draws)
        rects = orc.pair_rects(cu, su, tex, draws, W, H)
    assert got.shape == want.shape == rects.shape
    # the restatement's `visible` is the product's, fragment setup included: the oracle's pair_rects carries that one, its vertex stage the
    # survivors before the fragment setup
    assert np.array_equal(rects["visible"], want["visible"])
    vis = want["visible"] == 1
    assert vis.sum() > 300 and (got["visible"][vis] == 1).all()
    _assert_records_equal(got, want, vis, (source, which, value))
    assert np.array_equal(_bits(rects["depth"][vis]), _bits(want["depth"][vis]))
    if value:
        off = OR.project_ortho_f32(cu, su, tex, draws)
        assert np.array_equal(off["visible"], want["visible"])
        assert not np.array_equal(_bits(off["major"][vis]), _bits(want["major"][vis]))
        assert (want["rgba"][vis][:, 3] <= off["rgba"][vis][:, 3]).all() and (want["rgba"][vis][:, 3] < off["rgba"][vis][:, 3]).any()


# ---- the filter under the perspective camera ------------------------------------------------------------------------------------------------
def _check_filtered(got, unf, value, splat_scale, label):
    """Filtered records against antialias_ref.filter_records of the unfiltered ones: the comparison tests/test_antialias_gpu.py makes for the
    GPU's records (same tolerances, same masking of clamped axes), except that a splat of alpha 0 -- these scenes have some -- must stay
    at 0 instead of entering a relative error.  Returns the number of records compared."""
    want, masked, n_masked = AA.filter_records(unf, value, splat_scale)
    assert got.shape == unf.shape
    vis = unf["visible"] == 1
    assert np.array_equal(got["visible"] == 1, vis), label            # the filter sits behind every rejection of the vertex stage
    assert n_masked <= 0.01 * vis.sum(), (label, n_masked)
    for fld in ("ndc", "depth"):
        assert np.array_equal(_bits(got[fld][vis]), _bits(unf[fld][vis])), (label, fld)
    assert np.array_equal(_bits(np.ascontiguousarray(got["rgba"][vis][:, :3])), _bits(np.ascontiguousarray(unf["rgba"][vis][:, :3]))), label
    ok = vis & ~masked
    gm, gn = got["major"][ok].astype(np.float64), got["minor"][ok].astype(np.float64)
    lm, ln = np.hypot(gm[:, 0], gm[:, 1]), np.hypot(gn[:, 0], gn[:, 1])
    rel = lambda g, w: float((np.abs(g - w) / w).max())
    ga, wa = got["rgba"][ok][:, 3].astype(np.float64), want["alpha"][ok]
    assert (ga[wa == 0] == 0).all(), label
    e = (rel(lm, want["len_major"][ok]), rel(ln, want["len_minor"][ok]), rel(ga[wa > 0], wa[wa > 0]))
    d = max(float(np.abs(gm / lm[:, None] - want["dir_major"][ok]).max()), float(np.abs(gn / ln[:, None] - want["dir_minor"][ok]).max()))
    print(f"{label}: {int(ok.sum())} records ({n_masked} masked) |major| {e[0] / AA.U:.2f} |minor| {e[1] / AA.U:.2f} alpha {e[2] / AA.U:.2f} x 2^-24 "
          f"(tolerance {AA.VARYINGS_RTOL / AA.U:.0f}), directions {d / AA.U:.2f} x 2^-24 (tolerance {AA.DIRECTION_ATOL / AA.U:.0f})")
    assert all(x <= AA.VARYINGS_RTOL for x in e), (label, e)          # (a NaN fails)
    assert d <= AA.DIRECTION_ATOL, (label, d)
    # the filter did something: every splat grew, and every one with some opacity lost some
    assert (lm > np.hypot(*unf["major"][ok].astype(np.float64).T)).all() and (ga[wa > 0] < unf["rgba"][ok][:, 3][wa > 0]).all(), label
    return int(ok.sum())


@pytest.mark.parametrize("value", [307, 4096])
@pytest.mark.parametrize("surface", list(S.SURFACES))
def test_perspective_filtered_records_follow_the_unfiltered_ones(surface, value):
    """The eigenvalues cannot be read out of the oracle: its filtered records against antialias_ref.filter_records of its unfiltered ones,
    tolerances and masking as tests/test_antialias_gpu.py applies them to the GPU's."""
    base = S.SURFACES[surface]()
    sc = S.framed(surface, S.Mode(aa=value))
    assert sc.aa_s == float(AA.aa_s(value, base.su.splat_scale)) > 0.0
    n = _check_filtered(sc.records(), base.records(), value, base.su.splat_scale, f"oracle {surface} filter {value}")
    assert n > 5000


@pytest.mark.parametrize("surface", list(S.SURFACES))
def test_filter_zero_gives_the_unfiltered_bits(surface):
    base = S.SURFACES[surface]()
    want, want_r = base.records(), base.rects()
    for sc in (dataclasses.replace(base, aa_s=0.0), dataclasses.replace(base, aa_s=-1.0)):
        assert sc.records().tobytes() == want.tobytes() and sc.rects().tobytes() == want_r.tobytes()
    # ... and so does the rounding sequence v2, which has no form of the three stages (the product refuses such frames)
    full = S.framed(surface, S.Mode(aa=4096, fade=True))
    with orc.v2():
        v2_plain, v2_mode = base.records(), dataclasses.replace(full, cam=base.cam).records()
    assert v2_plain.tobytes() == v2_mode.tobytes() and v2_plain.tobytes() != want.tobytes()


# ---- the fade ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("aa", [0, 4096])
@pytest.mark.parametrize("which", [None, "top", "oblique"], ids=["perspective", "top", "oblique"])
def test_faded_plane_records_equal_the_exact_reference(which, aa):
    sc = S.framed("plane", S.Mode(which, aa, True))
    off = dataclasses.replace(sc, ramp=None)
    p = AT.params(sc.atmosphere())
    assert p["fade_on"] and float(p["fade_end"]) == sc.ramp[1] > sc.ramp[0] == float(p["fade_start"])
    dist = AT.dist_f32(sc.cam.cam_pos, sc.su, sc.case.pp.tex, sc.case.orc_draws)
    t, fs = AT.fade_f32(dist, p)
    got, unf = sc.records(), off.records()
    assert np.array_equal(got["visible"] == 1, (unf["visible"] == 1) & (t > 0))
    vis = got["visible"] == 1
    share = 1.0 - vis.sum() / (unf["visible"] == 1).sum()
    inside = int(((t > 0) & (t < 1) & vis).sum())
    print(f"{sc.name}: ramp {sc.ramp}, the fade discards {share:.3f} of {int((unf['visible'] == 1).sum())} survivors, {inside} on the ramp")
    assert 0.1 <= share <= 0.5 and inside > 1000
    with np.errstate(all="ignore"):
        alpha = (unf["rgba"][:, 3] * fs).astype(np.float32)
    assert np.array_equal(_bits(got["rgba"][vis][:, 3]), _bits(alpha[vis]))
    assert (got["rgba"][vis][:, 3] < unf["rgba"][vis][:, 3]).sum() > 1000
    for fld in ("ndc", "depth", "major", "minor"):
        assert np.array_equal(_bits(got[fld][vis]), _bits(unf[fld][vis])), fld
    assert np.array_equal(_bits(np.ascontiguousarray(got["rgba"][vis][:, :3])), _bits(np.ascontiguousarray(unf["rgba"][vis][:, :3])))
    # the rectangles of the survivors are the unfaded frame's, the others' are gone
    r, r0 = sc.rects(), off.rects()
    keep = r["visible"] == 1
    assert np.array_equal(keep, (r0["visible"] == 1) & (t > 0)) and r[keep].tobytes() == r0[keep].tobytes()
    assert (S.rect_areas(r[~keep]) == 0).all()


# ---- the lists discriminate ----------------------------------------------------------------------------------------------------------------
def _changed_tiles(a, b):
    return sum(1 for t in range(a.n_tiles) if not np.array_equal(a.tile(t), b.tile(t)))


@pytest.mark.parametrize("name,mode", S.FRAMES, ids=FRAME_IDS)
def test_frames_exercise_what_they_are_there_for(name, mode):
    sc = S.framed(name, mode)
    r = sc.rects()
    e = sc.expected(PL.ORDER_DEPTH)
    _, st = sc.render(PL.ORDER_DEPTH)
    assert e.total() == st["n_pairs16"] == int(S.rect_areas(r).sum()) and int(r["visible"].sum()) == st["n_visible"]
    with_list = int((e.lengths() > 0).sum())
    line = f"{sc.name}: {with_list} / {e.n_tiles} tiles with a list, {e.total()} pairs, {st['n_visible']} visible"
    if name == "plane":
        assert e.n_tiles == 187 and with_list >= 150 and e.total() >= 10000, line
    else:
        assert 2 * with_list >= e.n_tiles and e.total() >= 5000, line
    if mode.aa:
        off = dataclasses.replace(sc, aa_s=0.0)
        r0 = off.rects()
        assert np.array_equal(r0["visible"], r["visible"])
        wider = int((S.rect_areas(r) > S.rect_areas(r0)).sum())
        line += f", {wider} entries widened by the filter"
        assert wider >= 1000 and not (S.rect_areas(r) < S.rect_areas(r0)).any(), line
        for order in (PL.ORDER_REFERENCE, PL.ORDER_DEPTH):
            assert PL.compare(off.expected(order), sc.expected(order)) is not None
    if mode.fade:
        off = dataclasses.replace(sc, ramp=None)
        v0 = int(off.rects()["visible"].sum())
        share = 1.0 - st["n_visible"] / v0
        changed = _changed_tiles(off.expected(PL.ORDER_DEPTH), e)
        line += f", the fade removes {share:.3f} of {v0} entries and changes {changed} tiles' lists"
        assert 0.1 <= share <= 0.5 and changed >= 20, line
    if mode.ortho:
        ties = S.twin_tie_tiles(sc)
        line += f", {ties} tile lists with a depth tie"
        assert ties >= 1, line
        # a list in depth order: ascending depths, ties by falling entry number (what the GPU's lists are compared with)
        for t in range(e.n_tiles):
            l = e.tile(t)
            d = r["depth"][l]
            assert (np.diff(d) >= 0).all() and (np.diff(l)[np.diff(d) == 0] < 0).all()
    print(line)


def test_dense_filtered_frame_has_long_lists_on_the_reference():
    sc = S.framed("dense", S.Mode(aa=4096))
    n, n0 = sc.expected(PL.ORDER_DEPTH).lengths(), S.dense().expected(PL.ORDER_DEPTH).lengths()
    print(f"{sc.name}: longest list {int(n.max())} (unfiltered {int(n0.max())}), {int((n > 4096).sum())} lists beyond 4096, {int(n.sum())} pairs")
    assert n.max() > 4096 and int((n > 512).sum()) >= 20 and n.sum() > n0.sum() + 10000


def test_shard_frames_reach_across_their_bands():
    """The column-band frames of the GPU tests: with the filter at 4096, entries whose unfiltered rectangle lies in one band reach into
    the next (these are what a band cull that forgets the filter's pad would lose)."""
    for name in ("plane", "hmap"):
        sc = S.framed(name, S.Mode(aa=4096))
        r, r0 = sc.rects(), dataclasses.replace(sc, aa_s=0.0).rects()
        tx = sc.tiles[0]
        bt = -(-tx // 3)                     # tile columns per band (the product pads the band to whole tiles; the GPU test reads its width)
        both = (S.rect_areas(r) > 0) & (S.rect_areas(r0) > 0)
        crosses = lambda q: (q["tx0"] // bt) != (q["tx1"] // bt)
        new = int((both & crosses(r) & ~crosses(r0)).sum())
        print(f"{sc.name}: {new} entries cross a band boundary only with the filter on")
        assert new >= 50


def test_bands_scene_pins_the_filter_term_of_the_band_cull():
    """On the oracle's rectangles and a float64 model of k_cull's band bound: without the filter's s in the pad, cells left of the first
    band boundary are dropped for the second band although their grown splats reach it; with the term nothing is lost."""
    sc = S.framed("bands", S.Mode(aa=4096))
    e = sc.expected(PL.ORDER_DEPTH)
    lost, kept = S.pairs_lost_by_an_unfiltered_band_pad(sc, 3), S.pairs_lost_by_an_unfiltered_band_pad(sc, 3, with_filter_term=True)
    print(f"{sc.name}: {int((e.lengths() > 0).sum())} / {e.n_tiles} tiles with a list, {e.total()} pairs; a band pad without the filter's term "
          f"loses {lost} pairs over 3 column bands, the kernel's pad {kept}")
    assert lost >= 20 and kept == 0 and e.total() >= 10000
    # ... and the same model loses nothing on the unfiltered frame: the loss is the filter's
    assert S.pairs_lost_by_an_unfiltered_band_pad(dataclasses.replace(sc, aa_s=0.0), 3) == 0


# ---- the two builds of the oracle ----------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(not orc.cpu_has_fma(), reason="the -mfma build needs the unit")
@pytest.mark.parametrize("name,mode", [("plane", S.Mode("oblique")), ("plane", S.Mode(aa=4096)), ("plane", S.Mode(fade=True)),
                                       ("plane", S.Mode("oblique", 307, True)), ("sphere", S.Mode("top", 4096)), ("hmap", S.Mode(aa=307, fade=True))],
                         ids=lambda v: v.id if isinstance(v, S.Mode) else v)
def test_both_builds_agree_bit_for_bit(name, mode):
    sc = S.framed(name, mode)
    out = []
    for fma in (False, True):
        with orc.use_build(fma):
            img, st = sc.render(PL.ORDER_DEPTH)
            out.append((sc.records().tobytes(), sc.rects().tobytes(), img.tobytes(), st))
            assert orc.frame_mode_is_default()
    assert out[0] == out[1]


def test_frame_mode_restores_what_it_found():
    l = orc.lib()
    with orc.frame_mode(ortho=1, aa_s=0.25, fade=(12.0, 0.5)):
        assert l.orc_get_projection() == 1 and l.orc_get_antialias() == 0.25 and not orc.frame_mode_is_default()
        with orc.frame_mode(aa_s=0.5):
            assert l.orc_get_projection() == 0 and l.orc_get_antialias() == 0.5
        assert l.orc_get_projection() == 1 and l.orc_get_antialias() == 0.25
        with pytest.raises(RuntimeError):
            with orc.frame_mode(fade=(3.0, 1.0)):
                raise RuntimeError("inside")
        assert l.orc_get_projection() == 1
    assert orc.frame_mode_is_default()
