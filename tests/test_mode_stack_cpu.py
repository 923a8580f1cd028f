"""tests/mode_stack_ref.py and its inputs, checked without a GPU (tests/test_mode_stack_gpu.py compares the device with that module).

  * Reduction: with exactly one mode on, the stack is the single-mode reference the tree already has, bit for bit; with tint, shadow
    and fog it is shadow_ref.chain_codes_f64.
  * Coverage: the lattice launches every one of the 64 (FULL, ORTHO, AA, ATM, STY, SHD) points.
  * Population: a condition on the inputs, from the reference alone.  At every lattice point each active discard removes at least 5
    otherwise-visible splats, each active alpha factor differs from 1 on at least 20 visible splats, every pair (and the triple) of
    active colour modes meets on at least 20, at least 20 kept splats lie strictly inside the fade's ramp in a dimmed cell, the plane
    case's draws in a LOD transition keep at least 10 under the fade, and the masks stay within AR.MAX_MASKED.  The counts are printed.
  * Order sensitivity: at the all-on points the stack with tint and shadow swapped, and with the fog in front of the shadow, is more than
    one code away from the true one on at least 20 % of the splats both stages touch.  A second quantisation between tint and shadow
    cannot move a byte by more than one code -- it moves the float by at most half a code and every later stage is a convex mix --, so
    there the condition is the one the device comparison can see: on the plain surface without fog, where colour is compared bit for
    bit, at least 20 % of the tinted and shadowed splats have another byte."""
import numpy as np
import pytest

from oracle import gswt_oracle as orc
from tests import antialias_ref as AAR
from tests import atmosphere_ref as AR
from tests import frame_modes as FM
from tests import mode_stack_ref as MS
from tests import ortho_ref as OR
from tests import shadow_ref as SR
from tests import tile_style_ref as TR

F32 = np.float32
IDS = [pt.id for pt in MS.LATTICE]
CORNERS = [MS.corner(case, cam) for case, cams in MS.CAMERAS.items() for cam in cams]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.fixture(autouse=True)
def _oracle_left_in_its_default_mode():
    yield
    assert orc.frame_mode_is_default()


# ---- reduction ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,cam", [("case_plane", "persp"), ("case_plane", "oblique"), ("case_sphere", "top"), ("case_hmap", "persp")])
def test_styles_alone_are_the_tile_style_reference(case, cam):
    st = MS.stack(MS.Point(case, cam, sty=True))
    unf = FM.view(case, cam)[4]
    want_vis, want = TR.apply(unf["rgba"], unf["visible"], st["sty"])
    assert st["how"] == "exact" and np.array_equal(st["visible"], want_vis) and 0 < want_vis.sum() < (unf["visible"] == 1).sum()
    assert np.array_equal(_bits(st["rgb"][want_vis]), _bits(want[want_vis][:, :3])) and np.array_equal(_bits(st["alpha"][want_vis]), _bits(want[want_vis][:, 3]))
    for fld in MS.GEOMETRY:
        assert np.array_equal(_bits(st["base"][fld][want_vis]), _bits(unf[fld][want_vis])), fld


@pytest.mark.parametrize("cam", ["persp", "oblique"])
def test_the_fade_alone_is_alpha_times_fs(cam):
    st = MS.stack(MS.Point("case_plane", cam, atm="fade"))
    g, cu, su, _, unf = FM.view("case_plane", cam)
    p = AR.params(MS.atmosphere_of(st["point"]))
    t, fs = AR.fade_f32(AR.dist_f32(orc.Camera176.from_buffer_copy(bytes(cu)).cam_pos, su, g["pp"].tex, g["draws"]), p)
    vis = (unf["visible"] == 1) & (t > 0)
    assert st["how"] == "exact" and np.array_equal(st["visible"], vis)
    assert np.array_equal(_bits(st["alpha"][vis]), _bits((unf["rgba"][:, 3].astype(F32) * fs).astype(F32)[vis]))
    assert np.array_equal(_bits(st["rgb"][vis]), _bits(unf["rgba"][vis][:, :3]))


@pytest.mark.parametrize("cam", ["persp", "oblique"])
def test_the_shadow_alone_is_the_shadow_reference(cam):
    st = MS.stack(MS.Point("case_plane", cam, shd=True))
    g, _, su, _, unf = FM.view("case_plane", cam)
    p = SR.params(MS.inputs("case_plane").shadow)
    sh = SR.lookup_f32(SR.centres_f32(su, g["pp"].tex, g["draws"]), p)[0]
    vis = unf["visible"] == 1
    assert st["how"] == "exact" and np.array_equal(st["visible"], vis)
    assert np.array_equal(_bits(st["rgb"][vis]), _bits(SR.shaded_rgb_f32(unf["rgba"][vis][:, :3], sh[vis], p)))
    assert np.array_equal(_bits(st["alpha"][vis]), _bits(unf["rgba"][vis][:, 3]))


def test_orthographic_and_filter_alone_are_the_float32_restatement():
    st = MS.stack(MS.Point("case_plane", "oblique", aa=True))
    g, cu, su, _, _ = FM.view("case_plane", "oblique")
    want = OR.project_ortho_f32(orc.Camera176.from_buffer_copy(bytes(cu)), su, g["pp"].tex, g["draws"], aa_s=AAR.aa_s(MS.AA_VALUE, su.splat_scale))
    vis = want["visible"] == 1
    assert np.array_equal(st["visible"], vis)
    for fld in MS.GEOMETRY:
        assert np.array_equal(_bits(st["base"][fld][vis]), _bits(want[fld][vis])), fld
    assert np.array_equal(_bits(st["alpha"][vis]), _bits(want["rgba"][vis][:, 3])) and np.array_equal(_bits(st["rgb"][vis]), _bits(want["rgba"][vis][:, :3]))


@pytest.mark.parametrize("cam", ["persp", "oblique"])
def test_tint_shadow_and_fog_are_the_float64_chain(cam):
    st = MS.stack(MS.Point("case_plane", cam, atm="fog", sty=True, shd=True))
    unf = FM.view("case_plane", cam)[4]
    wd = MS.world("case_plane", cam)
    fog_p = AR.params(MS.atmosphere_of(st["point"]))
    assert st["how"] == "rint"
    ids = np.unique(st["sty"][:, :4], axis=0)
    assert len(ids) == 4                                   # three tints and none
    for row in ids:
        m = st["visible"] & (st["sty"][:, :4] == row).all(1)
        tint = tuple(int(x) for x in row) if row[3] else None
        want = SR.chain_codes_f64(unf["rgba"][m][:, :3], tint, wd["sh"][m], wd["p"], wd["dist"][m], fog_p)
        assert m.sum() > 0 and np.array_equal(st["codes"][m], want)
    vis = st["visible"]
    staged = MS.staged_codes_f64(unf["rgba"][vis][:, :3], st["sty"][vis], st["sh"][vis], wd["p"], wd["dist"][vis], fog_p)
    assert np.abs(staged - st["codes"][vis]).max() < 1e-9


# ---- coverage -----------------------------------------------------------------------------------------------------------------------------
def test_the_lattice_launches_all_64_instantiations():
    assert len(set(IDS)) == len(IDS) == 32 + 32 + 7 + 2
    for debug in (True, False):
        seen = {pt.instantiation(debug) for pt in MS.LATTICE}
        assert len(seen) == 64
    assert {pt.atm for pt in MS.LATTICE} == set(MS.ATMS)


# ---- population -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pt", MS.LATTICE, ids=IDS)
def test_populations(pt):
    st = MS.stack(pt)
    pop = MS.populations(st)
    print(f"{pt.id} [{st['how']}] {pt.instantiation(True)}: " + ", ".join(f"{k} {v}" for k, v in pop.items()))
    for k, v in pop.items():
        if k.startswith("discard_"):
            assert v >= 5, (k, v)
        elif k.startswith("alpha_") or "+" in k or k == "ramp_and_dim":
            assert v >= 20, (k, v)
    if pt.case == "case_plane" and pt.fade:
        assert int(MS.draw_index(pt.case)[1].sum()) >= 5 and pop["lod_transition_kept"] >= 10
    if st["how"] == "bound":
        assert pop["masked"] <= AR.MAX_MASKED * pop["visible"]
        assert np.isfinite(st["bound"][st["visible"]]).all() and np.isfinite(st["codes"][st["visible"]]).all()
    elif st["how"] == "rint":
        assert pop["near_half"] <= AR.MAX_MASKED * 3 * pop["visible"]
    assert pop["visible"] >= 50


# ---- order sensitivity ------------------------------------------------------------------------------------------------------------------------
def _both(st, a, b):
    tinted = TR.classes(st["sty"])[2]
    sets = dict(tint=tinted, shadow=st["sh"] != 0, fog=st["F"] > 0)
    return st["visible"] & sets[a] & sets[b]


@pytest.mark.parametrize("pt", CORNERS, ids=[pt.id for pt in CORNERS])
def test_another_order_is_other_bytes(pt):
    st = MS.stack(pt)
    wd = MS.world(pt.case, pt.cam)
    fog_p = AR.params(MS.atmosphere_of(pt))
    dist = np.where(np.isfinite(wd["dist"]), wd["dist"], 0.0)
    rgb0 = st["base"]["rgba"][:, :3]
    true = np.rint(st["codes"])
    for label, order, pair in (("shadow before tint", ("shadow", "tint", "fog"), ("tint", "shadow")), ("fog before shadow", ("tint", "fog", "shadow"), ("shadow", "fog"))):
        wrong = np.rint(MS.codes_f64(rgb0, st["sty"], st["sh"], wd["p"], dist, fog_p, order=order))
        m = _both(st, *pair)
        share = float((np.abs(wrong - true)[m].max(1) > 1.0).mean())
        print(f"{pt.id}: {label}: {int(m.sum())} splats touched by both, {share:.3f} of them more than one code away")
        assert m.sum() >= 20 and share >= 0.2, (label, share)


@pytest.mark.parametrize("cam", ["persp", "oblique"])
def test_a_second_quantisation_is_other_bytes(cam):
    st = MS.stack(MS.Point("case_plane", cam, sty=True, shd=True))
    assert st["how"] == "exact"
    wd = MS.world("case_plane", cam)
    sty, sh, rgb0 = st["sty"], wd["sh"], st["base"]["rgba"][:, :3]
    # the binary32 chain with the tinted floats quantised in between, as a tint_requantise call between the two stages would leave them
    tinted = TR.classes(sty)[2]
    ct = TR.tinted_rgb(rgb0, sty)
    ct = np.where(tinted[:, None], (SR.quantise_f32(ct) / F32(255.0)).astype(F32), ct).astype(F32)
    wrong = SR.shaded_rgb_f32(ct, sh, wd["p"])
    m = _both(st, "tint", "shadow")
    differs = (_bits(wrong[m]) != _bits(st["rgb"][m])).any(1)
    print(f"{cam}: a second quantisation: {int(m.sum())} tinted and shadowed splats, {differs.mean():.3f} of them with another byte")
    assert m.sum() >= 20 and differs.mean() >= 0.2
    codes = lambda c: np.rint(c.astype(np.float64) * 255.0)
    assert np.abs(codes(wrong[m]) - codes(st["rgb"][m])).max() == 1.0
