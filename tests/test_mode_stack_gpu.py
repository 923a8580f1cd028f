"""The frame modes of the strict vertex stage on one another, on the GPU: every one of the 64 (FULL, ORTHO, AA, ATM, STY, SHD) points of
k_project<DEBUG, FULL, STRICT, ORTHO, AA, ATM, STY, SHD> launched as its DEBUG and as its normal instantiation, against the composed
reference of tests/mode_stack_ref.py (pinned without a GPU by tests/test_mode_stack_cpu.py).  Frames are 72 x 40 (tests/ortho_ref.py) on
the three golden cases with the draws of their own perspective sort event.

Each lattice point renders two frames.  The DEBUG_VARYINGS frame's records against the stack: `visible`, n_visible, ndc, depth, both axes
and alpha bit for bit; colour bit for bit, or against the float64 chain as that module says.  Then the normal frame (the DEBUG = false
instantiation over k_cull's live table) with depth, in depth order over a background: the same n_visible and n_pairs, and image, depth
and pick against the CPU references over the GPU's own records (tests/frame_modes.py: image_case).

A test id is <case>-<camera>-<modes>; the instantiation it launches is k_project<DEBUG, FULL, true, ORTHO, AA, ATM, STY, SHD> with

    <case>-<camera>    FULL   ORTHO          <modes>            AA  ATM  STY  SHD        <modes>            AA  ATM  STY  SHD
    plane-persp        0      0              plain              0   0    0    0          aa                 1   0    0    0
    plane-oblique      0      1              shd                0   0    0    1          aa+shd             1   0    0    1
    sphere-persp       1      0              sty                0   0    1    0          aa+sty             1   0    1    0
    sphere-top         1      1              sty+shd            0   0    1    1          aa+sty+shd         1   0    1    1
    hmap-persp         0      0              both               0   1    0    0          aa+both            1   1    0    0
                                             both+shd           0   1    0    1          aa+both+shd        1   1    0    1
                                             both+sty           0   1    1    0          aa+both+sty        1   1    1    0
                                             both+sty+shd       0   1    1    1          aa+both+sty+shd    1   1    1    1

("both": the far fade and the fog together.)  plane-persp, plane-oblique, sphere-persp and sphere-top run all sixteen <modes>;
hmap-persp (the plane's instantiations through map_height_surface) runs aa+both+sty+shd and the six pairs aa+both, aa+sty, aa+shd,
both+sty, both+shd, sty+shd; plane-persp-aa+fade+sty+shd and plane-persp-aa+fog+sty+shd are <0, 0, 1, 1, 1, 1> again with one of ATM's
two uniform branches off.

And what stays off: with exactly one of the four flags off, the records the flag would not touch are those of the all-on frame."""
import dataclasses

import numpy as np
import pytest

from gswt_renderer_amd import _lib as L
from tests import atmosphere_ref as AR
from tests import frame_modes as FM
from tests import mode_stack_ref as MS
from tests import ortho_ref as OR
from tests import tile_style_ref as TR

pytestmark = pytest.mark.gpu
# the share of the frame some splat covers, at least: the sphere fills a sixth of the perspective frame
MIN_COVER = {"case_plane": 0.3, "case_hmap": 0.3, "case_sphere": 0.1}


@pytest.fixture(autouse=True)
def _defaults(renderer):
    """FM.restore_defaults does not know the shadow map: the shared context goes back without one as well."""
    yield
    renderer.set_shadow_map(None)
    FM.restore_defaults(renderer)


@pytest.mark.parametrize("pt", MS.LATTICE, ids=[pt.id for pt in MS.LATTICE])
def test_lattice_point(renderer, pt):
    st = MS.stack(pt)
    print(f"{pt.id}: {pt.instantiation(True)} and DEBUG=0 [{st['how']}]: " + ", ".join(f"{k} {v}" for k, v in MS.populations(st).items()))
    c = FM.image_case(renderer, pt.cam, L.GSWT_ORDER_DEPTH, True, OR.SPLAT_SCALE, MS.render_kw(pt), "stack " + pt.id, min_cover=MIN_COVER[pt.case],
                      name=pt.case)
    print(MS.check_records(c["sp"], c["t_debug"]["n_visible"], st))
    assert (c["t"]["n_visible"], c["t"]["n_pairs"]) == (c["t_debug"]["n_visible"], c["t_debug"]["n_pairs"]) and c["t"]["n_pairs"] > 0


def _untouched(flag, st, wd):
    """Per field, the splats on which the all-on point's flag `flag` does nothing, from the reference."""
    n = st["visible"].shape[0]
    every = np.ones(n, bool)
    if flag == "aa":                                        # the filter is on every splat's axes and alpha, and on nothing else
        return {"ndc": every, "depth": every, "rgb": every}
    if flag == "atm":                                       # alpha where t == 1; colour where the fog has not begun
        pt = st["point"]
        p = AR.params(MS.atmosphere_of(pt))
        with np.errstate(all="ignore"):
            raw = (float(p["fade_end"]) - wd["dist"]) * float(p["fade_inv"])
        slack = MS.t_tolerance(pt, wd)
        reach = wd["delta"] + 8.0 * AR.U * float(p["fog_start"])
        return {**{f: every for f in MS.GEOMETRY}, "alpha": raw - 1.0 > slack, "rgb": wd["dist"] < float(p["fog_start"]) - reach}
    if flag == "sty":
        keep = TR.classes(st["sty"])[3]
    else:
        keep = (st["sh"] == 0) & ~wd["near_ld"]
    return {f: keep for f in MS.GEOMETRY + ("alpha", "rgb")}


def _field(rec, f):
    return rec["rgba"][:, :3] if f == "rgb" else rec["rgba"][:, 3] if f == "alpha" else rec[f]


@pytest.mark.parametrize("flag", ["aa", "atm", "sty", "shd"])
@pytest.mark.parametrize("case,cam", [(case, cam) for case in ("case_plane", "case_sphere") for cam in MS.CAMERAS[case]])
def test_a_flag_that_is_off_leaves_the_others_alone(renderer, case, cam, flag):
    on = MS.corner(case, cam)
    off = dataclasses.replace(on, **{flag: None if flag == "atm" else False})
    g, cu, su, proj, _ = FM.view(case, cam)
    FM.bind(renderer, g)
    a, _ = FM.varyings(renderer, cu, su, projection=proj, **MS.render_kw(on))
    b, _ = FM.varyings(renderer, cu, su, projection=proj, **MS.render_kw(off))
    both = (a["visible"] == 1) & (b["visible"] == 1)
    counts = {}
    for f, m in _untouched(flag, MS.stack(on), MS.world(case, cam)).items():
        m = m & both
        counts[f] = int(m.sum())
        assert FM.bits_equal(np.ascontiguousarray(_field(a, f)[m]), np.ascontiguousarray(_field(b, f)[m])), (on.id, flag, f)
    print(f"{on.id} without {flag}: of {int(both.sum())} splats visible in both frames, bit-identical " + ", ".join(f"{f} {k}" for f, k in counts.items()))
    assert both.sum() >= 50 and max(counts.values()) > 0
    assert not all(FM.bits_equal(np.ascontiguousarray(_field(a, f)[both]), np.ascontiguousarray(_field(b, f)[both])) for f in MS.GEOMETRY + ("alpha", "rgb"))
