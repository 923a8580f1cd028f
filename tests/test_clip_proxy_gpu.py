"""The clip volumes in the proxy passes (gswt_proxy_render, gswt_proxy_render_ortho, gswt_proxy_render_sphere in both projections) on
the GPU, against the float64 hit points of the proxy references (tests/clip_ref.py: proxy_scene, proxy_expect; the sets are pinned without
a GPU by tests/test_clip_proxy_cpu.py).

Under a set of volumes flagged GSWT_CLIP_GROUND a pixel whose hit point is hidden beyond the margin holds the clear colour and the clear
depth exactly, a pixel kept beyond it equals the unclipped pass bit for bit, any other pixel may be either, and those are at most 2 % of
the frame.  On the sphere a near surface that is cut away shows the far one: its depth is the reference's second candidate.  Volumes
without the flag, and a set that is switched off, leave the passes byte for byte untouched."""
import numpy as np
import pytest

from gswt_renderer_amd import atmosphere as A
from tests import clip_ref as CR
from tests import frame_modes as FM
from tests import proxy_raster_ref as R

pytestmark = pytest.mark.gpu
MAX_UNDECIDED = 0.02


@pytest.fixture(autouse=True)
def _defaults(renderer):
    """Every test leaves the shared context as it found it."""
    yield
    renderer.set_clip_volumes(None)
    renderer.set_atmosphere(A.OFF)
    renderer.set_shadow_map(None)
    renderer.configure(None)


def _draw(r, sc, volumes):
    """(depth, colour) of the scene's pass over the sky image and a cleared depth buffer, under the set `volumes`."""
    import torch
    W, H = sc["W"], sc["H"]
    r.set_atmosphere(A.OFF)
    r.set_shadow_map(None)
    r.set_clip_volumes(volumes)
    rgba = torch.from_numpy(R.sky(W, H)).cuda()
    depth = torch.zeros((H, W), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    if "cand" in sc:
        r.proxy_configure(sc["mips"], grid_dim=24)
        r.proxy_render_sphere(sc["u"], sc["radius"], W, H, rgba.data_ptr(), depth.data_ptr(), clear_depth=True, projection=sc["projection"])
    else:
        r.configure(sc["hm"])
        r.proxy_configure(sc["mips"], grid_dim=sc["grid_dim"])
        r.proxy_render(sc["us"][0], W, H, rgba.data_ptr(), depth.data_ptr(), clear_depth=True, projection=sc["projection"])
    r.synchronize()
    return depth.cpu().numpy(), rgba.cpu().numpy()


def _check(sc, e, got, plain, label):
    """The clipped pass `got` against the expectation `e` and the unclipped pass `plain`."""
    sky = R.sky(sc["W"], sc["H"])
    (d, c), (d0, c0) = got, plain
    undecided = float(e["undecided"].mean())
    print(f"{label}: clear {int(e['clear'].sum())}, same {int(e['same'].sum())}, far {int(e['far'].sum())}, undecided {undecided:.4f} of {d.size} pixels")
    assert undecided <= MAX_UNDECIDED
    assert (d[e["clear"]] == np.float32(1.0)).all() and FM.same(c[e["clear"]], sky[e["clear"]]), label
    assert FM.same(d[e["same"]], d0[e["same"]]) and FM.same(c[e["same"]], c0[e["same"]]), label
    assert e["clear"].sum() + e["far"].sum() > 0 and (d0[e["clear"]] < 1.0).all()
    if e["far"].any():
        err = np.abs(d[e["far"]].astype(np.float64) - e["far_depth"][e["far"]])
        print(f"{label}: far surface, max depth error {err.max():.3e} (bound {sc['depth_tol']:.3e})")
        assert (err <= sc["depth_tol"]).all() and (d[e["far"]] > d0[e["far"]]).all()
        assert (c[e["far"]][:, 3] == 1.0).all()                                       # a ground fragment, not the sky
    # every pixel, decided or not, is one of the states a fragment can leave: untouched sky, or a written fragment
    untouched = (d == np.float32(1.0))
    assert FM.same(c[untouched], sky[untouched])


@pytest.mark.parametrize("name", ["cut", "keep"])
@pytest.mark.parametrize("kind", CR.PROXY_SCENES)
def test_ground_volumes_cut_the_pass(renderer, kind, name):
    sc = CR.proxy_scene(kind)
    vols = CR.proxy_volumes(sc)[name]
    plain = _draw(renderer, sc, [])
    assert not (np.not_equal(plain[0] < 1.0, sc["hit"]) & ~sc["amb"]).any()       # the unclipped pass covers what the reference covers
    _check(sc, CR.proxy_expect(sc, vols), _draw(renderer, sc, vols), plain, f"{kind} {name}")


def test_a_cut_near_cap_shows_the_far_surface(renderer):
    sc = CR.proxy_scene("sphere_persp")
    vols = CR.proxy_volumes(sc, near_cap=True)["near_cap"]
    e = CR.proxy_expect(sc, vols)
    assert e["far"].sum() >= 0.05 * sc["hit"].sum()
    _check(sc, e, _draw(renderer, sc, vols), _draw(renderer, sc, []), "sphere_persp near cap")


@pytest.mark.parametrize("kind", CR.PROXY_SCENES)
def test_unflagged_volumes_and_a_set_switched_off_leave_the_pass_untouched(renderer, kind):
    sc = CR.proxy_scene(kind)
    sets = CR.proxy_volumes(sc)
    plain = _draw(renderer, sc, None)
    cut = _draw(renderer, sc, sets["cut"])
    assert not FM.same(cut[0], plain[0])
    for label, vols in (("unflagged", sets["unflagged"]), ("empty list", []), ("None", None)):
        got = _draw(renderer, sc, vols)
        assert FM.same(got[0], plain[0]) and FM.same(got[1], plain[1]), (kind, label)
