"""The clip volumes of the proxy passes without a GPU: the sets tests/test_clip_proxy_gpu.py uses (tests/clip_ref.py: proxy_volumes,
built over the float64 hit points of the proxy references) decide nearly every pixel, and cut through what the passes draw."""
import numpy as np
import pytest

from tests import clip_ref as CR

MAX_UNDECIDED = 0.02


@pytest.mark.parametrize("name", ["cut", "keep"])
@pytest.mark.parametrize("kind", CR.PROXY_SCENES)
def test_ground_sets_decide_the_pixels_and_cut_through_the_pass(kind, name):
    sc = CR.proxy_scene(kind)
    e = CR.proxy_expect(sc, CR.proxy_volumes(sc)[name])
    n_hit = int(sc["hit"].sum())
    shares = {k: float((e[k] & sc["hit"]).sum()) / n_hit for k in ("clear", "same", "far")}
    undecided = float(e["undecided"].mean())
    print(f"{kind} {name}: {n_hit} of {sc['hit'].size} pixels hit; of them clear {shares['clear']:.3f}, same {shares['same']:.3f}, far {shares['far']:.3f}; "
          f"undecided {undecided:.4f} of the frame, largest delta {np.nanmax(sc['delta'][sc['hit']]):.2e}")
    assert undecided <= MAX_UNDECIDED
    assert shares["clear"] + shares["far"] >= 0.10 and shares["same"] >= 0.10
    assert not (e["clear"] & e["same"]).any() and not (e["far"] & (e["same"] | e["clear"])).any()


@pytest.mark.parametrize("kind", ["sphere_persp"])
def test_a_cut_near_cap_leaves_the_far_surface_in_sight(kind):
    sc = CR.proxy_scene(kind)
    e = CR.proxy_expect(sc, CR.proxy_volumes(sc, near_cap=True)["near_cap"])
    print(f"{kind} near cap: far {int(e['far'].sum())}, clear {int(e['clear'].sum())}, same {int((e['same'] & sc['hit']).sum())}, undecided {e['undecided'].mean():.4f}")
    assert e["far"].sum() >= 0.05 * sc["hit"].sum() and e["undecided"].mean() <= MAX_UNDECIDED
    assert (e["far_depth"][e["far"]] > sc["cand"][0]["dep"][e["far"]]).all()


def test_unflagged_volumes_are_not_seen():
    sc = CR.proxy_scene("plane_persp")
    e = CR.proxy_expect(sc, CR.proxy_volumes(sc)["unflagged"])
    assert not e["clear"].any() and np.array_equal(e["same"], ~sc["amb"])
