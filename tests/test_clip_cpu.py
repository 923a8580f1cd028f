"""The clip volumes without a GPU: tests/clip_ref.py pinned by known answers, gswt_renderer_amd/clip.py's constructors and record layout,
the conditions on the volume sets the GPU tests use (checked from the oracle's unclipped records), and project_modes' rule with the
volume count as its seventh input (tools/frame_modes_clip_main.cpp, built by the host compiler alone and run once)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from gswt_renderer_amd import _lib as L
from gswt_renderer_amd import clip as CL
from tests import atmosphere_ref as AR
from tests import clip_ref as CR
from tests import ortho_ref as OR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
V = CL.ClipVolume


def _in32(v, pts):
    p = np.asarray(pts, F32).reshape(-1, 3)
    return CR.inside_f32(CR.params([v])[0], p[:, 0], p[:, 1], p[:, 2]).tolist()


# ---- clip_ref: known answers --------------------------------------------------------------------------------------------------------------
def test_box_known_answers_and_its_boundary():
    box = V.box((1.0, 2.0, 3.0), (2.0, 1.0, 0.5))                # every coefficient exact in binary32
    pts = [(1, 2, 3), (3, 2, 3), (3, 3, 3.5), (3.0000002, 2, 3), (1, 3.0000002, 3), (1, 2, 2.4999998), (-1, 1, 2.5), (-1.0000005, 1, 2.5)]
    assert _in32(box, pts) == [True, True, True, False, False, False, True, False]
    # rotated by 90 degrees about z: the box's x axis is the world's y axis (cos 90 is 6e-17 in float64 and rounds into the rows: inside points only)
    rot = V.box((0.0, 0.0, 0.0), (4.0, 1.0, 1.0), CR.rot_z(90.0))
    assert _in32(rot, [(0, 3.5, 0), (3.5, 0, 0), (0.5, -3.9, 0.9), (1.1, 0, 0)]) == [True, False, True, False]


def test_ellipsoid_known_answers_and_its_boundary():
    e = V.ellipsoid((0.0, 0.0, 0.0), (2.0, 4.0, 8.0))
    pts = [(0, 0, 0), (2, 0, 0), (0, -4, 0), (0, 0, 8), (2.0000002, 0, 0), (1.5, 2.0, 0), (1.5, 3.0, 0), (0, 0, -8.000001)]
    # (1.5 / 2)^2 + (2 / 4)^2 = 0.8125; (1.5 / 2)^2 + (3 / 4)^2 = 1.125
    assert _in32(e, pts) == [True, True, True, True, False, True, False, False]
    unit = V.ellipsoid((0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
    assert _in32(unit, [(0.6, 0.8, 0.0), (0.6, 0.8, 0.001)]) == [bool(F32(0.6) * F32(0.6) + F32(0.8) * F32(0.8) <= F32(1.0)), False]


def test_half_space_inside_is_the_side_the_normal_points_away_from():
    h = V.half_space((0.0, 0.0, 2.0), (0.0, 0.0, 4.0))           # normalised: u2 = z - 2
    assert _in32(h, [(5, 5, 2), (0, 0, 1.9999999), (0, 0, 2.0000002), (-7, 9, -100)]) == [True, True, False, True]
    p = CR.params([h])[0]
    assert p["shape"] == CL.HALFSPACE and (p["M"][:2] == 0).all() and p["M"][2].tolist() == [0.0, 0.0, 1.0, -2.0]
    # rows 0 and 1 are not read: whatever they hold, the answer is row 2's
    junk = V(np.concatenate([np.full(8, 1e30), h.world_to_unit[8:]]), CL.HALFSPACE)
    assert _in32(junk, [(5, 5, 2), (0, 0, 2.0000002)]) == [True, False]
    tilted = V.half_space((1.0, 1.0, 1.0), (1.0, 1.0, 0.0))
    assert _in32(tilted, [(0, 0, 50), (3, 3, -50), (2, 0, 0), (2.1, 0, 0)]) == [True, False, True, False]


def test_nan_is_not_inside_and_f64_agrees_off_the_boundary():
    vols = CR.params([V.box((0, 0, 0), (1, 1, 1)), V.ellipsoid((0, 0, 0), (1, 1, 1)), V.half_space((0, 0, 0), (0, 0, 1))])
    nan = F32(np.nan)
    for v in vols:
        for k in range(3):
            c = [np.zeros(1, F32), np.zeros(1, F32), np.full(1, -0.5, F32)]
            c[k] = np.full(1, nan)
            # (a half-space reads row 2 alone, whose x and y coefficients are 0: 0 * NaN is NaN all the same)
            assert not CR.inside_f32(v, *c)[0] and not CR.inside_f64(v, *c)[0]
    # a NaN point is inside no keep volume (hidden) and inside no cut volume (kept when there are only cuts)
    keep, cut = CR.params([V.box((0, 0, 0), (1, 1, 1), keep=True)]), CR.params([V.box((0, 0, 0), (1, 1, 1))])
    c = [np.full(1, nan), np.zeros(1, F32), np.zeros(1, F32)]
    assert CR.hidden(keep, *c)[0] and not CR.hidden(cut, *c)[0]
    rng = np.random.default_rng(5)
    p = rng.uniform(-2, 2, (4000, 3))
    for v in vols:
        far = np.abs(CR.boundary_f64(v, p)) > 1e-5
        a = CR.inside_f32(v, *p.astype(F32).T)
        assert np.array_equal(a[far], CR.inside_f64(v, *p.T)[far]) and 0.05 < a.mean() < 0.95
        assert np.array_equal(CR.inside_f64(v, *p.T), CR.boundary_f64(v, p) <= 0)


def test_keep_and_cut_rule_with_zero_one_and_two_keeps():
    x = np.arange(-5.0, 6.0).astype(F32)                           # points on the x axis, -5 .. 5
    zero = np.zeros_like(x)
    hid = lambda vols: CR.hidden(CR.params(vols), x, zero, zero).astype(int).tolist()
    cut = V.box((0, 0, 0), (1, 9, 9))                              # hides -1 .. 1
    k1 = V.box((-3, 0, 0), (1, 9, 9), keep=True)                   # keeps -4 .. -2
    k2 = V.ellipsoid((2, 0, 0), (2, 9, 9), keep=True)              # keeps 0 .. 4
    assert hid([]) == [0] * 11
    assert hid([cut]) == [0, 0, 0, 0, 1, 1, 1, 0, 0, 0, 0]
    assert hid([k1]) == [1, 0, 0, 0, 1, 1, 1, 1, 1, 1, 1]
    assert hid([k1, k2]) == [1, 0, 0, 0, 1, 0, 0, 0, 0, 0, 1]
    assert hid([k2, cut, k1]) == [1, 0, 0, 0, 1, 1, 1, 0, 0, 0, 1]   # a cut wins inside a keep; the order does not matter
    g = V.box((0, 0, 0), (1, 9, 9), ground=True)
    assert CR.hidden(CR.params([g, k1]), x, zero, zero, ground_only=True).astype(int).tolist() == hid([cut])


# ---- clip.py ----------------------------------------------------------------------------------------------------------------------------------
def test_pack_is_the_64_byte_record():
    v = V(np.arange(1.0, 13.0), CL.ELLIPSOID, CL.KEEP | CL.GROUND)
    raw = CL.pack([v, V.half_space((0, 0, 0), (0, 0, 1))])
    assert len(raw) == 128 and C.sizeof(L.ClipVolume) == CL.VOLUME_BYTES == 64
    rec = (L.ClipVolume * 2).from_buffer_copy(raw)
    assert list(rec[0].world_to_unit) == [float(k) for k in range(1, 13)] and (rec[0].shape, rec[0].flags) == (1, 3)
    assert list(rec[0].reserved) == [0, 0] and (rec[1].shape, rec[1].flags) == (CL.HALFSPACE, 0)
    assert (L.ClipVolume.shape.offset, L.ClipVolume.flags.offset, L.ClipVolume.reserved.offset) == (48, 52, 56)
    assert (L.GSWT_CLIP_BOX, L.GSWT_CLIP_ELLIPSOID, L.GSWT_CLIP_HALFSPACE) == (CL.BOX, CL.ELLIPSOID, CL.HALFSPACE)
    assert (L.GSWT_CLIP_KEEP, L.GSWT_CLIP_GROUND, L.GSWT_MAX_CLIP_VOLUMES) == (CL.KEEP, CL.GROUND, CL.MAX_VOLUMES)
    assert CL.pack([]) == b""
    with pytest.raises(ValueError):
        CL.pack([v] * 9)
    with pytest.raises(TypeError):
        CL.pack([b"\0" * 64])
    for bad in (lambda: V(np.zeros(11), CL.BOX), lambda: V(np.zeros(12), 3), lambda: V(np.zeros(12), CL.BOX, 4),
                lambda: V(np.full(12, np.inf), CL.BOX), lambda: V.box((0, 0, 0), (1, 0, 1)), lambda: V.half_space((0, 0, 0), (0, 0, 0))):
        with pytest.raises(ValueError):
            bad()


def test_header_states_the_contract():
    hdr = open(os.path.join(ROOT, "include", "gswt_hip.h")).read()
    for line in ("#define GSWT_MAX_CLIP_VOLUMES 8", "#define GSWT_CLIP_BOX        0u", "#define GSWT_CLIP_ELLIPSOID  1u", "#define GSWT_CLIP_HALFSPACE  2u",
                 "#define GSWT_CLIP_KEEP    1u", "#define GSWT_CLIP_GROUND  2u",
                 "GSWT_API int gswt_set_clip_volumes(gswt_ctx *ctx, const gswt_clip_volume *v, size_t n);"):
        assert line in hdr, line


# ---- the conditions on the GPU tests' inputs --------------------------------------------------------------------------------------------------
POINTS = [(case, cam, name) for case, cams in CR.CASE_CAMERAS.items() for cam in cams for name in CR.SET_NAMES]


def _members_on_both_sides(case, hid, msk, vis):
    n_both, o = 0, 0
    for d in OR.golden(case)["draws"]:
        s = slice(o, o + len(np.asarray(d.gs_index)))
        o = s.stop
        n_both += d.tile.single_draw == 1 and bool((hid[s] & ~msk[s]).any()) and bool((vis[s] & ~hid[s] & ~msk[s]).any())
    return n_both


@pytest.mark.parametrize("case,cam,name", POINTS, ids=["-".join(p) for p in POINTS])
def test_volume_sets_cut_through_the_frames_they_are_used_on(case, cam, name):
    vols = CR.volume_sets(case)[name]
    assert len(vols) == (8 if name == "eight" else 1)
    if name == "eight":
        assert sum(v.keep for v in vols) == 2 and {v.shape for v in vols if not v.keep} == {CL.BOX, CL.ELLIPSOID, CL.HALFSPACE}
    hid, msk, unf = CR.expected(case, cam, vols)
    vis = unf["visible"] == 1
    n = int(vis.sum())
    hid, msk = hid & vis, msk & vis
    share_hidden, share_kept, share_masked = hid.sum() / n, (vis & ~hid).sum() / n, msk.sum() / n
    both = _members_on_both_sides(case, hid, msk, vis)
    print(f"{case} {cam} {name}: {n} visible, hidden {share_hidden:.3f}, masked {share_masked:.4f}, merged draws on both sides {both}")
    assert share_hidden >= 0.10 and share_kept >= 0.10
    assert share_masked <= AR.MAX_MASKED
    assert both >= 1
    assert case != "case_plane" or not msk.any()                    # the plain surface is exact: no mask
    # ground = True changes the flag alone
    assert [(v.shape, v.flags & ~CL.GROUND) for v in CR.volume_sets(case, ground=True)[name]] == [(v.shape, v.flags) for v in vols]


@pytest.mark.parametrize("case,cam", [(c, cam) for c, cams in CR.CASE_CAMERAS.items() for cam in cams])
def test_the_two_exempt_sets_hide_everything_and_nothing(case, cam):
    sets = CR.volume_sets(case)
    hid, msk, unf = CR.expected(case, cam, sets["all"])
    vis = unf["visible"] == 1
    assert np.array_equal(hid & vis, vis) and not (msk & vis).any()
    hid, msk, _ = CR.expected(case, cam, sets["none"])
    assert not hid.any() and not (msk & vis).any()


# ---- project_modes with the volume count as an input --------------------------------------------------------------------------------------------
def test_project_modes_holds_over_all_128_inputs(tmp_path):
    exe = tmp_path / "frame_modes_clip"
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "gswt_renderer_amd", "csrc"),
           os.path.join(ROOT, "tools", "frame_modes_clip_main.cpp"), "-o", str(exe)]
    subprocess.run(cmd, check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0 and not out.stderr, (out.stdout[-2000:], out.stderr[-2000:])
    assert out.stdout.splitlines() == ["project_modes: 128 inputs, 64 strict outputs"]
