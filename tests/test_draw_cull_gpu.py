"""The per-draw viewport cull and LOD-enable mask of k_cull (draw_is_culled, renderer.rs:472-497) on the GPU, against
tests/draw_cull_ref.py and the oracle's draw loop: culling_dist and lod_enable_mask swept over the three ways a draw list reaches
the device, single-ulp knife edges, hand-made corners (behind the eye, w = 0, NaN, the z branch), and the same two fields through
the frame variants that carry a Frame (graph node updates, frames in flight, overflow re-runs, depth order, shards, depth / pick
output, the orthographic projection, the chunk cull).

How a decision is observed: with GSWT_OPT_DEBUG_VARYINGS (and GSWT_OPT_NO_LOD_PREFILTER, so that the lists are the oracle's) the
"visible" flags of gswt_debug_read_projected hold one entry per list entry of every submitted draw, culled or not; a culled draw's
entries are all 0.  Only a draw with at least one visible entry is evidence: each test prints how many it saw.  tests/
test_draw_cull_cpu.py pins the reference and the scene (46 draws, 13 of them with visible entries: 10 cull-enabled, 3 merged)."""
import contextlib
import ctypes as C
import functools

import numpy as np
import pytest

from gswt_renderer_amd import _lib as L
from gswt_renderer_amd import host, ortho
from gswt_renderer_amd.pipeline import GSWTPipeline
from gswt_renderer_amd.renderer import PICK_NONE, make_draw
from gswt_renderer_amd.worker import DeviceWorker
from oracle import gswt_oracle as orc
from tests import draw_cull_ref as R
from tests import helpers as H

pytestmark = pytest.mark.gpu
TOL = 1e-4
W, Hh = R.W, R.H
ALL = 0xFFFFFFFF
PATHS = ("set_draws", "merge_groups", "worker")
DEBUG = dict(NO_LOD_PREFILTER=1, DEBUG_VARYINGS=1)


def _c_float(x):
    """The binary32 x as the Python float ctypes stores unchanged (checked: same bits after the store)."""
    v = float(np.float32(x))
    if not np.isnan(v):
        assert R.f32_bits(C.c_float(v).value) == R.f32_bits(x)
    return v


@functools.lru_cache(maxsize=1)
def _camera():
    cu, vp = host.camera_uniforms(R.CAM[0], R.CAM[1], (0, 0, 1), 45.0, 0.1, 2400.0, W, Hh)
    assert np.array_equal(np.asarray(vp, np.float32).view(np.uint32), R.scene().vp.view(np.uint32))     # the matrix the terms were taken with
    return cu, vp


@contextlib.contextmanager
def _bound(renderer, path):
    """The scene's draw list made current on the shared renderer through one of the three submission paths."""
    sc = R.scene()
    cu, vp = _camera()
    pos = R.CAM[0]
    pipe = GSWTPipeline(sc.verts, host.user_data(**R.CFG), renderer=renderer, device_merge=path != "set_draws")
    dw = None
    try:
        if path == "worker":
            dw = DeviceWorker(renderer, pipe.wang)
            pipe.wang.check_update(pos)
            pipe.wang.build_tiles(pos)
            dw.build_tiles(pos)
            dw.sort_tiles(pos, vp)
            dw.swap_in()                                          # gswt_set_draws_from_worker
        else:
            pipe.update(pos, vp)                                  # gswt_set_draws / gswt_set_draws_merge_groups
            assert [int(d.tile.map_index) for d in pipe.sort.draws] == sc.map_index
        yield pipe
    finally:
        if dw is not None:
            renderer.synchronize()
            dw.close()


@functools.lru_cache(maxsize=1)
def _full():
    """vs_main over all 46 draws (culling_dist = inf): the visible flags, each draw's entry range and visible count."""
    sc = R.scene()
    want = orc.project_draws(sc.cam.uniforms(), sc.su, sc.pp.tex, sc.all_draws)
    off = np.concatenate([[0], np.cumsum([len(d.gs_index) for d in sc.all_draws])]).astype(np.int64)
    nvis = [int(want["visible"][off[i]:off[i + 1]].sum()) for i in range(len(sc.all_draws))]
    assert sum(1 for n in nvis if n > 0) == 13
    return want["visible"].copy(), off, nvis


def _expected_visible(keep):
    vis, off, _ = _full()
    out = vis.copy()
    for i, k in enumerate(keep):
        if not k:
            out[off[i]:off[i + 1]] = 0
    return out


_ORACLE_FRAMES = {}


def _oracle_frame(keep):
    """orc.render over the kept draws (computed once per keep set)."""
    key = tuple(bool(k) for k in keep)
    if key not in _ORACLE_FRAMES:
        sc = R.scene()
        draws = [d for d, k in zip(sc.all_draws, key) if k]
        _ORACLE_FRAMES[key] = orc.render(sc.cam.uniforms(), sc.su, sc.pp.tex, draws, W, Hh)
    return _ORACLE_FRAMES[key]


def _evidence(keep):
    """(kept, dropped, kept with visible entries, dropped with visible entries)."""
    _, _, nvis = _full()
    kept, dropped = sum(1 for k in keep if k), sum(1 for k in keep if not k)
    return kept, dropped, sum(1 for k, n in zip(keep, nvis) if k and n), sum(1 for k, n in zip(keep, nvis) if not k and n)


def _debug_visible(renderer, pipe_or_none, cu, su, w, h, cd, mask, **kw):
    if pipe_or_none is not None:
        pipe_or_none.render(cu, w, h, culling_dist=cd, lod_enable_mask=mask, **kw)
    else:
        renderer.render(cu, su, w, h, culling_dist=cd, lod_enable_mask=mask, **kw)
    return renderer.read_projected()["visible"].copy()


# ---- a + b. culling_dist and LOD masks over the three submission paths ------------------------------------------------------------
SWEEP = ([(cd, ALL) for cd, _ in R.CULL_DISTS] + [(1.0, m) for m, _ in R.LOD_MASKS] + [(1.0, m | 0xFFFFFFF8) for m in range(8)] +
         [(1.0, 0xFFFFFFF8), (0.5, 5), (0.25, 2)])
SWEEP_IDS = [f"cd={cd!r}-mask={m:#x}" for cd, m in SWEEP]


@pytest.fixture(scope="module")
def sweep(renderer):
    """Every (culling_dist, mask) of SWEEP through every path: the visible flags of the debug frame, and image + counts of the plain
    frame.  Two binds and 2 x len(SWEEP) small frames per path; the tests below only compare."""
    cu, _ = _camera()
    out = {}
    for path in PATHS:
        with _bound(renderer, path) as pipe:
            plain = []
            for cd, mask in SWEEP:
                img = pipe.render(cu, W, Hh, culling_dist=_c_float(cd), lod_enable_mask=mask)
                t = renderer.timings()
                plain.append((img, {k: t[k] for k in ("n_draws", "n_instanced", "n_visible", "n_pairs")}))
        with renderer.options(**DEBUG):
            with _bound(renderer, path) as pipe:
                flags = [_debug_visible(renderer, pipe, cu, None, W, Hh, _c_float(cd), mask) for cd, mask in SWEEP]
        out[path] = (flags, plain)
    return out


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("k", range(len(SWEEP)), ids=SWEEP_IDS)
def test_sweep_decisions_match_the_reference(sweep, path, k):
    sc = R.scene()
    cd, mask = SWEEP[k]
    keep = sc.ref_keep(cd, mask)
    kept_ids = [int(d.tile.map_index) for d in sc.oracle_draws(cd, mask)]
    assert kept_ids == [mi for mi, kp in zip(sc.map_index, keep) if kp]                # the reference is the oracle's draw loop
    if mask & 7 == 7:                                                                   # merged draws survive every culling_dist
        assert all(kp for kp, kind in zip(keep, sc.kind) if kind == "merged")
    flags, plain = sweep[path]
    print(f"{path} culling_dist={cd!r} mask={mask:#x}: kept {_evidence(keep)[0]}, dropped {_evidence(keep)[1]}; with visible entries: "
          f"kept {_evidence(keep)[2]}, dropped {_evidence(keep)[3]}")
    want = _expected_visible(keep)
    assert flags[k].shape == want.shape
    assert np.array_equal(flags[k], want)                                              # element for element
    img, t = plain[k]
    ref, st = _oracle_frame(keep)
    assert t["n_draws"] == 46                                                           # culling does not shrink the set
    assert t["n_visible"] == st["n_visible"]
    assert t["n_pairs"] == st["n_pairs16"]
    assert H.max_abs_diff(img, ref) <= TOL


def test_sweep_is_not_vacuous(sweep):
    """What the sweep can see: below culling_dist 1 and under every mask but 7, draws with visible entries are dropped."""
    sc = R.scene()
    for (cd, _), dropped_visible in zip(R.CULL_DISTS, (10, 6, 4, 2, 0, 0, 0, 0, 0, 0, 10)):
        assert _evidence(sc.ref_keep(cd, ALL))[3] == dropped_visible, cd
    for (mask, _), dropped_visible in zip(R.LOD_MASKS, (13, 11, 8, 6, 7, 5, 2, 0)):
        assert _evidence(sc.ref_keep(1.0, mask))[3] == dropped_visible, mask
    # a blending draw that reads the list of LOD - 1 and has visible entries: LOD 1 alone keeps it, LOD 0 alone drops it
    _, _, nvis = _full()
    blend = [i for i, d in enumerate(sc.all_draws) if d.base is not None and d.base[0] != sc.lod[i] and nvis[i] > 0]
    assert blend and all(sc.ref_keep(1.0, 1 << sc.lod[i])[i] and not sc.ref_keep(1.0, 1 << sc.all_draws[i].base[0])[i] for i in blend)
    merged = [i for i, kind in enumerate(sc.kind) if kind == "merged"]
    assert all(nvis[i] > 0 for i in merged)
    flags = sweep["set_draws"][0]
    assert len({f.tobytes() for f in flags[:5]}) == 5                                   # culling_dist 0 .. 1: five different frames
    assert len({f.tobytes() for f in flags[11:19]}) == 8                                # eight masks: eight different frames


@pytest.mark.parametrize("k", range(len(SWEEP)), ids=SWEEP_IDS)
def test_sweep_paths_agree_bit_for_bit(sweep, k):
    f0, p0 = sweep[PATHS[0]]
    for path in PATHS[1:]:
        f, p = sweep[path]
        assert np.array_equal(f[k], f0[k]), path
        assert p[k][1] == p0[k][1], path
        assert np.array_equal(p[k][0].view(np.uint32), p0[k][0].view(np.uint32)), path


def test_mask_bits_above_the_scenes_lods_change_nothing(sweep):
    flags, plain = sweep["set_draws"]
    for m in range(8):
        a, b = SWEEP.index((1.0, m)), SWEEP.index((1.0, m | 0xFFFFFFF8))
        assert np.array_equal(flags[a], flags[b]) and np.array_equal(plain[a][0], plain[b][0]), m
    a, b = SWEEP.index((1.0, 0)), SWEEP.index((1.0, 0xFFFFFFF8))
    assert np.array_equal(flags[a], flags[b]) and not flags[b].any() and not plain[b][0].any()


# ---- hand-made draws: a small grid the default camera sees, one short static list per draw ------------------------------------------
def _hand_case(pp, n, overrides=None):
    """n plain LOD-0 draws on the cells (ix, iy), ix = -2 .. 2, iy = 3 .., rows far to near; overrides[i] replaces add_static arguments of draw i."""
    case = H.Case(pp)
    cells = [(ix, iy) for iy in range(7, 2, -1) for ix in range(-2, 3)]
    assert n <= len(cells)
    for i in range(n):
        ix, iy = cells[i]
        args = dict(lod=0, tile=(3 * i + 1) % pp.n_tile, view=2, offset=(ix * 4.0, iy * 4.0, 0.0), valid_lod_id=0, map_index=i,
                    map_coord=(ix + 2, iy - 3))
        args.update((overrides or {}).get(i, {}))
        case.add_static(**args)
    return case


def _hand_pp():
    return H.tileset(n_lod=2, n_tile=16, lod0_count=300)


def _ranges(case):
    return np.concatenate([[0], np.cumsum([len(d.gs_index) for d in case.orc_draws])]).astype(np.int64)


def _check_hand_frames(renderer, case, cam_u, su, vp, frames, w, h, keep_of, projection=None):
    """Each (culling_dist, mask) of `frames` on the bound case: visible flags == vs_main with the dropped draws zeroed, and the image
    against orc.render over the kept draws (perspective only).  keep_of(i, cd, mask) -> bool.  Returns per frame (keep, visible counts)."""
    kw = {} if projection is None else dict(projection=projection)
    pp = case.pp
    n = len(case.orc_draws)
    off = _ranges(case)
    plain = []
    case.upload(renderer)
    for cd, mask in frames:
        img = renderer.render(cam_u, su, w, h, culling_dist=_c_float(cd), lod_enable_mask=mask, **kw)
        plain.append((img, renderer.timings()))
    with renderer.options(**DEBUG):
        case.upload(renderer)
        got = [_debug_visible(renderer, None, cam_u, su, w, h, _c_float(cd), mask, **kw) for cd, mask in frames]
        if projection is None:
            full = orc.project_draws(cam_u, su, pp.tex, case.orc_draws)["visible"]
        else:
            full = _debug_visible(renderer, None, cam_u, su, w, h, float("nan"), ALL, **kw)     # nothing culled: the GPU's own vertex stage
    nvis = [int(full[off[i]:off[i + 1]].sum()) for i in range(n)]
    seen = []
    for (cd, mask), flags, (img, t) in zip(frames, got, plain):
        keep = [keep_of(i, cd, mask) for i in range(n)]
        want = full.copy()
        for i, k in enumerate(keep):
            if not k:
                want[off[i]:off[i + 1]] = 0
        assert np.array_equal(flags, want), (cd, mask, [i for i in range(n) if not np.array_equal(flags[off[i]:off[i + 1]], want[off[i]:off[i + 1]])])
        assert t["n_draws"] == len(case.draws)
        assert t["n_visible"] == int(want.sum())
        if projection is None:
            ref, st = orc.render(cam_u, su, pp.tex, [d for d, k in zip(case.orc_draws, keep) if k], w, h)
            assert t["n_visible"] == st["n_visible"] and t["n_pairs"] == st["n_pairs16"]
            assert H.max_abs_diff(img, ref) <= TOL, (cd, mask)
        seen.append((keep, nvis))
    return seen


def test_lod_field_of_31_and_beyond_wraps(renderer):
    """gswt_draw.lod is what the mask indexes -- not base_lod, not tile_id -- and bit (lod & 31) decides (include/gswt_hip.h); the
    reference would panic at lod >= lod_enable.len()."""
    pp = _hand_pp()
    # draws 5, 6: blending draws of LOD 1 reading the list of LOD 0 (base_lod = lod - 1): their bit is that of LOD 1
    blend = dict(lod=1, base_lod=0, valid_lod_id=-1, changing=1, changing_to_lower=0)
    case = _hand_case(pp, 10, {5: blend, 6: blend})
    lods = [0, 1, 31, 32, 33, 1, 1, 0, 31, 33]
    for d, l in zip(case.draws, lods):
        d.lod = l
    renderer.configure(None)
    W2, H2 = 160, 96
    cam = orc.default_camera(W2, H2)
    su = orc.scene_uniforms(num_lod=pp.n_lod, map_half_wh=(2, 2))
    frames = [(1.0, m) for m in (ALL, 0, 1, 2, 3, 1 << 31, (1 << 31) | 2, ~(1 << 31) & ALL, 0xFFFFFFFC)]
    seen = _check_hand_frames(renderer, case, cam.uniforms(), su, cam.view_proj(), frames, W2, H2,
                              lambda i, cd, mask: R.lod_kept(mask, lods[i]))
    nvis = seen[0][1]
    assert all(n > 0 for n in nvis), nvis                                               # every draw is evidence
    by_mask = {m: keep for (_, m), (keep, _) in zip(frames, seen)}
    assert by_mask[1] == [l in (0, 32) for l in lods] and by_mask[2] == [l in (1, 33) for l in lods]
    assert by_mask[1 << 31] == [l == 31 for l in lods]
    for (_, m), (keep, _) in zip(frames, seen):
        print(f"lod wrap mask={m:#x}: kept {sum(keep)}, dropped {len(keep) - sum(keep)} of {len(keep)} draws, all with visible entries")


def _persp_point(cam, nx, ny, d):
    """The world point at distance d along the default camera's axis (+y from (0, 0, 5)) that lands near NDC (nx, ny)."""
    p0, p5 = float(cam.projection[0]), float(cam.projection[5])
    return (nx * d / p0, d, 5.0 + ny * d / p5)


def _hand_corners(cam):
    """name -> four world corners, for the default perspective camera (near 0.1: NDC z is 0 at twice the near distance)."""
    P = lambda nx, ny, d: _persp_point(cam, nx, ny, d)
    nan, inf = float("nan"), float("inf")
    in_view = [P(0.3, 0.3, 10), P(-0.3, 0.3, 10), P(-0.3, -0.3, 12), P(0.3, -0.3, 12)]
    x_out = [P(1.5, 0.0, 10), P(2.5, 0.1, 10), P(2.0, -0.1, 12), P(1.7, 0.0, 9)]
    y_out = [P(0.0, 1.5, 10), P(0.1, 2.5, 10), P(-0.1, 2.0, 12), P(0.0, 1.7, 9)]
    sets = {
        "in_view": in_view, "x_out": x_out, "y_out": y_out,
        "x_half": [P(0.5, 0.0, 10), P(0.8, 0.1, 10), P(0.9, -0.1, 12), P(0.7, 0.0, 8)],
        "y_half": [P(0.0, 0.5, 10), P(0.1, 0.8, 10), P(-0.1, 0.9, 12), P(0.0, 0.7, 8)],
        "both_out": [P(1.5, 1.5, 10), P(2.5, 2.0, 10), P(2.0, 1.7, 12), P(1.7, 2.2, 9)],
        "straddle": [P(-0.4, 0.2, 10), P(0.6, 0.2, 10), P(0.6, 0.5, 12), P(-0.4, 0.5, 12)],
        # all four corners between the eye and twice the near distance: mz < 0; one of them on the axis: mx = my = 0 -- the z term alone
        "near_z_only": [P(0.0, 0.0, 0.15), P(0.2, 0.1, 0.12), P(-0.1, 0.2, 0.17), P(0.1, -0.1, 0.13)],
        "near_z_mixed": [P(0.0, 0.0, 0.15), P(0.0, 0.0, 0.12), P(0.0, 0.0, 0.3), P(0.0, 0.0, 0.18)],
        "near_z_deep": [P(0.0, 0.0, 0.101), P(0.1, 0.0, 0.105), P(0.0, 0.1, 0.11), P(-0.1, -0.1, 0.102)],
        "inside_near": [P(0.0, 0.0, 0.05), P(0.1, 0.0, 0.04), P(0.0, 0.1, 0.06), P(-0.1, -0.1, 0.05)],
        "beyond_far": [P(0.0, 0.0, 3000.0), P(0.2, 0.0, 3100.0), P(0.0, 0.2, 2900.0), P(-0.2, -0.2, 3000.0)],
        # behind the eye: w < 0
        "behind_on_axis": [P(0.0, 0.0, -1.0), P(0.1, 0.0, -2.0), P(0.0, 0.1, -1.5), P(-0.1, -0.1, -1.0)],
        "behind_off_axis": [P(1.5, 0.0, -1.0), P(2.5, 0.1, -2.0), P(2.0, -0.1, -1.5), P(1.7, 0.0, -1.0)],
        # w exactly 0: a corner in the plane y = 0 through the eye; the eye itself: 0 / 0
        "w_zero_one_in_view": [(1.0, 0.0, 6.0)] + in_view[1:],
        "w_zero_one_out": [(1.0, 0.0, 6.0)] + x_out[1:],
        "w_zero_all": [(1.0, 0.0, 6.0), (-1.0, 0.0, 6.0), (2.0, 0.0, 4.0), (-3.0, 0.0, 7.0)],
        "eye_corner": [(0.0, 0.0, 5.0)] + in_view[1:],
        "nan_one_in_view": [(nan, in_view[0][1], in_view[0][2])] + in_view[1:],
        "nan_z_one_out": [x_out[0], (x_out[1][0], x_out[1][1], nan)] + x_out[2:],
        "nan_all": [(nan, nan, nan)] * 4,
        "inf_coord": [(inf, 10.0, 5.0)] + in_view[1:],
        "huge": [(3e38, 3e38, 3e38)] + y_out[1:],
        # terms of denormal size: on the axis up to a few denormal steps of x
        "denormal_x": [P(1e-44, 0.0, 10), P(2e-44, 0.0, 10), P(3e-44, 0.0, 12), P(4e-44, 0.0, 9)],
    }
    return sets


HAND_CLIPS = [0.0, -0.0, 1e-45, -1e-45, 0.25, 1.0, 3.5, float("inf"), float("-inf"), float("nan")]


def test_hand_made_corners(renderer):
    """The rule on corners no real tile has, each draw one short list the camera sees, at +-0, denormal, ordinary, infinite and NaN
    culling_dist; a merged draw with count = 0 (and cull_enable = 1) rides along.  Expectations from draw_cull_ref alone."""
    pp = _hand_pp()
    W2, H2 = 160, 96
    cam = orc.default_camera(W2, H2)
    vp = cam.view_proj()
    sets = _hand_corners(cam)
    names = list(sets)
    assert len(names) == 24
    corners = [np.asarray(sets[nm], dtype=np.float32) for nm in names]
    case = _hand_case(pp, len(names), {i: dict(corners=c) for i, c in enumerate(corners)})
    # count = 0: no list entry, no chunk; the frame and the other draws are untouched
    tu = orc.tile_uniforms(single_draw=1, map_index=24, single_lod_id=0, tile_id=(0, 0, 2))
    case.draws.append(make_draw(H.to_product_tile(tu), merged_range=(0, 0), corners=corners[names.index("x_out")], lod=0))
    assert case.draws[-1].merged_count == 0 and case.draws[-1].cull_enable == 1
    terms = [R.cull_terms(vp, c) for c in corners]
    t_of = dict(zip(names, terms))
    assert t_of["near_z_only"][0] == 0 and t_of["near_z_only"][1] == 0 and t_of["near_z_only"][2] < 0
    assert t_of["near_z_mixed"][2] > 0 and t_of["behind_on_axis"][2] > 1 and t_of["nan_all"] == (R.FLT_MAX, R.FLT_MAX, -R.FLT_MAX)
    assert 0 < t_of["denormal_x"][0] < np.finfo(np.float32).tiny
    renderer.configure(None)
    su = orc.scene_uniforms(num_lod=pp.n_lod, map_half_wh=(2, 2))
    frames = [(cd, ALL) for cd in HAND_CLIPS]
    seen = _check_hand_frames(renderer, case, cam.uniforms(), su, vp, frames, W2, H2, lambda i, cd, mask: R.keeps(terms[i], cd))
    nvis = seen[0][1]
    assert all(n > 0 for n in nvis), dict(zip(names, nvis))
    # the reference yields both outcomes for each term: alone (the other two silent) and silent, on draws with visible entries
    alone = {"x": 0, "y": 0, "z": 0}
    quiet = 0
    with np.errstate(all="ignore"):
        for cd in HAND_CLIPS:
            clip = np.float32(cd)
            for mx, my, mz in terms:
                fires = {"x": bool(mx > clip), "y": bool(my > clip), "z": bool(mz < -clip)}
                quiet += int(not any(fires.values()))
                for k in alone:
                    alone[k] += int(fires[k] and sum(fires.values()) == 1)
    assert min(alone.values()) >= 3 and quiet >= 20, (alone, quiet)
    for cd, (keep, _) in zip(HAND_CLIPS, seen):
        print(f"hand-made culling_dist={cd!r}: kept {sum(keep)}, dropped {len(keep) - sum(keep)} of {len(keep)} draws, all with visible entries")
    by_cd = {repr(cd): dict(zip(names, keep)) for cd, (keep, _) in zip(HAND_CLIPS, seen)}
    assert not by_cd["0.0"]["near_z_only"] and by_cd["0.0"]["near_z_mixed"] and by_cd["1.0"]["near_z_only"]
    assert all(by_cd["nan"].values()) and not any(by_cd["-inf"].values())
    assert by_cd["1e-45"]["near_z_mixed"] and not by_cd["1e-45"]["denormal_x"]          # a denormal bound is not flushed to zero
    assert by_cd["1.0"]["behind_on_axis"] and not by_cd["1.0"]["behind_off_axis"]


# ---- c. knife edges on the GPU -----------------------------------------------------------------------------------------------------
def _knife_draws():
    """Cull-enabled draws for the knife-edge frames: every draw with visible entries (8 with a g of their own, and the two that share
    one), then draws without visible entries up to four per (governing axis, class) -- their frames must still equal the reference."""
    sc = R.scene()
    _, _, nvis = _full()
    idx = [i for i, ce in enumerate(sc.cull_enable) if ce]
    bits = [R.f32_bits(sc.g(i)) for i in idx]
    unique = [i for i, b in zip(idx, bits) if bits.count(b) == 1]
    observable = [i for i in idx if nvis[i] > 0]
    chosen = list(observable)
    per_class = {}
    for i in unique:
        key = ("x" if sc.terms[i][0] >= sc.terms[i][1] else "y", sc.kind[i])
        if i in chosen or per_class.get(key, 0) >= 2:
            continue
        per_class[key] = per_class.get(key, 0) + 1
        chosen.append(i)
    return chosen, unique, observable


@pytest.mark.parametrize("path", PATHS)
def test_knife_edges(renderer, path):
    """culling_dist = g = max(mx, my) of a draw keeps it, the next binary32 toward zero drops it: the two frames' visible flags differ
    in exactly that draw's visible entries (for the two draws that share a g: in both)."""
    sc = R.scene()
    vis, off, nvis = _full()
    chosen, unique, observable = _knife_draws()
    picked_unique = [i for i in chosen if i in unique]
    assert len(picked_unique) >= 12
    axes = {("x" if sc.terms[i][0] >= sc.terms[i][1] else "y") for i in picked_unique}
    assert axes == {"x", "y"} and {sc.kind[i] for i in picked_unique} == {"plain", "blend"}
    seen_axes = {("x" if sc.terms[i][0] >= sc.terms[i][1] else "y") for i in observable}
    assert len(observable) == 10 and seen_axes == {"x", "y"} and {sc.kind[i] for i in observable} == {"plain", "blend"}
    cu, _ = _camera()
    flipped_visible = 0
    with renderer.options(**DEBUG):
        with _bound(renderer, path) as pipe:
            for i in chosen:
                g = sc.g(i)
                lo = R.next_toward_zero(g)
                at_g = _debug_visible(renderer, pipe, cu, None, W, Hh, _c_float(g), ALL)
                below = _debug_visible(renderer, pipe, cu, None, W, Hh, _c_float(lo), ALL)
                keep_g, keep_lo = sc.ref_keep(g, ALL), sc.ref_keep(lo, ALL)
                assert keep_g[i] and not keep_lo[i]
                assert np.array_equal(at_g, _expected_visible(keep_g)), i
                assert np.array_equal(below, _expected_visible(keep_lo)), i
                same_g = [j for j in range(46) if sc.cull_enable[j] and R.f32_bits(sc.g(j)) == R.f32_bits(g)]
                assert same_g == [i] if i in unique else len(same_g) == 2
                want_diff = np.zeros(len(vis), dtype=bool)
                for j in same_g:
                    want_diff[off[j]:off[j + 1]] = vis[off[j]:off[j + 1]] == 1
                assert np.array_equal(at_g != below, want_diff), i
                flipped_visible += int(want_diff.any())
    assert flipped_visible == 10
    print(f"{path} knife edges: {len(chosen)} draws ({len(picked_unique)} with a g of their own), {flipped_visible} of them with visible entries "
          f"flipped by one ulp of culling_dist")


# ---- e. the two fields through the frame variants -----------------------------------------------------------------------------------
VALUES = [(0.5, 5), (0.25, 6), (1.5, 3), (0.75, ALL), (3.0, 2), (0.0, 7), (1.0, 4), (float("nan"), 1)]


def _sync_frames(renderer, pipe, cu, values, **kw):
    out = []
    for cd, mask in values:
        img = pipe.render(cu, W, Hh, culling_dist=_c_float(cd), lod_enable_mask=mask, **kw)
        t = renderer.timings()
        out.append((img, t["n_visible"], t["n_pairs"]))
    return out


def _check_sync_against_oracle(frames, values, order_mode=0):
    sc = R.scene()
    for (img, n_vis, n_pairs), (cd, mask) in zip(frames, values):
        keep = sc.ref_keep(cd, mask)
        if order_mode == 0:
            ref, st = _oracle_frame(keep)
        else:
            ref, st = orc.render(sc.cam.uniforms(), sc.su, sc.pp.tex, [d for d, k in zip(sc.all_draws, keep) if k], W, Hh, order_mode=order_mode)
        assert n_vis == st["n_visible"] and n_pairs == st["n_pairs16"], (cd, mask)
        assert H.max_abs_diff(img, ref) <= TOL, (cd, mask)
        print(f"culling_dist={cd!r} mask={mask:#x}: kept {_evidence(keep)[0]}, dropped {_evidence(keep)[1]}; with visible entries: "
              f"kept {_evidence(keep)[2]}, dropped {_evidence(keep)[3]}")


def _variant_graph(renderer, pipe, cu):
    """GSWT_OPT_GRAPH: camera and draws unchanged, (culling_dist, mask) alternating: kernel-node updates, no rebuilt graph."""
    values = [VALUES[0], VALUES[2]] * 3
    want = _sync_frames(renderer, pipe, cu, values[:2])
    _check_sync_against_oracle(want, values[:2])
    assert not np.array_equal(want[0][0], want[1][0])
    with renderer.options(TIMING=0, GRAPH=1):
        _sync_frames(renderer, pipe, cu, values[:2])                       # the slot's graph exists from here on
        s0 = renderer.graph_stats()
        got = _sync_frames(renderer, pipe, cu, values)
        s1 = renderer.graph_stats()
    assert s1[0] - s0[0] >= 6 and s1[2] - s0[2] >= 6 and s1[1] == s0[1], (s0, s1)
    for k, g in enumerate(got):
        assert np.array_equal(g[0], want[k % 2][0]) and g[1:] == want[k % 2][1:], k


def _variant_in_flight(renderer, pipe, cu):
    """Every frame slot in flight, each frame with its own values and output."""
    import torch
    slots = renderer.frame_slots()
    values = [VALUES[k % len(VALUES)] for k in range(slots)]
    want = _sync_frames(renderer, pipe, cu, values)
    _check_sync_against_oracle(want[:len(VALUES)], values[:len(VALUES)])
    su = pipe.wang.scene_uniforms()
    outs = [torch.zeros((Hh, W, 4), dtype=torch.float32, device="cuda") for _ in values]
    torch.cuda.synchronize()
    tickets = [renderer.render_async(cu, su, W, Hh, o.data_ptr(), culling_dist=_c_float(cd), lod_enable_mask=mask)
               for (cd, mask), o in zip(values, outs)]
    assert sorted(tickets) == list(range(slots))
    for t, w in zip(tickets, want):
        renderer.render_wait(t)
        tm = renderer.timings()
        assert (tm["n_visible"], tm["n_pairs"]) == w[1:]
    torch.cuda.synchronize()
    for o, w in zip(outs, want):
        assert np.array_equal(o.cpu().numpy(), w[0])
    assert len({w[0].tobytes() for w in want[:len(VALUES)]}) >= min(slots, len(VALUES)) - 1


def _variant_overflow(renderer, pipe, cu):
    """GSWT_OPT_PAIR_CAP = 256: the frame overflows and is re-run; the re-run keeps its culling_dist and mask."""
    values = VALUES[:3]
    want = _sync_frames(renderer, pipe, cu, values)
    _check_sync_against_oracle(want, values)
    for (cd, mask), w in zip(values, want):
        assert w[2] > 256
        with renderer.options(PAIR_CAP=256):
            got = _sync_frames(renderer, pipe, cu, [(cd, mask)])[0]
        assert np.array_equal(got[0], w[0]) and got[1:] == w[1:], (cd, mask)


def _variant_depth_order(renderer, pipe, cu):
    """GSWT_ORDER_DEPTH, tile-local depth sort and global depth passes."""
    values = VALUES[:4]
    want = None
    for depth_sort in (0, 1):
        with renderer.options(DEPTH_SORT=depth_sort):
            got = _sync_frames(renderer, pipe, cu, values, order_mode=L.GSWT_ORDER_DEPTH)
        if want is None:
            want = got
            _check_sync_against_oracle(want, values, order_mode=1)
        for g, w in zip(got, want):
            assert np.array_equal(g[0], w[0]) and g[1:] == w[1:], depth_sort


def _variant_shards(renderer, pipe, cu):
    """Row shards and column bands, n = 3, at culling_dist 0.5 and mask 5: the union is the unsharded frame (the band cull stacks on
    top of the draw cull)."""
    cd, mask = VALUES[0]
    want = _sync_frames(renderer, pipe, cu, [(cd, mask)])
    _check_sync_against_oracle(want, [(cd, mask)])
    full = want[0][0]
    assert full[..., 3].max() > 0.5
    n = 3
    rows_p, bw = renderer.shard_rows_padded(Hh, n), renderer.shard_cols_padded(W, n)
    img = np.zeros_like(full)
    for r in range(n):
        part = pipe.render(cu, W, Hh, shard=(r, n), culling_dist=cd, lod_enable_mask=mask)
        assert part.shape == (rows_p, W, 4)
        for y in range(Hh):
            if (y // 16) % n == r:
                img[y] = part[((y // 16) // n) * 16 + (y % 16)]
    assert np.array_equal(img, full)
    img = np.zeros_like(full)
    vis = []
    for r in range(n):
        part = pipe.render(cu, W, Hh, shard=(r, n, "cols"), culling_dist=cd, lod_enable_mask=mask)
        vis.append(renderer.timings()["n_visible"])
        x0, x1 = r * bw, min(W, (r + 1) * bw)
        img[:, x0:x1] = part[:, :x1 - x0]
    assert np.array_equal(img, full)
    assert max(vis) <= want[0][1] and sum(vis) > 0                      # a band never projects a draw the draw cull dropped


def _variant_depth_and_pick(renderer, pipe, cu):
    """depth=True and pick=True: no pick record names a dropped draw, and the depth is the background where only dropped draws covered
    the pixel."""
    sc = R.scene()
    _, full_z, full_pk = pipe.render(cu, W, Hh, culling_dist=float("inf"), lod_enable_mask=ALL, depth=True, pick=True)
    for cd, mask in (VALUES[0], VALUES[1], (1.0, 4)):
        want = _sync_frames(renderer, pipe, cu, [(cd, mask)])
        _check_sync_against_oracle(want, [(cd, mask)])
        img, z, pk = pipe.render(cu, W, Hh, culling_dist=_c_float(cd), lod_enable_mask=mask, depth=True, pick=True)
        assert np.array_equal(img, want[0][0])
        keep = sc.ref_keep(cd, mask)
        dropped = set()
        for i, (ti, (key, value)) in enumerate(zip(sc.insts, sc.sort["render_data_vec"])):
            if not keep[i]:
                dropped |= {int(ti.map_index)} if value is None else {int(m) for m in np.unique(value["gs_map_id"])}
        named = set(int(m) for m in np.unique(pk["map_index"])) - {PICK_NONE}
        assert named and not (named & dropped), sorted(named & dropped)
        empty = pk["map_index"] == PICK_NONE
        assert np.array_equal(z[empty], np.ones(int(empty.sum()), np.float32)) and not img[empty].any()
        was_dropped = np.isin(full_pk["map_index"], sorted(dropped))
        assert (was_dropped & empty).sum() > 0                            # pixels that only dropped draws covered exist
        assert (full_z[was_dropped & empty] < 1.0).all()


def _variant_chunk_cull(renderer, pipe, cu):
    """GSWT_OPT_NO_CHUNK_CULL 0 against 1: the chunk cull runs on the draws the draw cull keeps."""
    values = [VALUES[0], (0.5, ALL)]
    want = _sync_frames(renderer, pipe, cu, values)
    _check_sync_against_oracle(want, values)
    with renderer.options(NO_CHUNK_CULL=1):
        got = _sync_frames(renderer, pipe, cu, values)
    for g, w in zip(got, want):
        assert np.array_equal(g[0], w[0]) and g[1:] == w[1:]


VARIANTS = {"graph": _variant_graph, "in_flight": _variant_in_flight, "overflow_rerun": _variant_overflow, "depth_order": _variant_depth_order,
            "shards": _variant_shards, "depth_and_pick": _variant_depth_and_pick, "chunk_cull": _variant_chunk_cull}


@pytest.mark.parametrize("variant", list(VARIANTS) + ["ortho"])
def test_frame_variants_carry_both_fields(renderer, variant):
    if variant == "ortho":
        return _variant_ortho(renderer)
    cu, _ = _camera()
    with _bound(renderer, "set_draws") as pipe:
        VARIANTS[variant](renderer, pipe, cu)


def _variant_ortho(renderer):
    """GSWT_OPT_PROJECTION = 1 with hand-made corners under an ortho.top_down camera: the same formula on that affine matrix (w = 1).
    The z branch is in reach here: NDC z < 0 is the upper half of the camera's height range."""
    pp = _hand_pp()
    W2, H2 = 160, 96
    cx, cy, half, z_top, z_bottom = 0.0, 20.0, 12.0, 3.0, -3.0
    cam = ortho.top_down((cx, cy), half, z_top, z_bottom, W2, H2)
    vp = cam.view_proj()
    hw = half * W2 / H2
    P = lambda nx, ny, nz: (cx + nx * hw, cy + ny * half, z_top - (nz + 1.0) * 0.5 * (z_top - z_bottom))
    nan = float("nan")
    in_view = [P(0.3, 0.3, 0.5), P(-0.3, 0.3, 0.5), P(-0.3, -0.3, 0.4), P(0.3, -0.3, 0.6)]
    sets = {
        "in_view": in_view,
        "x_out": [P(1.5, 0.0, 0.5), P(2.5, 0.1, 0.5), P(2.0, -0.1, 0.4), P(1.7, 0.0, 0.6)],
        "y_out": [P(0.0, 1.5, 0.5), P(0.1, 2.5, 0.5), P(-0.1, 2.0, 0.4), P(0.0, 1.7, 0.6)],
        "x_half": [P(0.5, 0.0, 0.5), P(0.8, 0.1, 0.5), P(0.9, -0.1, 0.4), P(0.7, 0.0, 0.6)],
        "z_upper_only": [P(0.0, 0.0, -0.5), P(0.2, 0.1, -0.4), P(-0.1, 0.2, -0.6), P(0.1, -0.1, -0.3)],
        "z_mixed": [P(0.0, 0.0, -0.5), P(0.0, 0.0, 0.4), P(0.0, 0.0, -0.6), P(0.0, 0.0, -0.3)],
        "above_top": [P(0.0, 0.0, -1.5), P(0.1, 0.0, -2.0), P(0.0, 0.1, -1.2), P(-0.1, -0.1, -1.7)],
        "below_bottom": [P(0.0, 0.0, 1.5), P(0.1, 0.0, 2.0), P(0.0, 0.1, 1.2), P(-0.1, -0.1, 1.7)],
        "nan_one": [(nan, in_view[0][1], in_view[0][2])] + in_view[1:],
        "nan_all": [(nan, nan, nan)] * 4,
    }
    names = list(sets)
    corners = [np.asarray(sets[nm], dtype=np.float32) for nm in names]
    case = _hand_case(pp, len(names), {i: dict(corners=c) for i, c in enumerate(corners)})
    terms = [R.cull_terms(vp, c) for c in corners]
    t_of = dict(zip(names, terms))
    assert t_of["z_upper_only"][0] == 0 and t_of["z_upper_only"][1] == 0 and t_of["z_upper_only"][2] < 0 and t_of["z_mixed"][2] > 0
    renderer.configure(None)
    su = orc.scene_uniforms(num_lod=pp.n_lod, map_half_wh=(2, 2))
    frames = [(0.0, ALL), (0.25, ALL), (0.5, ALL), (1.0, ALL), (1.0, 0), (float("nan"), ALL)]
    lods = [0] * len(names)
    with renderer.options(PROJECTION=L.GSWT_PROJECTION_ORTHO):     # (the frames set it themselves; the block puts it back)
        seen = _check_hand_frames(renderer, case, cam.uniforms(), su, vp, frames, W2, H2,
                                  lambda i, cd, mask: R.keeps(terms[i], cd) and R.lod_kept(mask, lods[i]), projection=L.GSWT_PROJECTION_ORTHO)
    nvis = seen[0][1]
    assert all(n > 0 for n in nvis), dict(zip(names, nvis))
    by_cd = {repr(cd) + ("" if mask else "/0"): dict(zip(names, keep)) for (cd, mask), (keep, _) in zip(frames, seen)}
    assert not by_cd["0.0"]["z_upper_only"] and by_cd["0.0"]["z_mixed"] and by_cd["0.5"]["z_upper_only"]
    assert by_cd["1.0"]["in_view"] and not by_cd["1.0"]["x_out"] and not by_cd["1.0"]["y_out"] and not by_cd["1.0"]["above_top"]
    assert by_cd["1.0"]["below_bottom"] and not any(by_cd["1.0/0"].values()) and all(by_cd["nan"].values())
    for (cd, mask), (keep, _) in zip(frames, seen):
        print(f"ortho culling_dist={cd!r} mask={mask:#x}: kept {sum(keep)}, dropped {len(keep) - sum(keep)} of {len(keep)} draws, all with visible entries")
