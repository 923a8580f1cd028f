"""The pick image's CPU reference (tests/pick_ref.py) and the pick ABI, without a GPU.

pick_ref keeps every covering instance of every pixel with its weight; its colour must reproduce the oracle's image (orc.render) within
the parity tolerance on the golden configurations and the grid of plain draws, in both order modes, with and without a proxy depth
buffer.  Closed-form scenes pin the definition (largest weight, front-most of equal weights, no hit behind the depth buffer), the
segmented fold is run on the reference's own events, and the share of indecisive pixels -- which the GPU test's exact-identity check
leaves out -- is bounded for every case the GPU test uses."""
import ctypes as C
import os

import numpy as np
import pytest

from gswt_renderer_amd import _lib as L
from oracle import gswt_oracle as orc
from tests import depth_ref as DR
from tests import helpers as H
from tests import pick_ref as PR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = PR.TOL
GOLDEN = ["case_plane", "case_hmap", "case_sphere", "case_plane_mode1"]
INDECISIVE_CAP = 0.05


def grid_case(W=320, Hh=240, splat_scale=1.0):
    """The reduced c3-style scene of the depth-output tests: a 3 x 5 grid of plain draws at 320 x 240.  "grid_dense" is the same grid at
    160 x 120 with splat_scale 24: pixels under hundreds of splats and screen tiles of more than 256 pairs, so that a 256-pair
    GSWT_OPT_SEGMENT cuts their lists and the segment fold runs against the reference."""
    pp = H.tileset()
    cam = orc.default_camera(W, Hh)
    su = orc.scene_uniforms(num_lod=pp.n_lod, map_half_wh=(1, 2), splat_scale=splat_scale)
    case = H.grid_case(pp)
    sp = orc.project_draws(cam.uniforms(), su, pp.tex, case.orc_draws)
    return dict(W=W, H=Hh, cam=cam, su=su, pp=pp, draws=case.orc_draws, hm=None, sp=sp, case=case)


_CASES, _EVENTS = {}, {}


def case(name):
    if name not in _CASES:
        _CASES[name] = grid_case() if name == "grid" else grid_case(160, 120, 24.0) if name == "grid_dense" else DR.golden_case(name)
    return _CASES[name]


def bg_of(name, bg):
    g = case(name)
    return DR.bg_images(g["W"], g["H"], seed=11 if name.startswith("grid") else 5) if bg else (None, None)


def events(name, order_mode, bg):
    k = (name, order_mode, bg)
    if k not in _EVENTS:
        g = case(name)
        bgc, bgd = bg_of(name, bg)
        _EVENTS[k] = PR.composite(g["sp"], g["W"], g["H"], splat_scale=g["su"].splat_scale, order_mode=order_mode, bg_rgba=bgc, bg_depth=bgd)
    return _EVENTS[k]


# the cases of tests/test_pick_gpu.py's comparison against the reference
GPU_CASES = [(n, o, b) for n in GOLDEN + ["grid", "grid_dense"] for o in (0, 1) for b in (False, True)]


@pytest.mark.parametrize("bg", [False, True], ids=["clear", "bg_depth"])
@pytest.mark.parametrize("order_mode", [0, 1], ids=["reference", "depth"])
@pytest.mark.parametrize("name", GOLDEN)
def test_pick_ref_colour_reproduces_the_oracle(name, order_mode, bg):
    g = case(name)
    W, Hh = g["W"], g["H"]
    bgc, bgd = bg_of(name, bg)
    ref, st = orc.render(g["cam"].uniforms(), g["su"], g["pp"].tex, g["draws"], W, Hh, height_map=g["hm"], bg_rgba=bgc, bg_depth=bgd,
                         order_mode=order_mode)
    ev = events(name, order_mode, bg)
    assert st["n_visible"] > 0 and ev["pix"].size > 0
    assert H.max_abs_diff(ev["img"], ref) <= TOL
    # the weights are the colour's: alpha = sum of the weights = 1 - T_final (no background alpha under it)
    if not bg:
        assert np.abs(np.bincount(ev["pix"], ev["w"], W * Hh).reshape(Hh, W) - ref[..., 3]).max() <= TOL


def _one(ndc, depth, alpha, half_px=4.0, W=32, Hh=32):
    sp = np.zeros(1, dtype=orc.SPLAT_DTYPE)
    sp["visible"] = 1
    sp["ndc"] = ndc
    sp["depth"] = depth
    sp["major"] = (2.0 * half_px, 0.0)            # (pixels: a quad of half axes half_px)
    sp["minor"] = (0.0, 2.0 * half_px)
    sp["rgba"] = (1.0, 0.5, 0.25, alpha)
    return sp


CENTRE = (1.0 / 32.0, -1.0 / 32.0)       # the centre of pixel (16, 16) of a 32 x 32 frame: r^2 = 0 there, e = alpha exactly


def _pick_at(sps, x=16, y=16, **kw):
    sp = np.concatenate(sps)
    ev = PR.composite(sp, 32, 32, **kw)
    win = PR.winners(ev)
    b = win["best"][y, x]
    return (int(ev["inst"][b]) if b >= 0 else -1), float(win["w1"][y, x]), ev, win


def test_single_splat():
    k, w, ev, win = _pick_at([_one(CENTRE, 0.5, 0.75)])
    assert k == 0 and w == 0.75
    assert win["best"][0, 0] == -1 and win["w1"][0, 0] == 0.0 and (win["n"] > 0).sum() > 4
    assert np.all(win["w1"][win["n"] > 0] <= 0.75)


def test_back_splat_wins_when_the_front_one_is_faint():
    # draw order is back to front: instance 0 is behind instance 1
    k, w, _, _ = _pick_at([_one(CENTRE, 0.6, 0.9), _one(CENTRE, 0.4, 0.125)])
    assert k == 0 and w == (1.0 - 0.125) * np.float64(np.float32(0.9))


def test_front_splat_wins():
    k, w, _, _ = _pick_at([_one(CENTRE, 0.6, 0.9), _one(CENTRE, 0.4, 0.75)])
    assert k == 1 and w == 0.75
    # depth order: the blend order follows the depths, not the draw order
    k, w, _, _ = _pick_at([_one(CENTRE, 0.4, 0.75), _one(CENTRE, 0.6, 0.9)], order_mode=1)
    assert k == 0 and w == 0.75


def test_exact_tie_goes_to_the_front_most():
    # front e = 0.5, back e = 1: w_back = (1 - 0.5) * 1 = 0.5 = w_front, in binary32 and binary64 alike
    k, w, ev, win = _pick_at([_one(CENTRE, 0.6, 1.0), _one(CENTRE, 0.4, 0.5)])
    assert k == 1 and w == 0.5 and win["w2"][16, 16] == 0.5
    # the segmented fold keeps it for every cut
    for seg_len in (1, 2):
        assert ev["inst"][PR.fold_segments(ev, seg_len)[16, 16]] == 1


def test_pixel_behind_bg_depth_has_no_hit():
    bgd = np.full((32, 32), 0.3, np.float32)
    bgd[:, 20:] = 0.9
    sp = _one(CENTRE, 0.5, 0.75, half_px=8.0)
    ev = PR.composite(sp, 32, 32, bg_depth=bgd)
    win = PR.winners(ev)
    assert win["best"][16, 16] == -1 and win["best"][16, 21] >= 0
    pick = reference_pick(ev, sp, np.zeros(1, np.uint32), np.array([7], np.uint32))
    assert pick[16, 16]["map_index"] == PR.NONE and pick[16, 16]["entry"] == PR.NONE and pick[16, 16]["weight"] == 0.0
    assert pick[16, 16]["depth"] == np.float32(0.3) and pick[0, 31]["depth"] == np.float32(0.9)
    assert pick[16, 21]["entry"] == 7 and pick[16, 21]["depth"] == np.float32(0.5)


def reference_pick(ev, sp, map_index, entry):
    """The reference's own pick image (its arg-max), in the public record layout."""
    from gswt_renderer_amd.renderer import PICK_DTYPE
    win = PR.winners(ev)
    out = np.zeros((ev["H"], ev["W"]), PICK_DTYPE)
    out["map_index"] = out["entry"] = PR.NONE
    out["depth"] = ev["zbg"]
    hit = win["best"] >= 0
    k = ev["inst"][win["best"][hit]]
    out["map_index"][hit], out["entry"][hit] = map_index[k], entry[k]
    out["depth"][hit] = sp["depth"][k]
    out["weight"][hit] = win["w1"][hit].astype(np.float32)
    return out


@pytest.mark.parametrize("name,order_mode,bg", GPU_CASES)
def test_indecisive_pixels_are_few_and_the_checker_checks(name, order_mode, bg):
    """Non-vacuity of the GPU test's exact-identity check: at most 5 % of a case's covered pixels are indecisive (leader - runner-up
    <= 2 tol).  And the checker itself: it passes the reference's own arg-max image and refuses a wrong identity, weight or depth."""
    g, ev = case(name), events(name, order_mode, bg)
    win = PR.winners(ev)
    share, ind = PR.indecisive_share(win)
    cov = win["n"] > 0
    print(f"{name} order={order_mode} bg={bg}: covered={int(cov.sum())} of {cov.size}, indecisive={int(ind.sum())} ({share:.4f}), "
          f"longest pixel list={int(win['n'].max())}")
    assert cov.sum() >= 30 and (~cov).any() and (win["n"] > 1).any()        # (the golden frames are small and sparse)
    assert share <= INDECISIVE_CAP
    mi, en = PR.identities(g["draws"])
    assert mi.shape == en.shape == g["sp"].shape
    pick = reference_pick(ev, g["sp"], mi, en)
    assert PR.check_pick(pick, ev, g["sp"], mi, en, label=name) <= 1e-7
    y, x = [int(v[0]) for v in np.nonzero(cov & ~ind & (win["n"] > 1))]
    for field, value in (("weight", pick[y, x]["weight"] + np.float32(3e-4)), ("depth", np.float32(0.123)), ("entry", 0x0FFFFFF0)):
        bad = pick.copy()
        bad[y, x][field] = value
        with pytest.raises(AssertionError):
            PR.check_pick(bad, ev, g["sp"], mi, en, label="tampered " + field)
    # the runner-up instead of the leader on a decisive pixel
    o = np.arange(ev["start"][y * ev["W"] + x], ev["start"][y * ev["W"] + x + 1])
    second = o[np.argsort(-ev["w"][o], kind="stable")[1]]
    k2 = ev["inst"][second]
    bad = pick.copy()
    bad[y, x] = (mi[k2], en[k2], g["sp"]["depth"][k2], np.float32(ev["w"][second]))
    if (mi[k2], en[k2]) != (pick[y, x]["map_index"], pick[y, x]["entry"]):
        with pytest.raises(AssertionError):
            PR.check_pick(bad, ev, g["sp"], mi, en, label="tampered runner-up")


@pytest.mark.parametrize("seg_len", [1, 2, 3])
@pytest.mark.parametrize("name", GOLDEN + ["grid", "grid_dense"])
def test_segment_fold_finds_the_maximum(name, seg_len):
    """The fold of T_prefix * w'_max over segments of the pixels' lists, in binary32: the folded winner's weight is within tol of the
    unsplit maximum at every pixel (and it is the same event wherever the pixel is decisive)."""
    for order_mode in (0, 1):
        ev = events(name, order_mode, False)
        win = PR.winners(ev)
        fb = PR.fold_segments(ev, seg_len)
        cov = win["n"] > 0
        assert np.array_equal(fb >= 0, cov)
        assert (win["n"] > 1).any()                 # seg_len 1 cuts every list of two or more (the golden frames' lists are short)
        wf = ev["w"][fb[cov]]
        assert (win["w1"][cov] - wf).max() <= TOL
        _, ind = PR.indecisive_share(win)
        dec = cov & ~ind
        assert np.array_equal(fb[dec], win["best"][dec])


def test_pick_abi():
    """The library exports the two entry points and gswt_pick is 16 bytes: map_index 0, entry 4, depth 8, weight 12."""
    import importlib.util
    lib = L.load()
    for name in ("gswt_render_pick", "gswt_render_async_pick"):
        assert getattr(lib, name) is not None and name in L.SYMBOLS
    assert len(L.SYMBOLS["gswt_render_pick"][1]) == len(L.SYMBOLS["gswt_render_depth"][1]) + 1
    assert len(L.SYMBOLS["gswt_render_async_pick"][1]) == len(L.SYMBOLS["gswt_render_async_depth"][1]) + 1
    spec = importlib.util.spec_from_file_location("_gen_rust", os.path.join(ROOT, "tools", "gen_rust_bindings.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    hdr = gen.Header(os.path.join(ROOT, "include", "gswt_hip.h"))
    size, _, offs = gen.struct_layout(hdr.structs["gswt_pick"], {}, hdr.known)
    want = [("map_index", 0), ("entry", 4), ("depth", 8), ("weight", 12)]
    assert size == 16 and offs == want
    assert C.sizeof(L.Pick) == 16 and [(n, getattr(L.Pick, n).offset) for n, _ in L.Pick._fields_] == want
    from gswt_renderer_amd.renderer import PICK_DTYPE
    assert PICK_DTYPE.itemsize == 16 and [(n, PICK_DTYPE.fields[n][1]) for n in PICK_DTYPE.names] == want
    assert [PICK_DTYPE.fields[n][0] for n in PICK_DTYPE.names] == [np.dtype("<u4"), np.dtype("<u4"), np.dtype("<f4"), np.dtype("<f4")]
