"""The depth image's CPU reference (tests/depth_ref.py) and the depth-output ABI, without a GPU.

depth_ref composites colour and depth together; its colour must reproduce the oracle's image (orc.render) within the parity
tolerance on the golden configurations (built as tests/golden/make_golden.py builds them) and a grid of plain draws, in both order
modes, with and without a proxy depth buffer.  Where no splat covers a pixel the depth is the background depth exactly."""
import os
import re

import numpy as np
import pytest

from gswt_renderer_amd import _lib as L
from oracle import gswt_oracle as orc
from tests import depth_ref as DR
from tests import helpers as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-4          # the parity tolerance of the image tests (BASELINE.json north_star)


def _grid_case():
    pp = H.tileset(lod0_count=400)
    W, Hh = 160, 120
    cam = orc.default_camera(W, Hh)
    su = orc.scene_uniforms(num_lod=pp.n_lod, map_half_wh=(1, 2))
    case = H.grid_case(pp)
    sp = orc.project_draws(cam.uniforms(), su, pp.tex, case.orc_draws)
    return dict(W=W, H=Hh, cam=cam, su=su, pp=pp, draws=case.orc_draws, hm=None, sp=sp)


_CASES = {}


def _case(name):
    if name not in _CASES:
        _CASES[name] = _grid_case() if name == "grid" else DR.golden_case(name)
    return _CASES[name]


@pytest.mark.parametrize("bg", [False, True], ids=["clear", "bg_depth"])
@pytest.mark.parametrize("order_mode", [0, 1], ids=["reference", "depth"])
@pytest.mark.parametrize("name", ["case_plane", "case_hmap", "case_sphere", "grid"])
def test_depth_ref_colour_reproduces_the_oracle(name, order_mode, bg):
    g = _case(name)
    W, Hh = g["W"], g["H"]
    bgc, bgd = DR.bg_images(W, Hh) if bg else (None, None)
    ref, st = orc.render(g["cam"].uniforms(), g["su"], g["pp"].tex, g["draws"], W, Hh, height_map=g["hm"], bg_rgba=bgc, bg_depth=bgd,
                         order_mode=order_mode)
    img, z, n_cover = DR.composite(g["sp"], W, Hh, splat_scale=g["su"].splat_scale, order_mode=order_mode, bg_rgba=bgc, bg_depth=bgd,
                                   with_cover=True)
    assert st["n_visible"] > 0 and n_cover.any()
    assert H.max_abs_diff(img, ref) <= TOL
    zbg = np.ones((Hh, W), np.float32) if bgd is None else bgd
    free = n_cover == 0
    assert free.any()
    assert np.array_equal(z[free].view(np.uint32), zbg[free].view(np.uint32))
    # covered pixels: the blend of depths in [0, 1] stays between the nearest splat and the background
    assert np.all(z >= 0.0) and np.all(z <= 1.0)


def test_depth_ref_is_expected_depth_over_the_background():
    """Z = T z_bg + sum w_i z_i: a single opaque-enough splat at depth d gives Z = (1 - a) z_bg + a d at its centre."""
    sp = np.zeros(1, dtype=orc.SPLAT_DTYPE)
    sp["visible"] = 1
    sp["ndc"] = (0.0, 0.0)
    sp["depth"] = 0.5
    sp["major"] = (4.0, 0.0)          # (pixels: a quad of half axes 2 px, so r^2 = 1/8 at the four centre pixels)
    sp["minor"] = (0.0, 4.0)
    sp["rgba"] = (1.0, 0.5, 0.25, 0.75)
    img, z = DR.composite(sp, 32, 32, splat_scale=1.0)
    a = img[16, 16, 3]
    assert 0.6 < a <= 0.75
    assert abs(float(z[16, 16]) - ((1.0 - a) * 1.0 + a * 0.5)) <= 1e-6
    assert z[0, 0] == 1.0


def _decl_args(header: str, name: str):
    src = open(os.path.join(ROOT, "include", header)).read()
    src = re.sub(r"/\*.*?\*/", " ", src, flags=re.S)
    m = re.search(r"GSWT_API\s+int\s+" + name + r"\s*\(([^)]*)\)", src)
    assert m, name
    return [a.strip() for a in m.group(1).split(",")]


@pytest.mark.parametrize("name,base", [("gswt_render_depth", "gswt_render"), ("gswt_render_async_depth", "gswt_render_async")])
def test_depth_entry_points_in_header_ctypes_and_rust(name, base):
    args, base_args = _decl_args("gswt_hip.h", name), _decl_args("gswt_hip.h", base)
    # the new entry point is its base with one f32 output pointer after the colour output
    k = next(i for i, a in enumerate(base_args) if a.startswith("float *out_rgba"))
    assert args[:k + 1] == base_args[:k + 1] and args[k + 2:] == base_args[k + 1:]
    assert re.fullmatch(r"float \*out_depth(_dev)?", args[k + 1])
    res, ct = L.SYMBOLS[name]
    assert res is L.SYMBOLS[base][0] and len(ct) == len(args)
    rs = open(os.path.join(ROOT, "rust", "src", "gswt_hip_sys.rs")).read()
    m = re.search(r"pub fn " + name + r"\(([^)]*)\)", rs, flags=re.S)
    assert m and len([a for a in m.group(1).split(",") if a.strip()]) == len(args)
    assert "out_depth" in m.group(1)
