"""The frame modes of the strict vertex stage stacked on one another (k_project<DEBUG, FULL, STRICT, ORTHO, AA, ATM, STY, SHD>): the expected
projected records of a golden case under a camera at one point of the lattice (orthographic, pixel filter, atmosphere as fade / fog /
both, tile styles, sun shadow).  numpy only, no tests here: tests/test_mode_stack_cpu.py pins this module and its inputs without a GPU,
tests/test_mode_stack_gpu.py compares the device with it.

No projection is restated here.  The stack composes the references the tree already has, each pinned per mode:

  base records   oracle.project_draws under oracle.frame_mode(ortho, aa_s, fade): `visible` (the pair rectangles', the product's),
                 ndc, depth, both axes, and alpha with the LOD-transition share, the filter's comp and the fade's fs in it, in the
                 kernel's order ((ca . lod) . comp) . fs.  tests/test_pair_list_modes_cpu.py pins these to the numpy references.
  styles         tests/tile_style_ref.py over tests/pick_ref.identities: a hidden cell is not visible; alpha = dimmed_alpha(base
                 alpha), the dim behind the three products above; the tint as unquantised binary32 floats (tinted_rgb).
  shadow         sh from tests/shadow_ref.py: lookup_f32 of centres_f32 on the plain surface (exact), lookup_f64 at the float64
                 unprojection of the splat's own unmoded record on the HeightMap and Sphere surfaces.
  fog            tests/atmosphere_ref.py's F(dist): dist_f32 on the plain surface (exact), the unprojected distance on the others.

Colour is tint -> shadow -> fog on unquantised floats with ONE quantisation behind them, and is compared in one of three ways (`how`):

  "exact"   no fog, and either the plain surface or no shadow: every operation is a correctly rounded binary32 one, restated operator
            by operator: c_t = c (1 - k) + t k;  c_s = c_t (1 - sh) + shade sh where sh != 0;  quantised once (shadow_ref.quantise_f32)
            if and only if the splat is tinted or sh != 0, otherwise the record's own floats untouched.  Bit for bit, no mask.
  "rint"    the plain surface with the fog on (__expf is not correctly rounded): shadow_ref.chain_codes_f64; a byte equals the float64
            rint wherever the code is farther than AR.FOG_MARGIN from a half-integer, is within one code everywhere, and at most
            AR.MAX_MASKED of the channels lie inside the margin.
  "bound"   HeightMap / Sphere with the shadow or the fog on.  The float64 code of chain_codes_f64 at the unprojected position, and a
            byte must lie within 0.5 + tol + SR.MARGIN of it, tol the SUM of the bounds the single-mode tests derive:
              * the unprojected position is off by at most delta world units: delta = SR.persp_delta(z, near) =
                AR.DEPTH_ROUNDINGS z^2 / near 2^-24 under the perspective camera (atmosphere_ref's derivation), and
                delta = AR.DEPTH_ROUNDINGS 2^-24 (far - near + |pos|) under an orthographic one (depth is linear there: its binary32
                rounding times the depth range along the ray, plus the coordinates' own, as tests/test_shadow_gpu.py's
                orthographic proxy case has it);
              * shadow: |dc / d sh| <= 1 and |d sh| <= SR.surface_tols(pos, delta, p)[0], in codes 255 times that; the fog that follows
                scales it by (1 - F) <= 1;
              * fog: c' = c (1 - F) + fog F, |dc' / dF| <= 1, F = fog_max (1 - exp(-density (dist - start))) has
                |dF / d dist| <= fog_max density, and |d dist| <= delta: in codes 255 fog_max density delta.
            A splat whose ld, ld - 1 or ld - bias lies within SR.surface_tols(...)[1] of zero (the `outside` test or a depth compare may
            fall on either side), or, with the fade on, whose t lies within its tolerance of 0, is left out (`masked`): at most
            AR.MAX_MASKED of the visible splats.

Visibility, geometry and alpha are bit for bit on all three surfaces, whatever `how` is.

The inputs (`inputs`) are chosen so that the modes meet: tests/test_mode_stack_cpu.py holds the conditions."""
from __future__ import annotations

import dataclasses
import functools

import numpy as np

from gswt_renderer_amd import atmosphere as A
from gswt_renderer_amd import shadows
from oracle import gswt_oracle as orc
from tests import antialias_ref as AAR
from tests import atmosphere_ref as AR
from tests import frame_modes as FM
from tests import ortho_ref as OR
from tests import pick_ref as PR
from tests import shadow_ref as SR
from tests import tile_style_ref as TR

F32 = np.float32
W, Hh = OR.W, OR.H
GEOMETRY = ("ndc", "depth", "major", "minor")
AA_VALUE = 307                                  # GSWT_OPT_ANTIALIAS: 307 / 1024 px^2
FOG = (0.15, 2.0, 0.9, (0.62, 0.71, 0.80))      # the atmosphere tests' fog
ATMS = (None, "fade", "fog", "both")
CAMERAS = {"case_plane": ("persp", "oblique"), "case_sphere": ("persp", "top"), "case_hmap": ("persp",)}
# the hostile cases of tests/hostile_cases.py, kept apart: the tests that walk CAMERAS hold conditions on the golden cases' own populations
HOSTILE_CAMERAS = {"case_plane_hostile": ("persp", "oblique"), "case_hmap_hostile": ("persp", "top")}
PLAIN_SURFACE = ("case_plane", "case_plane_hostile")


@dataclasses.dataclass(frozen=True)
class Point:
    """One lattice point: a golden case under a camera with the modes that are on."""
    case: str
    cam: str
    aa: bool = False
    atm: str | None = None              # None, "fade", "fog" or "both"
    sty: bool = False
    shd: bool = False

    @property
    def fade(self):
        return self.atm in ("fade", "both")

    @property
    def fog(self):
        return self.atm in ("fog", "both")

    @property
    def id(self):
        on = [w for w, b in (("aa", self.aa), (self.atm, self.atm), ("sty", self.sty), ("shd", self.shd)) if b]
        return f"{self.case[5:]}-{self.cam}-" + ("+".join(on) or "plain")

    def instantiation(self, debug):
        """The k_project instantiation the point's frame launches."""
        b = lambda x: "1" if x else "0"
        return (f"k_project<DEBUG={b(debug)}, FULL={b(self.case == 'case_sphere')}, STRICT=1, ORTHO={b(self.cam != 'persp')}, AA={b(self.aa)}, "
                f"ATM={b(self.atm)}, STY={b(self.sty)}, SHD={b(self.shd)}>")


def corner(case, cam, atm="both"):
    return Point(case, cam, True, atm, True, True)


def square(case, cam):
    """The 2^4 combinations of (AA, ATM, STY, SHD) with ATM as fade + fog together."""
    return [Point(case, cam, bool(k & 8), "both" if k & 4 else None, bool(k & 2), bool(k & 1)) for k in range(16)]


def pairs_and_corner(case, cam):
    """All four on, and the six pairs."""
    out = [corner(case, cam)]
    for i in range(4):
        for j in range(i + 1, 4):
            on = [k in (i, j) for k in range(4)]
            out.append(Point(case, cam, on[0], "both" if on[1] else None, on[2], on[3]))
    return out


LATTICE = (square("case_plane", "persp") + square("case_plane", "oblique") + square("case_sphere", "persp") + square("case_sphere", "top")
           + pairs_and_corner("case_hmap", "persp") + [corner("case_plane", "persp", "fade"), corner("case_plane", "persp", "fog")])


# ---- the inputs ----------------------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass(frozen=True)
class Inputs:
    fade: tuple                 # (fade_start, fade_end)
    cells: dict                 # {map cell: tile_style_ref entry}
    n_styles: int
    shadow: object              # shadows.ShadowMap

    @property
    def entries(self):
        return TR.entries(self.cells, self.n_styles)


# The plane case: the shadow tests' light and map; a table whose tinted cells are the ones the fade keeps and the map shadows under both
# cameras (13, 8, 17), with dim on a tinted cell (8) and on an untinted one (18), one hidden cell the fade keeps (12) and one it
# discards anyway (24).  No tint is at full strength: a tint of strength 255 lands on a byte exactly, and a second quantisation behind it
# (tests/test_mode_stack_cpu.py's order check) would not show on that cell's 60 splats of the oblique frame.
PLANE_CELLS = {13: TR.entry((0, 255, 64), 160), 8: TR.entry((255, 64, 0), 160, 96), 17: TR.entry((10, 20, 250), 200), 18: TR.entry(dim=128),
               12: TR.HIDE, 24: TR.HIDE}
# The surfaces start from tests/test_tile_style_gpu.py's cells.  The HeightMap case draws six cells with 122 visible splats: the tints go
# to the two cells the light shadows and the fade keeps (13, 8), the dims to the two with the most splats on the ramp (13, 18), and the
# hidden cells are one the fade keeps (14) and one it discards anyway (19).  The Sphere case keeps that file's table and adds what it
# lacks where the modes meet: a tinted and a tinted-and-dimmed cell that are shadowed and on the ramp (28, 19), a dimmed cell on the
# ramp (18), a hidden cell the fade discards anyway (9); cells 32 .. 39 lie past the table.
SURFACE_CELLS = {
    "case_hmap": ({13: TR.entry((20, 200, 90), 180, 100), 8: TR.entry((250, 30, 30), 200), 18: TR.entry(dim=128), 14: TR.HIDE, 19: TR.HIDE}, 20),
    "case_sphere": ({27: TR.HIDE, 31: TR.entry((20, 200, 90), 180), 25: TR.entry(dim=77), 26: TR.entry((250, 30, 30), 255, 40), 30: TR.HIDE,
                     3: TR.entry((0, 0, 255), 90), 28: TR.entry((200, 30, 160), 200), 19: TR.entry((240, 220, 20), 150, 60), 18: TR.entry(dim=128),
                     9: TR.HIDE}, 32)}
SURFACE_SHADE = dict(bias=0.0, strength=0.8, shade_color=(0.05, 0.1, 0.3))


@functools.lru_cache(maxsize=None)
def inputs(case) -> Inputs:
    if case == "case_plane_hostile":            # its own ramp, table and light: tests/hostile_cases.py says why
        from tests import hostile_cases as HC
        light = HC.plane_light()
        m = shadows.from_ortho_camera(light, HC.plane_map(light), bias=0.002, strength=0.75, shade_color=(0.1, 0.05, 0.2))
        return Inputs(HC.PLANE_FADE, HC.PLANE_CELLS, HC.PLANE_N_STYLES, m)
    if case in PLAIN_SURFACE:
        light = SR.plane_light()
        m = shadows.from_ortho_camera(light, SR.plane_map(light), bias=0.002, strength=0.75, shade_color=(0.1, 0.05, 0.2))
        return Inputs((4.0, 8.0), PLANE_CELLS, 25, m)
    # a ramp over the distances of the perspective frame's visible splats, and a top-down light whose left half shadows everything
    _, cu, _, _, unf = FM.view(case, "persp")
    vis = unf["visible"] == 1
    dist, _ = AR.dist_f64(_block(cu), unf["ndc"][vis], unf["depth"][vis])
    light = OR.ortho_camera_of(OR.surface_camera_args(case, "top"), 32, 24)
    m = shadows.from_ortho_camera(light, SR.two_region_map(32, 24), **SURFACE_SHADE)
    cells, n = SURFACE_CELLS["case_hmap" if case == "case_hmap_hostile" else case]
    return Inputs(AR.ramp_from_percentiles(dist), cells, n, m)


def _block(cu):
    return orc.Camera176.from_buffer_copy(bytes(cu))


def atmosphere_of(pt):
    if pt.atm is None:
        return A.OFF
    return A.Atmosphere(fade=inputs(pt.case).fade if pt.fade else None, fog=FOG if pt.fog else None)


def render_kw(pt):
    """The mode keywords of GSWTRenderer.render for the point (the projection is the view's)."""
    inp = inputs(pt.case)
    return dict(antialias=AA_VALUE / 1024.0 if pt.aa else 0.0, atmosphere=atmosphere_of(pt),
                tile_styles=TR.pack(inp.entries) if pt.sty else b"", shadow=inp.shadow if pt.shd else shadows.OFF)


# ---- the base records and what the world gives ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def base_records(case, cam, aa, fade, draw_mode=0, point_cloud_radius=0.0):
    """The oracle's records of the case under the camera with the filter and the fade on or off, `visible` the pair rectangles'.
    draw_mode, point_cloud_radius: on a copy of the view's scene block carrying them (tests/debug_modes_ref.py)."""
    g, cu, su, proj, _ = FM.view(case, cam)
    if draw_mode or point_cloud_radius:
        su = orc.Scene160.from_buffer_copy(bytes(su))
        su.draw_mode, su.point_cloud_radius = int(draw_mode), float(point_cloud_radius)
    s = float(AAR.aa_s(AA_VALUE, su.splat_scale)) if aa else 0.0
    fd = None
    if fade:
        p = AR.params(A.Atmosphere(fade=inputs(case).fade))
        fd = (float(p["fade_end"]), float(p["fade_inv"]))
    block = _block(cu)
    with orc.frame_mode(ortho=int(proj == FM.ORTHO), aa_s=s, fade=fd):
        sp = orc.project_draws(block, su, g["pp"].tex, g["draws"], height_map=g["hm"]).copy()
        sp["visible"] = orc.pair_rects(block, su, g["pp"].tex, g["draws"], W, Hh, height_map=g["hm"])["visible"]
    return sp


@functools.lru_cache(maxsize=None)
def world(case, cam):
    """Per instance, what the shadow and the atmosphere read: dist from cam_pos, sh, and on the surfaces the tolerances of the module
    docstring (zero on the plain surface, where dist and sh are the device's own binary32 numbers).  Rows of instances that are not
    visible without any mode hold dist = inf, sh = 0."""
    g, cu, su, proj, _ = FM.view(case, cam)
    block = _block(cu)
    p = SR.params(inputs(case).shadow)
    unf = base_records(case, cam, False, False)
    n = unf.shape[0]
    vis = unf["visible"] == 1
    zero = np.zeros(n)
    if case in PLAIN_SURFACE:
        dist = AR.dist_f32(block.cam_pos, su, g["pp"].tex, g["draws"]).astype(np.float64)
        sh = SR.lookup_f32(SR.centres_f32(su, g["pp"].tex, g["draws"]), p)[0]
        return dict(exact=True, dist=dist, sh=sh, delta=zero, tol_sh=zero, near_ld=np.zeros(n, bool), z=zero, near=0.0, p=p)
    pos, z = AR.unproject_f64(block, unf["ndc"][vis], unf["depth"][vis])
    cp = np.array([float(block.cam_pos[k]) for k in range(3)])
    if proj == FM.ORTHO:
        span = 2.0 / abs(float(block.projection[10]))
        delta, near = AR.DEPTH_ROUNDINGS * SR.U * (span + np.abs(pos).max(1)), 0.0
    else:
        near = AR.near_of(block)
        delta = SR.persp_delta(z, near)
    s, _, _, (_, _, ld) = SR.lookup_f64([pos[:, 0], pos[:, 1], pos[:, 2]], p)
    tol_sh, tol_ld = SR.surface_tols(pos, delta, p)
    near_ld = (np.abs(ld) <= tol_ld) | (np.abs(ld - 1.0) <= tol_ld) | (np.abs(ld - float(p["bias"])) <= tol_ld)

    def full(a, fill, dt=np.float64):
        out = np.full(n, fill, dt)
        out[vis] = a
        return out

    return dict(exact=False, dist=full(np.sqrt(((pos - cp) ** 2).sum(1)), np.inf), sh=full(s, 0.0), delta=full(delta, 0.0), tol_sh=full(tol_sh, 0.0),
                near_ld=full(near_ld, False, bool), z=full(z, 0.0), near=near, p=p)


def t_tolerance(pt, wd):
    """What the fade's t may be off by where dist is an unprojected one (atmosphere_ref: surface_t_tol; delta of the orthographic cameras
    in the place of the perspective one's)."""
    p = AR.params(atmosphere_of(pt))
    if wd["exact"]:
        return np.zeros_like(wd["dist"])
    if pt.cam == "persp":
        return AR.surface_t_tol(wd["z"], wd["near"], p)
    return wd["delta"] * float(p["fade_inv"]) + 4.0 * AR.U


def draw_index(case):
    """The draw every instance belongs to, and the mask of the draws in a LOD transition."""
    draws = OR.golden(case)["draws"]
    idx = np.concatenate([np.full(len(np.asarray(d.gs_index)), k, np.int64) for k, d in enumerate(draws)])
    return idx, np.array([d.tile.changing == 1 for d in draws])


# ---- colour -----------------------------------------------------------------------------------------------------------------------------------
def colour_f32(rgb0, sty, sh, p):
    """how = "exact": the binary32 chain of the module docstring over the record's own floats rgb0 [n, 3]."""
    rgb0, sh = np.asarray(rgb0, F32), np.asarray(sh, F32)
    tinted = TR.classes(sty)[2]
    c = TR.tinted_rgb(rgb0, sty)
    one = F32(1.0)
    for k in range(3):
        c[:, k] = np.where(sh != 0, (c[:, k] * (one - sh)).astype(F32) + (p["shade"][k] * sh).astype(F32), c[:, k])
    touched = tinted | (sh != 0)
    q = (SR.quantise_f32(c) / F32(255.0)).astype(F32)
    return np.where(touched[:, None], q, rgb0).astype(F32)


ORDER = ("tint", "shadow", "fog")


def codes_f64(rgb0, sty, sh, p, dist, fog_p, order=ORDER, requantise_after_tint=False):
    """The unrounded 255 c' in float64 with the three colour stages in `order` (sh = None / fog_p = None: that stage is off) -- the stack's
    own order through SR.chain_codes_f64, per tint; any other order, or a second quantisation behind the tint, is a mutation for
    tests/test_mode_stack_cpu.py's order check."""
    rgb0 = np.asarray(rgb0, np.float64)
    n = rgb0.shape[0]
    tinted = TR.classes(sty)[2]
    s = np.zeros(n) if sh is None else np.asarray(sh, np.float64)
    if tuple(order) == ORDER and not requantise_after_tint:
        out = np.zeros((n, 3))
        tints = {None: ~tinted}
        for t in {tuple(r) for r in sty[tinted][:, :4].tolist()}:
            tints[t] = tinted & (sty[:, :4] == np.array(t, np.uint8)).all(1)
        for t, m in tints.items():
            if m.any():
                out[m] = SR.chain_codes_f64(rgb0[m], t, s[m], p, None if fog_p is None else np.asarray(dist, np.float64)[m], fog_p)
        return out
    return staged_codes_f64(rgb0, sty, s, p, dist, fog_p, order, requantise_after_tint)


def staged_codes_f64(rgb0, sty, s, p, dist, fog_p, order=ORDER, requantise_after_tint=False):
    """codes_f64 stage by stage, in any order (in the stack's own it is chain_codes_f64 up to float64 rounding)."""
    tinted = TR.classes(sty)[2]
    c = np.asarray(rgb0, np.float64).copy()
    for stage in order:
        if stage == "tint":
            k = (sty[:, 3].astype(np.float64) / 255.0)[:, None] * tinted[:, None]
            c = c * (1.0 - k) + sty[:, :3].astype(np.float64) / 255.0 * k
            if requantise_after_tint:
                c = np.where(tinted[:, None], np.rint(np.clip(c, 0.0, 1.0) * 255.0) / 255.0, c)
        elif stage == "shadow":
            c = c * (1.0 - s[:, None]) + p["shade"].astype(np.float64)[None, :] * s[:, None]
        elif fog_p is not None:
            F = AR.fog_amount_f64(dist, fog_p)[:, None]
            c = c * (1.0 - F) + fog_p["fog_color"].astype(np.float64)[None, :] * F
    return 255.0 * np.clip(c, 0.0, 1.0)


# ---- the stack ----------------------------------------------------------------------------------------------------------------------------------
def stack(pt: Point, base=None) -> dict:
    """The expected records of the point.  `base` (geometry of the visible ones), `visible`, `alpha` (binary32, exact), `how` and with it
    `rgb` (binary32 floats, "exact") or `codes` (float64) with `bound` [n] ("bound": codes a byte may be off by) and `masked` [n]; and
    what the population conditions read: `sty`, `sh`, `dist`, `t`, `F`, `alpha_base` (the unmoded frame's alpha).
    base: other base records of the same instances under the point's filter and fade (tests/debug_modes_ref.py: the point cloud's); what the
    world gives stays that of the case's own centres, which a point cloud does not move."""
    inp = inputs(pt.case)
    if base is None:
        base = base_records(pt.case, pt.cam, pt.aa, pt.fade)
    unf = base_records(pt.case, pt.cam, False, False)
    wd = world(pt.case, pt.cam)
    n = base.shape[0]
    ids = PR.identities(OR.golden(pt.case)["draws"])[0]
    sty = TR.lookup(inp.entries, ids) if pt.sty else np.zeros((n, 5), np.uint8)
    hidden = TR.classes(sty)[0]
    visible = (base["visible"] == 1) & ~hidden
    atm_p = AR.params(atmosphere_of(pt))
    sh = wd["sh"] if pt.shd else np.zeros(n, wd["sh"].dtype)
    with np.errstate(all="ignore"):
        t = AR.fade_f64(wd["dist"], atm_p)[0] if pt.fade else np.ones(n)
        F = AR.fog_amount_f64(np.where(np.isfinite(wd["dist"]), wd["dist"], 0.0), atm_p) if pt.fog else np.zeros(n)
    out = dict(point=pt, base=base, visible=visible, alpha=TR.dimmed_alpha(base["rgba"][:, 3], sty), sty=sty, sh=np.asarray(sh, np.float64), dist=wd["dist"],
               t=t, F=F, alpha_base=unf["rgba"][:, 3], masked=np.zeros(n, bool), bound=np.zeros(n))
    rgb0 = base["rgba"][:, :3]
    if not pt.fog and (wd["exact"] or not pt.shd):
        out.update(how="exact", rgb=colour_f32(rgb0, sty, sh, wd["p"]))
        return out
    dist = np.where(np.isfinite(wd["dist"]), wd["dist"], 0.0)
    out["codes"] = codes_f64(rgb0, sty, sh if pt.shd else None, wd["p"], dist, atm_p if pt.fog else None)
    if wd["exact"]:
        out["how"] = "rint"
        return out
    tol = np.zeros(n)
    masked = np.zeros(n, bool)
    if pt.shd:
        tol += 255.0 * wd["tol_sh"]
        masked |= wd["near_ld"]
    if pt.fog:
        tol += 255.0 * float(atm_p["fog_max"]) * float(atm_p["fog_density"]) * wd["delta"]
    if pt.fade:
        with np.errstate(all="ignore"):
            raw = (float(atm_p["fade_end"]) - wd["dist"]) * float(atm_p["fade_inv"])
        masked |= np.abs(raw) <= t_tolerance(pt, wd)
    out.update(how="bound", bound=0.5 + tol + SR.MARGIN, masked=masked)
    return out


# ---- the populations -----------------------------------------------------------------------------------------------------------------------------
def populations(st) -> dict:
    """Counts of the splats on which the point's modes act and meet, from the reference alone; a key is there only where its modes are on."""
    pt = st["point"]
    unf = base_records(pt.case, pt.cam, False, False)
    vis0 = unf["visible"] == 1
    vis = st["visible"]
    hidden, _, tinted, _ = TR.classes(st["sty"])
    dim = (st["sty"][:, 4] > 0) & (st["sty"][:, 4] < 255)
    shadowed, fogged = st["sh"] != 0, st["F"] > 0
    ramp = (st["t"] > 0) & (st["t"] < 1)
    pop = dict(visible=int(vis.sum()), of=int(vis0.sum()))
    if pt.sty:
        # otherwise visible: by every other discard of the point
        pop["discard_hide"] = int(((st["base"]["visible"] == 1) & hidden).sum())
        pop["alpha_dim"] = int((vis & dim).sum())
    if pt.fade:
        pop["discard_fade"] = int(((base_records(pt.case, pt.cam, pt.aa, False)["visible"] == 1) & ~hidden & (st["base"]["visible"] != 1)).sum())
        pop["alpha_fade"] = int((vis & ramp).sum())
        idx, changing = draw_index(pt.case)
        pop["lod_transition_kept"] = int((vis & changing[idx]).sum())
    if pt.aa:
        pop["alpha_comp"] = int((vis & (base_records(pt.case, pt.cam, True, False)["rgba"][:, 3] != unf["rgba"][:, 3])).sum())
    if pt.fade and pt.sty:
        pop["ramp_and_dim"] = int((vis & ramp & dim).sum())
    on = dict(tint=(pt.sty, tinted), shadow=(pt.shd, shadowed), fog=(pt.fog, fogged))
    names = [k for k, (b, _) in on.items() if b]
    for i, a in enumerate(names):
        for b in names[i + 1:]:
            pop[f"{a}+{b}"] = int((vis & on[a][1] & on[b][1]).sum())
    if len(names) == 3:
        pop["tint+shadow+fog"] = int((vis & tinted & shadowed & fogged).sum())
    if st["how"] == "bound":
        pop["masked"] = int((vis & st["masked"]).sum())
    elif st["how"] == "rint":
        pop["near_half"] = int(AR.fog_bytes(st["codes"][vis])[1].sum())
    return pop


# ---- the comparison ---------------------------------------------------------------------------------------------------------------------------------
def check_records(got, n_visible, st, nan_equal=False, colour=True):
    """Projected records `got` (orc.SPLAT_DTYPE) and the frame's n_visible against the stack `st`.  Returns a line for the log.
    nan_equal: a field of a visible record that is a NaN on both sides counts as equal whatever its payload (FM.bits_equal_or_nan, for the
    hostile cases of tests/hostile_cases.py); colour=False: `visible`, n_visible, geometry and alpha only."""
    pt, vis, base = st["point"], st["visible"], st["base"]
    label = pt.id
    same = FM.bits_equal_or_nan if nan_equal else FM.bits_equal
    assert got.shape == base.shape, label
    assert np.array_equal(got["visible"] == 1, vis), (label, "visible", int((got["visible"] == 1).sum()), int(vis.sum()), np.flatnonzero((got["visible"] == 1) != vis)[:8])
    assert n_visible == int(vis.sum()), label
    for fld in GEOMETRY:
        assert same(np.ascontiguousarray(got[fld][vis]), np.ascontiguousarray(base[fld][vis])), (label, fld)
    assert same(got["rgba"][vis][:, 3].copy(), st["alpha"][vis].copy()), (label, "alpha")
    if not colour:
        return f"{label}: visible, geometry and alpha bit for bit on {int(vis.sum())} splats, colour not compared"
    if st["how"] == "exact":
        assert same(np.ascontiguousarray(got["rgba"][vis][:, :3]), np.ascontiguousarray(st["rgb"][vis])), (label, "colour")
        return f"{label}: colour bit for bit on {int(vis.sum())} splats"
    codes = got["rgba"][vis][:, :3].astype(np.float64) * 255.0
    have = np.rint(codes)
    assert np.abs(codes - have).max() < 1e-4, label                         # rgba[k] = (float)byte' / 255.0f
    if st["how"] == "rint":
        want, near_half = AR.fog_bytes(st["codes"][vis])
        assert near_half.mean() <= AR.MAX_MASKED, label
        assert np.abs(have - want).max() <= 1.0, label
        assert np.array_equal(have[~near_half], want[~near_half]), label
        return f"{label}: {int(near_half.sum())} channels inside the margin, {int((have != want).sum())} bytes off the float64 rint"
    ok = ~st["masked"][vis]
    assert (~ok).mean() <= AR.MAX_MASKED, label
    err = np.abs(have - st["codes"][vis]).max(1)
    bound = st["bound"][vis]
    ratio = float(np.max((err / bound)[ok]))
    used = float(np.max(((err - 0.5) / (bound - 0.5))[ok]))                  # of the derived part, behind the byte's own half code
    line = (f"{label}: {int((~ok).sum())} masked of {int(vis.sum())}, max err / bound {ratio:.3f} (largest bound {bound[ok].max():.3f} codes), "
            f"max (err - 0.5) / (bound - 0.5) {used:.3f}")
    assert (err <= bound)[ok].all(), line
    return line
