"""CPU references of the anti-aliasing filter (GSWT_OPT_ANTIALIAS, include/gswt_hip.h), in numpy (no tests here).

The filter is defined on the two eigenvalues of cov2d, after the strict vertex stage has decided rejection and direction on the
unfiltered ones: with s = 4 v / splat_scale^2, v = value / 1024 px^2,

    l1f = l1 + s;  l2f = l2 + s;
    smaj = min(sqrt(2 l1f), 1024);   smin = min(sqrt(2 l2f), 1024);
    comp = clamp(sqrt(l1 / l1f) * sqrt(l2 / l2f), 0, 1)        alpha' = alpha comp

(a) filter_records: the expected filtered records from UNFILTERED vertex-stage records (the oracle's, or tests/ortho_ref.py's), in
    float64: l1 = |major|^2 / 2, l2 = |minor|^2 / 2 are read back from the stored axes, the formulas applied, the axes rebuilt along the
    stored directions.
(b) filter_f32: the three lines as the kernel evaluates them, one np.float32 operation per written operator.
(c) lattice_mass: the float64 brute-force sum of a splat's fragment weights over pixel centres, for the known-answer tests.

s itself is an input of the definition, not a result: aa_s restates the host's binary32 expression, and (a) and (c) take that number."""
from __future__ import annotations

import math

import numpy as np

F32 = np.float32
U = 2.0 ** -24                      # unit roundoff of binary32
CLAMP = 1024.0                      # the axis clamp of gswt.wgsl:257-258

# Relative tolerance of |major|, |minor| and alpha of a filtered GPU record against filter_records of the unfiltered one:
# (the largest relative error of filter_f32 against float64 on the grid of tests/test_antialias_cpu.py + the 4 ulp that reading the
# eigenvalues back from binary32 axes costs) x 2, in units of 2^-24.  The measured maximum is 3.53 (comp; smaj and smin 1.49; the
# first-order worst case of the operator chains is 5 and 1.5); it is recorded here rounded up to the next integer, and
# tests/test_antialias_cpu.py fails if its measurement ever exceeds the recorded figure.
F32_MEASURED_ULP = 4.0
VARYINGS_RTOL = (F32_MEASURED_ULP + 4.0) * U * 2.0
DIRECTION_ATOL = 4.0 * U


def aa_s(value: int, splat_scale) -> np.float32:
    """s as the host computes it once per frame: (4.0f * v) / (splat_scale * splat_scale) in binary32, v = value / 1024 exact."""
    assert 0 <= int(value) <= 4096
    v = F32(int(value)) / F32(1024.0)
    sc = F32(splat_scale)
    with np.errstate(all="ignore"):
        return F32((F32(4.0) * v) / (sc * sc))


def _clamp01(e):
    return np.fmin(np.fmax(e, F32(0.0)), F32(1.0))          # fminf(fmaxf(e, 0), 1): a NaN gives 0


def filter_f32(l1, l2, s):
    """(smaj, smin, comp) from binary32 eigenvalues and s, operator by operator in np.float32 (element-wise numpy float32 operations
    are single IEEE operations)."""
    l1, l2, s = np.asarray(l1, F32), np.asarray(l2, F32), np.asarray(s, F32)
    with np.errstate(all="ignore"):
        l1f = l1 + s
        l2f = l2 + s
        smaj = np.fmin(np.sqrt(F32(2.0) * l1f), F32(CLAMP))
        smin = np.fmin(np.sqrt(F32(2.0) * l2f), F32(CLAMP))
        comp = _clamp01(np.sqrt(l1 / l1f) * np.sqrt(l2 / l2f))
    return smaj, smin, comp


def filter_f64(l1, l2, s):
    """The same three lines in float64."""
    l1, l2, s = np.asarray(l1, np.float64), np.asarray(l2, np.float64), np.asarray(s, np.float64)
    with np.errstate(all="ignore"):
        l1f, l2f = l1 + s, l2 + s
        smaj = np.minimum(np.sqrt(2.0 * l1f), CLAMP)
        smin = np.minimum(np.sqrt(2.0 * l2f), CLAMP)
        comp = np.sqrt(l1 / l1f) * np.sqrt(l2 / l2f)
        comp = np.where(np.isnan(comp), 0.0, np.clip(comp, 0.0, 1.0))
    return smaj, smin, comp


def filter_records(sp, value: int, splat_scale):
    """Expected filtered records of the unfiltered records `sp` (orc.SPLAT_DTYPE), in float64.

    Returns (out, masked, n_masked): out is a dict of float64 arrays -- `major`, `minor` [n, 2], their lengths `len_major`,
    `len_minor`, the unit directions `dir_major`, `dir_minor` (the minor one is the major one turned, (ey, -ex): the stored minor axis
    of a splat with l2 == 0 has no direction of its own), `alpha`, `comp`, and `l1`, `l2` as read back; masked [n] marks the visible
    records whose unfiltered or filtered axis sits at the 1024 clamp (the eigenvalue cannot be read back from a clamped axis).
    value = 0 returns the input's own axes and alpha bit for bit (as float64)."""
    maj, mnr = sp["major"].astype(np.float64), sp["minor"].astype(np.float64)
    alpha = sp["rgba"][:, 3].astype(np.float64)
    vis = sp["visible"] == 1
    len_maj, len_mnr = np.hypot(maj[:, 0], maj[:, 1]), np.hypot(mnr[:, 0], mnr[:, 1])
    with np.errstate(all="ignore"):
        d_maj = maj / len_maj[:, None]
    d_mnr = np.stack([d_maj[:, 1], -d_maj[:, 0]], -1)
    l1, l2 = 0.5 * len_maj * len_maj, 0.5 * len_mnr * len_mnr
    if int(value) == 0:
        out = dict(major=maj, minor=mnr, len_major=len_maj, len_minor=len_mnr, dir_major=d_maj, dir_minor=d_mnr, alpha=alpha,
                   comp=np.ones_like(alpha), l1=l1, l2=l2)
        return out, np.zeros(len(sp), bool), 0
    s = float(aa_s(value, splat_scale))
    smaj, smin, comp = filter_f64(l1, l2, s)
    edge = CLAMP * (1.0 - 8.0 * U)
    masked = vis & ((len_maj >= edge) | (len_mnr >= edge) | (smaj >= edge) | (smin >= edge))
    out = dict(major=smaj[:, None] * d_maj, minor=smin[:, None] * d_mnr, len_major=smaj, len_minor=smin, dir_major=d_maj,
               dir_minor=d_mnr, alpha=alpha * comp, comp=comp, l1=l1, l2=l2)
    return out, masked, int(masked.sum())


def analytic_mass(l1, l2, splat_scale, alpha=1.0):
    """Integral of a splat's fragment weight alpha exp(-|p|^2) over |p|^2 <= 4, in pixels: the pixel offset is x = 0.5 splat_scale
    (p.x major + p.y minor) with |major| |minor| = 2 sqrt(l1 l2), so d2x = 0.5 splat_scale^2 sqrt(l1 l2) d2p, and the integral of
    exp(-|p|^2) over the disc of radius 2 is pi (1 - e^-4).  With the filter on, comp sqrt(l1f l2f) = sqrt(l1 l2): the same number."""
    return alpha * (1.0 - math.exp(-4.0)) * math.pi * 0.5 * float(splat_scale) ** 2 * math.sqrt(float(l1) * float(l2))


def lattice_mass(l1, l2, theta, cx, cy, splat_scale, value: int = 0, alpha=1.0, with_count=False):
    """Sum over pixel centres (i + 0.5, j + 0.5) of alpha comp exp(-|p|^2) inside |p|^2 <= 4 for one isolated splat whose cov2d has
    eigenvalues l1 >= l2 and major direction (cos theta, sin theta) on screen, centre (cx, cy) in pixels; float64, brute force.
    with_count: also the number of pixel centres inside."""
    s = float(aa_s(value, splat_scale)) if int(value) else 0.0
    smaj, smin, comp = (float(x) for x in filter_f64(l1, l2, s))
    hs = 0.5 * float(splat_scale)
    ex, ey = math.cos(theta), math.sin(theta)
    ux, uy = hs * smaj * ex, hs * smaj * ey                  # the two half axes in pixels
    vx, vy = hs * smin * ey, -hs * smin * ex
    uu, vv = ux * ux + uy * uy, vx * vx + vy * vy
    if not (uu > 0.0 and vv > 0.0):
        return (0.0, 0) if with_count else 0.0
    reach = 2.0 * math.sqrt(uu) + 1.0
    xs = np.arange(math.floor(cx - reach) - 1, math.ceil(cx + reach) + 2) + 0.5
    ys = np.arange(math.floor(cy - reach) - 1, math.ceil(cy + reach) + 2) + 0.5
    dx, dy = np.meshgrid(xs - cx, ys - cy)
    pu, pv = (dx * ux + dy * uy) / uu, (dx * vx + dy * vy) / vv
    r2 = pu * pu + pv * pv
    inside = r2 <= 4.0
    m = float(alpha * comp * np.exp(-r2[inside]).sum())
    return (m, int(inside.sum())) if with_count else m


def lattice_bound(l1, l2, splat_scale, value: int):
    """Relative bound of |lattice_mass / analytic_mass - 1| with the filter at `value` > 0, from reasoning (not from measurements):

    The weight is g = exp(-|p|^2) cut off at |p| = 2, where it still is e^-4.  Write g = G - h + e^-4 1_E: G the whole Gaussian, E the
    ellipse |p| <= 2, h = min(G, e^-4) (continuous).  The lattice sums of the smooth parts G and h equal their integrals up to aliasing:
    by Poisson summation the relative error for a Gaussian whose on-screen variance is at least v in every direction is at most
    4 exp(-2 pi^2 v) (four nearest frequencies; 2.1e-4 at v = 0.5, which is why the tests use value = 512), and h, bounded by e^-4 and
    with only a gradient kink, adds less still: 2e-3 covers both with room.  The lattice sum of 1_E is the number N of pixel centres
    in a convex region of area A and perimeter P, and |N - A| <= P / 2 + 1 (Nosarzewska 1948 from above, Bokowski, Hadwiger and Wills
    1972 from below).  The mass is pi (1 - e^-4) A / (4 pi) -- the ellipse is the image of a disc of area 4 pi --, so

        |ratio - 1| <= 4 e^-4 (P / 2 + 1) / ((1 - e^-4) A) + 2e-3,    P <= 2 pi sqrt((a^2 + b^2) / 2)

    a, b the half axes of E in pixels: splat_scale sqrt(2 l1f), splat_scale sqrt(2 l2f).  4.5 % for the smallest ellipse at
    value = 512 (a = b = 2 px), less for larger ones."""
    s = float(aa_s(value, splat_scale))
    a = float(splat_scale) * math.sqrt(2.0 * (float(l1) + s))
    b = float(splat_scale) * math.sqrt(2.0 * (float(l2) + s))
    area = math.pi * a * b
    perim = 2.0 * math.pi * math.sqrt(0.5 * (a * a + b * b))
    return 4.0 * math.exp(-4.0) * (0.5 * perim + 1.0) / ((1.0 - math.exp(-4.0)) * area) + 2e-3
