"""The HIP path on splat records outside the benign region of synth.make_tile (tests/special_splats.py), against the CPU oracle:
the known-answer scenes K9-K15 of tests/test_oracle_kat.py rendered on the GPU, every f16 pattern of a covariance slot through the
vertex stage, hostile tile sets end to end (every compositor, depth-sort path, chunk cull and shard mode), the hostile presort's
per-splat varyings, exact depth ties, and the column-band cull on covariances the decode leaves indefinite."""

import numpy as np
import pytest

from gswt_renderer_amd import _lib as L
from oracle import gswt_oracle as orc
from tests import helpers as H
from tests import special_splats as S
from tests.test_end_to_end_gpu import _run_case

pytestmark = pytest.mark.gpu
TOL = 1e-4
MAX_PAIRS = 1 << 22
ORDERS = [L.GSWT_ORDER_REFERENCE, L.GSWT_ORDER_DEPTH]


def _frame(renderer, scene, pdraws, cu, su, W, Hh, **kw):
    renderer.configure(None)
    scene.upload(renderer)
    renderer.set_draws(pdraws)
    img = renderer.render(cu, su, W, Hh, **kw)
    return img, renderer.timings()


def _parity(renderer, scene, cu, su, W, Hh, order_mode, *, view=0, bg_rgba=None, bg_depth=None, **tile_kw):
    """Render one raw scene on both sides; n_visible / n_pairs equal, image within TOL.  -> (gpu image, oracle image, oracle stats)."""
    od, pd = scene.draws(view=view, **tile_kw)
    ref, st = orc.render(cu, su, scene.tex, od, W, Hh, bg_rgba=bg_rgba, bg_depth=bg_depth, order_mode=order_mode)
    assert st["n_pairs16"] < MAX_PAIRS
    img, t = _frame(renderer, scene, pd, cu, su, W, Hh, order_mode=order_mode, bg_rgba=bg_rgba, bg_depth=bg_depth)
    assert t["n_visible"] == st["n_visible"] and t["n_pairs"] == st["n_pairs16"], (t, st)
    assert H.max_abs_diff(img, ref) <= TOL
    return img, ref, st


def _varyings(renderer, scene, pdraws, cu, su, W, Hh):
    with renderer.options(NO_LOD_PREFILTER=1, DEBUG_VARYINGS=1):
        _frame(renderer, scene, pdraws, cu, su, W, Hh)
        return renderer.read_projected()


def _assert_varyings_equal(got, want, what=""):
    """visible equal for every splat; ndc, depth, major, minor, rgba bitwise equal for the visible ones.  A field that is NaN on both
    sides counts as equal whatever its payload (NaN only: an Inf or a finite value must match bit for bit)."""
    assert got.shape == want.shape
    # the product's debug flag is set after fragment setup F1 / F2 (|major|^2, |minor|^2 in (0, inf)), which the oracle applies in
    # orc_render (frag_setup) rather than in orc_project: a vertex-stage survivor with a zero or infinite axis draws nothing on either
    # side, so the oracle's flag is restated with that test (float32, as the kernel)
    want = want.copy()
    hs = np.float32(0.5)
    maj, mnr = want["major"].astype(np.float32), want["minor"].astype(np.float32)
    with np.errstate(all="ignore"):
        uu = (np.float64(hs * maj[:, 1]) ** 2 + np.float64((hs * maj[:, 0]) * (hs * maj[:, 0]))).astype(np.float32)
        ww = (np.float64(hs * mnr[:, 1]) ** 2 + np.float64((hs * mnr[:, 0]) * (hs * mnr[:, 0]))).astype(np.float32)
    ok = (uu > 0) & (ww > 0) & (uu < np.inf) & (ww < np.inf)
    want["visible"] = np.where(ok, want["visible"], 0)
    bad = np.flatnonzero(got["visible"] != want["visible"])
    assert bad.size == 0, (what, "visible", bad[:8], got["visible"][bad[:8]], want["visible"][bad[:8]])
    vis = want["visible"] == 1
    for fld in ("ndc", "depth", "major", "minor", "rgba"):
        a, b = got[fld][vis], want[fld][vis]
        same = (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))
        if same.ndim > 1:
            same = same.all(axis=1)
        bad = np.flatnonzero(~same)
        assert bad.size == 0, (what, fld, np.flatnonzero(vis)[bad[:8]], a[bad[:4]], b[bad[:4]])
    return int(vis.sum())


# ---- K9 - K15 through the HIP path --------------------------------------------------------------------------------------
def _one(pos, sigma, rgba=(255, 128, 0, 255)):
    return S.raw_scene([(pos, S.diag_halves(sigma), rgba)])


@pytest.mark.parametrize("order_mode", ORDERS)
def test_k9_single_splat_analytic(renderer, order_mode):
    W, Hh, D = 64, 48, 4.0
    cu = orc.default_camera(W, Hh).uniforms()
    sig = (0.05, 0.05, 0.1)
    img, ref, st = _parity(renderer, _one((0.0, D, 5.0), sig), cu, orc.scene_uniforms(num_lod=1), W, Hh, order_mode, valid_lod_id=0)
    assert st["n_visible"] == 1
    sx_px, sy_px = sig[0] * cu.focal[0] / D, sig[2] * cu.focal[1] / D
    ys, xs = np.mgrid[0:Hh, 0:W]
    dx, dy = xs + 0.5 - W / 2, ys + 0.5 - Hh / 2
    r2 = dx * dx / (2 * sx_px * sx_px) + dy * dy / (2 * sy_px * sy_px)
    want_a = np.where(r2 <= 4.0, np.exp(-r2), 0.0)
    assert np.allclose(img[..., 3], want_a, atol=2e-3)
    assert np.allclose(img[..., 0], want_a, atol=2e-3)
    assert np.allclose(img[..., 1], want_a * (128 / 255), atol=2e-3)
    assert img[..., 2].max() == 0.0 and img[Hh // 2, W // 2, 3] > 0.5


@pytest.mark.parametrize("order_mode", ORDERS)
def test_k9_exactly_isotropic_centred_splat_draws_nothing(renderer, order_mode):
    W = Hh = 64
    cu = orc.default_camera(W, Hh).uniforms()
    img, ref, st = _parity(renderer, _one((0.0, 4.0, 5.0), (0.05, 0.05, 0.05)), cu, orc.scene_uniforms(num_lod=1), W, Hh, order_mode,
                           valid_lod_id=0)
    assert st["n_visible"] == 0 and renderer.timings()["n_visible"] == 0
    assert not img.any()                                          # normalize(vec2(0, 0)) -> NaN axes: nothing, not even -0.0


@pytest.mark.parametrize("order_mode", ORDERS)
def test_k10_two_splats_over(renderer, order_mode):
    W = Hh = 32
    cu = orc.default_camera(W, Hh).uniforms()
    su = orc.scene_uniforms(num_lod=1)
    far = ((0.0, 6.0, 5.0), S.diag_halves((0.4, 0.4, 0.5)), (255, 0, 0, 128))
    near = ((0.0, 3.0, 5.0), S.diag_halves((0.2, 0.2, 0.25)), (0, 0, 255, 128))
    sc = S.raw_scene([far, near], lists=[([0, 1], [0, 0]), ([1, 0], [0, 0])])
    both, _, _ = _parity(renderer, sc, cu, su, W, Hh, order_mode, view=0, valid_lod_id=0)
    rev, _, _ = _parity(renderer, sc, cu, su, W, Hh, order_mode, view=1, valid_lod_id=0)
    f_img, _, _ = _parity(renderer, S.raw_scene([far]), cu, su, W, Hh, order_mode, valid_lod_id=0)
    n_img, _, _ = _parity(renderer, S.raw_scene([near]), cu, su, W, Hh, order_mode, valid_lod_id=0)
    assert np.allclose(both, n_img + f_img * (1.0 - n_img[..., 3:4]), atol=1e-6)      # far first, near "over" it
    if order_mode == L.GSWT_ORDER_REFERENCE:
        assert np.abs(rev - both).max() > 0.05                 # the draw order decides
    else:
        assert H.max_abs_diff(rev, both) <= TOL                # depth order: the list order does not matter


@pytest.mark.parametrize("dist,t_expected", [(9.5, 0.0), (9.75, 0.0), (10.0, 0.5), (10.125, 0.75), (10.25, 1.0), (10.5, 1.0)])
def test_k11_lod_transition_ratio(renderer, dist, t_expected):
    W = Hh = 32
    cu = orc.default_camera(W, Hh).uniforms()
    su = orc.scene_uniforms(num_lod=2, transition_width_ratio=0.05, transition_dist=(10.0, 20.0))
    sc = S.raw_scene([((0.0, dist, 5.0), S.diag_halves((0.3, 0.3, 0.35)), (255, 255, 255, 255))],
                     lists=[([0], [0]), ([0], [1])], n_lod=2)
    for lod_id in (0, 1):
        od, pd = sc.draws(view=lod_id, changing=1, changing_to_lower=1, tile_id=(0, 0, 0))
        want = orc.project_draws(cu, su, sc.tex, od)
        got = _varyings(renderer, sc, pd, cu, su, W, Hh)
        _assert_varyings_equal(got, want, (dist, lod_id))
        sp = got[0]
        if (lod_id == 0 and t_expected == 1.0) or (lod_id == 1 and t_expected == 0.0):
            assert sp["visible"] == 0
        else:
            assert sp["visible"] == 1
            assert abs(sp["rgba"][3] - ((1.0 - t_expected) if lod_id == 0 else t_expected)) < 1e-5
        for order_mode in ORDERS:
            _parity(renderer, sc, cu, su, W, Hh, order_mode, view=lod_id, changing=1, changing_to_lower=1, tile_id=(0, 0, 0))


@pytest.mark.parametrize("order_mode", ORDERS)
def test_k14_depth_test_at_equality(renderer, order_mode):
    W = Hh = 32
    cu = orc.default_camera(W, Hh).uniforms()
    su = orc.scene_uniforms(num_lod=1)
    sc = _one((0.0, 5.0, 5.0), (0.5, 0.5, 0.6), (255, 255, 255, 255))
    od, _ = sc.draws(valid_lod_id=0)
    depth = np.float32(orc.project_draws(cu, su, sc.tex, od)[0]["depth"])
    bg = np.full((Hh, W, 4), 0.25, dtype=np.float32)
    behind, _, _ = _parity(renderer, sc, cu, su, W, Hh, order_mode, bg_rgba=bg, bg_depth=np.full((Hh, W), depth, np.float32), valid_lod_id=0)
    assert np.array_equal(behind, bg)                              # depth < depthbuf fails on equality: the background, bit for bit
    front, _, _ = _parity(renderer, sc, cu, su, W, Hh, order_mode, bg_rgba=bg,
                          bg_depth=np.full((Hh, W), np.nextafter(depth, np.float32(2.0)), np.float32), valid_lod_id=0)
    assert front[Hh // 2, W // 2, 0] > 0.9


@pytest.mark.parametrize("order_mode", ORDERS)
def test_k15_near_far_clip(renderer, order_mode):
    W = Hh = 32
    cu = orc.default_camera(W, Hh).uniforms()
    su = orc.scene_uniforms(num_lod=1)
    for y, vis in ((0.05, 0), (0.2, 1), (2399.0, 1), (2500.0, 0), (-1.0, 0)):
        sc = _one((0.0, y, 5.0), (0.01, 0.01, 0.012))
        od, pd = sc.draws(valid_lod_id=0)
        got = _varyings(renderer, sc, pd, cu, su, W, Hh)
        _assert_varyings_equal(got, orc.project_draws(cu, su, sc.tex, od), y)
        assert got[0]["visible"] == vis, y
        _parity(renderer, sc, cu, su, W, Hh, order_mode, valid_lod_id=0)
    # depth rounds to exactly 1.0: visible in the varyings, but the `Less` test against the 1.0 clear draws nothing
    sc = _one((0.0, 2401.0, 5.0), (30.0, 30.0, 36.0))
    od, pd = sc.draws(valid_lod_id=0)
    got = _varyings(renderer, sc, pd, cu, su, W, Hh)
    _assert_varyings_equal(got, orc.project_draws(cu, su, sc.tex, od))
    assert got[0]["visible"] == 1 and got[0]["depth"] == 1.0
    img, _, st = _parity(renderer, sc, cu, su, W, Hh, order_mode, valid_lod_id=0)
    assert not img.any() and renderer.timings()["n_visible"] == st["n_visible"]


# ---- every f16 pattern of a covariance slot through the vertex stage ------------------------------------------------------
@pytest.mark.parametrize("slot", ["xx", "xy"])
def test_every_half_pattern_through_the_vertex_stage(renderer, slot):
    """65 536 splats, one per pattern of the slot: the GPU's half decode (v_cvt_f32_f16, the 2^-15 subnormal scale, Inf / NaN -> 0)
    must give the oracle's varyings bit for bit.  xx: yy and zz small, so that even subnormal xx keep most splats visible.  xy:
    xx = yy, so that |xy| < xx stays positive definite, seen by a camera looking diagonally across x and y (at the screen centre of
    an axis-aligned view xy would not reach the 2D covariance)."""
    W, Hh = 32, 32
    pats = np.arange(65536)
    if slot == "xx":
        cu = orc.default_camera(W, Hh).uniforms()
        base = S.cov_halves(yy=1e-3, zz=1e-3)
        rows = [((0.0, 4.0, 5.0), [p] + base[1:], (200, 100, 50, 255)) for p in pats]
    else:
        cu = orc.Camera(W, Hh, (-3.0, 1.0, 5.0), (0.0, 4.0, 5.0), [0, 0, 1]).uniforms()
        base = S.cov_halves(xx=1.0, yy=1.0, zz=0.5)
        rows = [((0.0, 4.0, 5.0), [base[0], p] + base[2:], (200, 100, 50, 255)) for p in pats]
    sc = S.raw_scene(rows)
    su = orc.scene_uniforms(num_lod=1)
    od, pd = sc.draws(valid_lod_id=0)
    want = orc.project_draws(cu, su, sc.tex, od)
    n_vis = _assert_varyings_equal(_varyings(renderer, sc, pd, cu, su, W, Hh), want, slot)
    assert n_vis > 1000, n_vis
    # the decode's edge classes are in the visible set: subnormal, the smallest normal, Inf / NaN (-> 0)
    vis = want["visible"] == 1
    assert vis[0x0001:0x0400].sum() > 500 and vis[0x0400]
    if slot == "xy":
        assert vis[0x7C00] and vis[0x7E00] and vis[0xFC00]      # Inf / NaN xy read as 0: a plain diagonal covariance


# ---- hostile tile sets end to end -------------------------------------------------------------------------------------
HOSTILE_CFGS = {
    "plane": dict(tile_map_half_wh=(3, 3), surface_type=0, lod_max_dist=20.0, tile_sort_type=3, merge_type=2),
    "hmap": dict(tile_map_half_wh=(3, 3), surface_type=1, lod_max_dist=20.0, tile_sort_type=3, merge_type=2, height_map_type=4,
                 height_map_wh=(6, 6), height_map_scale=(1.0, 1.0, 0.4)),
}
HOSTILE_CAMS = {
    "level": ((4.2, 1.0, 1.5), (5.0, 3.0, 1.5)),
    "grazing": ((4.2, 1.0, 0.45), (9.0, 6.0, 0.0)),
    "closeup": ((4.3, 1.1, 0.25), (4.6, 1.6, 0.1)),           # inside floaters (log-scales +2 .. +7: radii of metres to kilometres)
}


def _hostile_verts(seed):
    return S.hostile_tileset(seed=seed, n_lod=3, lod0_count=500)[0]


@pytest.mark.parametrize("surface", ["plane", "hmap"])
@pytest.mark.parametrize("cam_name", list(HOSTILE_CAMS))
def test_hostile_tileset_end_to_end(renderer, surface, cam_name):
    cfg, cam = HOSTILE_CFGS[surface], HOSTILE_CAMS[cam_name]
    verts = _hostile_verts(1 if surface == "hmap" else 0)
    W, Hh = 320, 240
    for order_mode in ORDERS:
        sorts = (0, 1) if order_mode == L.GSWT_ORDER_DEPTH else (0,)
        for ds in sorts:
            with renderer.options(DEPTH_SORT=ds):
                for eps in (0.0, 1e-5):
                    img, ref, _, st = _run_case(renderer, cfg, cam, W, Hh, verts=verts, order_mode=order_mode, t_eps=eps, max_pairs=MAX_PAIRS)
                    assert np.isfinite(img).all(), (order_mode, ds, eps)
                    assert st["n_visible"] > 200, st
                    assert H.max_abs_diff(img, ref) <= TOL + eps, (order_mode, ds, eps, H.max_abs_diff(img, ref))


@pytest.mark.parametrize("surface", ["plane", "hmap"])
def test_hostile_tileset_variants_bitwise(renderer, surface):
    """On one hostile frame per camera: the chunk cull changes nothing, and the column-band and row-interleaved shard unions equal the
    unsharded image bit for bit -- the band cull's covariance bound and its "never cull" path on non-finite positions are what the hostile rows exercise."""
    cfg = HOSTILE_CFGS[surface]
    verts = _hostile_verts(1 if surface == "hmap" else 0)
    W, Hh = 320, 240
    for cam_name in ("level", "closeup"):
        cam = HOSTILE_CAMS[cam_name]
        for order_mode in ORDERS:
            full, ref, _, st = _run_case(renderer, cfg, cam, W, Hh, verts=verts, order_mode=order_mode, max_pairs=MAX_PAIRS)
            assert H.max_abs_diff(full, ref) <= TOL
            t_full = renderer.timings()
            with renderer.options(NO_CHUNK_CULL=1):
                img, _, _, _ = _run_case(renderer, cfg, cam, W, Hh, verts=verts, order_mode=order_mode, max_pairs=MAX_PAIRS)
                t = renderer.timings()
            assert np.array_equal(img, full), (cam_name, order_mode, float(np.abs(img - full).max()))
            assert (t["n_visible"], t["n_pairs"]) == (t_full["n_visible"], t_full["n_pairs"]), cam_name
            img, _, _, _ = _run_case(renderer, cfg, cam, W, Hh, verts=verts, order_mode=order_mode, shard=3, shard_cols=True)
            assert np.array_equal(img, full), (cam_name, order_mode, "cols")
            img, _, _, _ = _run_case(renderer, cfg, cam, W, Hh, verts=verts, order_mode=order_mode, shard=3)
            assert np.array_equal(img, full), (cam_name, order_mode, "rows")


@pytest.mark.parametrize("surface", ["plane", "hmap"])
def test_hostile_presort_vertex_stage_bit_exact(renderer, surface):
    pp = orc.preprocess([[orc.scene_load(v) for v in lod] for lod in _hostile_verts(0)])
    W, Hh = 320, 240
    hm = None
    kw = dict(scene_scale=(0.9, 1.2, 1.3))
    if surface == "hmap":
        hm = np.random.default_rng(5).random((16, 16), dtype=np.float32)
        kw.update(surface_type=1, height_map_scale=(1.0, 1.0, 0.4))
    su = orc.scene_uniforms(num_lod=pp.n_lod, map_half_wh=(1, 2), **kw)
    case = H.grid_case(pp, lod_of=lambda ix, iy: (ix + iy) % 3)
    cu = orc.default_camera(W, Hh).uniforms()
    with renderer.options(NO_LOD_PREFILTER=1, DEBUG_VARYINGS=1):
        try:
            renderer.configure(hm)
            case.upload(renderer)
            renderer.render(cu, su, W, Hh)
            got = renderer.read_projected()
        finally:
            renderer.configure(None)
    want = orc.project_draws(cu, su, pp.tex, case.orc_draws, height_map=hm)
    assert _assert_varyings_equal(got, want, surface) > 300


# ---- exact depth ties ------------------------------------------------------------------------------------------------
def test_exact_depth_ties_follow_the_oracle(renderer):
    """Groups of 2 and 3 splats at one position with one covariance and different colours: their depths tie exactly, so the depth
    order is the sort's tie rule alone -- both depth-sort paths must give the oracle's stable order (a swapped pair changes the
    pixel by ~0.1)."""
    W, Hh = 96, 64
    cu = orc.default_camera(W, Hh).uniforms()
    su = orc.scene_uniforms(num_lod=1)
    rng = np.random.default_rng(3)
    rows = []
    for g in range(12):
        pos = (rng.uniform(-1.5, 1.5), rng.uniform(3.0, 6.0), rng.uniform(4.2, 5.8))
        cov = S.diag_halves(rng.uniform(0.05, 0.3, 3))
        for j in range(2 + g % 2):
            rows.append((pos, cov, tuple(int(x) for x in rng.integers(0, 256, 3)) + (160,)))
    perm = rng.permutation(len(rows))
    sc = S.raw_scene(rows, lists=[(np.arange(len(rows)), np.zeros(len(rows))), (perm, np.zeros(len(rows)))])
    for view in (0, 1):
        for ds in (0, 1):
            with renderer.options(DEPTH_SORT=ds):
                img, ref, st = _parity(renderer, sc, cu, su, W, Hh, L.GSWT_ORDER_DEPTH, view=view, valid_lod_id=0)
            assert st["n_visible"] == len(rows)
    swapped = list(rows)
    swapped[0], swapped[1] = swapped[1], swapped[0]
    other, _ = orc.render(cu, su, S.raw_scene(swapped).tex, sc.draws()[0], W, Hh, order_mode=L.GSWT_ORDER_DEPTH)
    assert H.max_abs_diff(other, ref) > 0.01                       # the tie order is visible in the image


# ---- the column-band cull on covariances the decode leaves indefinite ---------------------------------------------------
@pytest.mark.parametrize("kind", ["overflowed_diagonal", "negative_diagonal"])
def test_column_bands_on_indefinite_decoded_covariance(renderer, kind):
    """gswt_upload_scene bounds every record's projected extent for the band cull.  The trace bounded it only for positive
    semi-definite decoded covariances; a diagonal that overflowed to Inf decodes to 0 beside finite off-diagonals, and a raw row may
    hold a negative diagonal -- the largest eigenvalue is then many times the trace.  One such splat to the right of the frame,
    reaching into the leftmost band: the band union must still be the unsharded image, bit for bit."""
    W, Hh, n = 320, 240, 3
    if kind == "overflowed_diagonal":
        # xx, yy stored as Inf (a flat floater: 4 s^2 > 65504) read as 0; xy = -3000 makes the decoded xy block indefinite (+-3000);
        # the camera looks about along (1, 1, 0), the negative eigenvector's direction, so the projection keeps the +3000 axis
        cov = [0x7C00, orc.float_to_half(-3000.0), orc.float_to_half(1.0), 0x7C00, 0, orc.float_to_half(2.0)]
        pos = (0.0, 0.0, 0.0)
        cam = orc.Camera(W, Hh, (-60.0, -59.0, 0.3), (0.0, 0.0, 0.0), [0, 0, 1])
    else:
        cov = S.cov_halves(xx=1000.0, yy=-1999.0, zz=1000.0)
        pos = (10.0, 60.0, 0.0)
        cam = orc.Camera(W, Hh, (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), [0, 0, 1])
    sc = S.raw_scene([(pos, cov, (255, 255, 255, 200))])
    cu = cam.uniforms()
    su = orc.scene_uniforms(num_lod=1)
    full, ref, st = _parity(renderer, sc, cu, su, W, Hh, L.GSWT_ORDER_REFERENCE, valid_lod_id=0)
    assert st["n_visible"] == 1
    assert ref[:, :W // n, 3].max() > 0.05 and ref[:, -W // n:, 3].max() > 0.05, "the splat must span the bands"
    _, pd = sc.draws(valid_lod_id=0)
    bw = renderer.shard_cols_padded(W, n)
    img = np.zeros_like(full)
    for r in range(n):
        part = renderer.render(cu, su, W, Hh, shard=(r, n, "cols"))
        x0, x1 = r * bw, min(W, (r + 1) * bw)
        img[:, x0:x1] = part[:, :x1 - x0]
    assert np.array_equal(img, full), [float(np.abs(img - full)[:, r * bw:(r + 1) * bw].max()) for r in range(n)]
