"""The sun shadows (gswt_set_shadow_map, include/gswt_hip.h) on the GPU: splats and proxy ground shaded by a light-space depth map.
Frames are 72 x 40 (tests/ortho_ref.py) on the golden cases with the draws of their own perspective sort event; maps are at most 64 x 64.

The shaded colour bytes bit for bit against tests/shadow_ref.py on the plain surface (perspective and both orthographic cameras) and
within the derived tolerance on the HeightMap and Sphere surfaces; known answers; the light's own depth frame fed back; image, depth
and pick against the CPU references over the GPU's own records; the same bits through graphs, frames in flight, the chunk cull
off, a pair-buffer overflow, output formats and shards; off leaves every output as it was; tint, shadow and fog in that order;
the refusals; the proxy passes; the pipeline's keyword."""
import ctypes as C
import struct

import numpy as np
import pytest

from gswt_renderer_amd import _lib as L
from gswt_renderer_amd import atmosphere as A
from gswt_renderer_amd import ortho, shadows
from gswt_renderer_amd import styles as ST
from gswt_renderer_amd.renderer import GSWTError
from oracle import gswt_oracle as orc
from tests import atmosphere_ref as AR
from tests import frame_modes as FM
from tests import ortho_ref as OR
from tests import proxy_ortho_ref as O
from tests import proxy_raster_ref as R
from tests import shadow_ref as SR
from tests import special_splats as S

pytestmark = pytest.mark.gpu
W, Hh = OR.W, OR.H
F32 = np.float32
ORTHO, PERSP = L.GSWT_PROJECTION_ORTHO, L.GSWT_PROJECTION_PERSPECTIVE
GEOMETRY = ("ndc", "depth", "major", "minor")
SHADE = (0.1, 0.05, 0.2)
LIGHT = SR.plane_light()
# the plane case's map, 32 x 24, and a second one of another size: a top-down light, 17 x 11, lit on the right
LIGHT_B = ortho.top_down(OR.CENTRE, 7.0, 10.0, -2.0, 17, 11)
MAPS = {"off": shadows.OFF,
        "a": shadows.from_ortho_camera(LIGHT, SR.plane_map(LIGHT), bias=0.002, strength=0.75, shade_color=SHADE),
        "b": shadows.from_ortho_camera(LIGHT_B, SR.two_region_map(17, 11), bias=0.0, strength=1.0, shade_color=(0.3, 0.0, 0.0))}


@pytest.fixture(autouse=True)
def _defaults(renderer):
    """FM.restore_defaults does not know the shadow map: the shared context goes back without one as well."""
    yield
    renderer.set_shadow_map(None)
    FM.restore_defaults(renderer)


def _block(cu):
    return orc.Camera176.from_buffer_copy(bytes(cu))


def _same_fields(got, base, m, fields, label):
    for fld in fields:
        assert FM.bits_equal(np.ascontiguousarray(got[fld][m]), np.ascontiguousarray(base[fld][m])), (label, fld)


def _codes(rgba):
    """(the bytes a record's float colours stand for, how far the floats are from byte / 255)."""
    codes = np.asarray(rgba, np.float64)[:, :3] * 255.0
    have = np.rint(codes)
    return have, float(np.abs(codes - have).max()) if codes.size else 0.0


# ---- 1. the plain surface, bit for bit ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cam", ["persp", "top", "oblique"])
def test_plain_surface_is_bit_exact(renderer, cam):
    g, cu, su, proj, unf = FM.view("case_plane", cam)
    FM.bind(renderer, g)
    m = MAPS["a"]
    p = SR.params(m)
    assert (p["W"], p["H"]) == (32, 24)
    sh = SR.lookup_f32(SR.centres_f32(su, g["pp"].tex, g["draws"]), p)[0]
    vis = unf["visible"] == 1
    lit, dark, between = SR.shares(sh[vis], p)
    print(f"{cam}: {int(vis.sum())} visible; fully lit {lit:.3f}, fully shadowed {dark:.3f}, between {between:.3f}")
    assert lit >= 0.2 and dark >= 0.2 and between >= 0.2
    base, tm0 = FM.varyings(renderer, cu, su, projection=proj, shadow=shadows.OFF)
    got, tm = FM.varyings(renderer, cu, su, projection=proj, shadow=m)
    assert got.shape == base.shape == sh.shape == (510,)
    assert np.array_equal(base["visible"] == 1, vis) and np.array_equal(got["visible"], base["visible"])
    assert tm["n_visible"] == tm0["n_visible"] == int(vis.sum()) and tm["n_pairs"] == tm0["n_pairs"]
    _same_fields(got, base, vis, GEOMETRY, cam)
    _same_fields(base, unf, vis, GEOMETRY + ("rgba",), cam)
    assert FM.bits_equal(got["rgba"][vis][:, 3].copy(), base["rgba"][vis][:, 3].copy())
    want = SR.shaded_rgb_f32(base["rgba"][vis][:, :3], sh[vis], p)
    assert FM.bits_equal(np.ascontiguousarray(got["rgba"][vis][:, :3]), want), cam             # every colour byte, no mask
    untouched = vis & (sh == 0)
    _same_fields(got, base, untouched, ("rgba",), cam)
    changed = (_codes(got["rgba"][vis & (sh > 0)])[0] != _codes(base["rgba"][vis & (sh > 0)])[0]).any(1).mean()
    assert changed > 0.8


# ---- 2. the surfaces ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["case_hmap", "case_sphere"])
def test_surfaces(renderer, name):
    g, cu, su, proj, unf = FM.view(name, "persp")
    FM.bind(renderer, g)
    cam = _block(cu)
    vis = unf["visible"] == 1
    pos, z = AR.unproject_f64(cam, unf["ndc"][vis], unf["depth"][vis])
    light = OR.ortho_camera_of(OR.surface_camera_args(name, "top"), 32, 24)
    m = shadows.from_ortho_camera(light, SR.two_region_map(32, 24), bias=0.0, strength=0.8, shade_color=(0.05, 0.1, 0.3))
    p = SR.params(m)
    assert set(np.unique(p["Z"])) == {0.0, 1.0}
    sh, _, _, (_, _, ld) = SR.lookup_f64([pos[:, 0], pos[:, 1], pos[:, 2]], p)
    tol_sh, tol_ld = SR.surface_tols(pos, SR.persp_delta(z, AR.near_of(cam)), p)
    masked = (np.abs(ld) <= tol_ld) | (np.abs(ld - 1.0) <= tol_ld)
    lit, dark, _ = SR.shares(sh, p)
    assert masked.mean() <= AR.MAX_MASKED and lit >= 0.2 and dark >= 0.2
    base, tm0 = FM.varyings(renderer, cu, su, projection=proj, shadow=shadows.OFF)
    got, tm = FM.varyings(renderer, cu, su, projection=proj, shadow=m)
    assert np.array_equal(base["visible"] == 1, vis) and np.array_equal(got["visible"], base["visible"])
    assert tm["n_visible"] == tm0["n_visible"] and tm["n_pairs"] == tm0["n_pairs"]
    _same_fields(got, base, vis, GEOMETRY, name)
    assert FM.bits_equal(got["rgba"][vis][:, 3].copy(), base["rgba"][vis][:, 3].copy())
    want = SR.shade_codes_f64(base["rgba"][vis][:, :3], sh, p)
    have, off = _codes(got["rgba"][vis])
    assert off < 1e-4                                                                # rgba[k] = (float)byte' / 255.0f
    err = np.abs(have - want).max(1)
    bound = 0.5 + 255.0 * tol_sh + SR.MARGIN
    print(f"{name}: {int(vis.sum())} visible, lit {lit:.3f}, shadowed {dark:.3f}, {int(masked.sum())} masked, largest tolerance {255.0 * tol_sh.max():.3f} codes, "
          f"max (|byte error| - 0.5) / (tolerance + margin) {np.max((err - 0.5)[~masked] / (bound - 0.5)[~masked]):.3f}")
    assert (err <= bound)[~masked].all(), name
    assert (have != _codes(base["rgba"][vis])[0]).any(1).mean() > 0.3


# ---- 3. known answers --------------------------------------------------------------------------------------------------------------------
BIAS = 0.03125
POINTS = [(2.5, 1.5, 0.0),           # 0: the centre of a lit texel
          (0.5, 1.5, 0.0),           # 1: deep inside the shadowing texels
          (2.0, 1.5, 0.0),           # 2: exactly midway between a shadowing and a lit texel
          (6.0, 1.5, 0.0),           # 3: outside the image
          (0.5, 1.5, -3.0),          # 4: ld = 1.25
          (0.5, 1.5, 3.0),           # 5: ld = -0.25
          (0.5, 1.5, 0.9375),        # 6: behind the texel's 0.25 by half the bias: lit
          (0.5, 1.5, 0.75),          # 7: behind it by twice the bias: shadowed
          (-0.25, 1.5, 0.0),         # 8: the image's edge, a quarter of the way into texel 0 from outside
          (0.5, 0.5, 0.0),           # 9, 10: for the 1 x 1 map: its centre, and a quarter texel to the right
          (0.75, 0.5, 0.0)]


def test_known_answers(renderer):
    """Opaque splats at positions exact in binary32 under tests/shadow_ref.py's unit light (texel (i, j) of a 4 x 4 map covers x in
    i .. i + 1, y in 3 - j .. 4 - j; depth 0.5 - z / 4), seen straight down.  The two left columns hold 0.25, the others 1.0."""
    # (longer along y than x: under this view an isotropic footprint has c01 = 0 and l1 = c00, a 0 / 0 direction in vs_main)
    halves = S.diag_halves((0.03, 0.06, 0.03))
    colours = [(200, 96 + 8 * k, 48, 255) for k in range(len(POINTS))]
    scene = S.raw_scene([(p, halves, c) for p, c in zip(POINTS, colours)])
    _, pd = scene.draws(map_index=7)
    renderer.configure(None)
    scene.upload(renderer)
    renderer.set_draws(pd)
    su = orc.scene_uniforms(num_lod=1)
    cu = ortho.top_down((2.0, 2.0), 3.0, 5.0, -5.0, W, Hh).uniforms()
    Z = np.ones((4, 4), F32)
    Z[:, :2] = 0.25
    m = SR.unit_light(Z, bias=BIAS, strength=0.5)
    base, tm0 = FM.varyings(renderer, cu, su, projection=ORTHO, shadow=shadows.OFF)
    n = len(POINTS)
    assert (base["visible"] == 1).all() and tm0["n_visible"] == n and (base["rgba"][:, 3] == 1.0).all()
    bb = _codes(base["rgba"])[0]
    assert np.array_equal(bb, np.array([c[:3] for c in colours], np.float64))
    got, tm = FM.varyings(renderer, cu, su, projection=ORTHO, shadow=m)
    assert tm["n_visible"] == n and tm["n_pairs"] == tm0["n_pairs"]
    _same_fields(got, base, np.ones(n, bool), GEOMETRY, "4 x 4")
    assert FM.bits_equal(got["rgba"][:, 3].copy(), base["rgba"][:, 3].copy())
    have, off = _codes(got["rgba"])
    assert off < 1e-4
    for k in (0, 3, 4, 5, 6):                                        # lit, outside, ld outside [0, 1], inside the bias: the record as it was
        assert FM.bits_equal(got["rgba"][k].copy(), base["rgba"][k].copy()), k
    strength = 0.5
    assert np.array_equal(have[1], np.rint(bb[1] * (1.0 - strength)))
    assert np.array_equal(have[7], np.rint(bb[7] * (1.0 - strength)))
    assert np.array_equal(have[2], np.rint(bb[2] * (1.0 - 0.5 * strength)))              # half of that
    assert np.array_equal(have[8], np.rint(bb[8] * (1.0 - 0.25 * strength)))             # three of its four texels' weight is lit
    assert (have[[1, 2, 7, 8]] < bb[[1, 2, 7, 8]]).all()
    # ... and all of them are the reference's
    p = SR.params(m)
    c = [np.array([q[k] for q in POINTS], F32) for k in range(3)]
    want = SR.shaded_rgb_f32(base["rgba"][:, :3], SR.lookup_f32(c, p)[0], p)
    assert FM.bits_equal(np.ascontiguousarray(got["rgba"][:, :3]), want)
    # a 1 x 1 map: x, y in 0 .. 1
    m1 = SR.unit_light(np.full((1, 1), 0.25, F32), bias=BIAS, strength=0.5)
    got, tm = FM.varyings(renderer, cu, su, projection=ORTHO, shadow=m1)
    have, _ = _codes(got["rgba"])
    assert tm["n_visible"] == n
    assert np.array_equal(have[9], np.rint(bb[9] * 0.5)) and np.array_equal(have[10], np.rint(bb[10] * (1.0 - 0.75 * strength)))
    p1 = SR.params(m1)
    want = SR.shaded_rgb_f32(base["rgba"][:, :3], SR.lookup_f32(c, p1)[0], p1)
    assert FM.bits_equal(np.ascontiguousarray(got["rgba"][:, :3]), want)
    for k in (0, 2, 3, 4, 5):                                        # outside the one texel's reach
        assert FM.bits_equal(got["rgba"][k].copy(), base["rgba"][k].copy()), k


# ---- 4. the loop closes ------------------------------------------------------------------------------------------------------------------
def test_the_lights_own_depth_frame_shadows_the_lower_splat(renderer):
    """Two opaque splats one above the other; the sun looks straight down.  Its depth frame, rendered by the library, is the map."""
    halves = S.diag_halves((0.3, 0.45, 0.3))
    scene = S.raw_scene([((2.0, 2.0, 1.0), halves, (200, 120, 48, 255)), ((2.0, 2.0, -1.0), halves, (200, 120, 48, 255))])
    _, pd = scene.draws(map_index=7)
    renderer.configure(None)
    scene.upload(renderer)
    renderer.set_draws(pd)
    su = orc.scene_uniforms(num_lod=1)
    sun = ortho.top_down((2.0, 2.0), 2.0, 3.0, -3.0, 64, 64)
    _, zmap = renderer.render(sun.uniforms(), su, 64, 64, projection=ORTHO, order_mode=L.GSWT_ORDER_DEPTH, depth=True)
    assert zmap.shape == (64, 64) and zmap.dtype == F32 and zmap.max() == 1.0
    d_up, d_low = (3.0 - 1.0) / 6.0, (3.0 + 1.0) / 6.0
    assert abs(float(zmap[31:33, 31:33].max()) - d_up) < 0.1 * (d_low - d_up)            # the upper splat is what the sun sees
    m = shadows.from_ortho_camera(sun, zmap, bias=0.02, strength=0.6, shade_color=(0.0, 0.0, 0.0))
    cu = ortho.top_down((2.0, 2.0), 3.0, 5.0, -5.0, W, Hh).uniforms()
    base, _ = FM.varyings(renderer, cu, su, projection=ORTHO, shadow=shadows.OFF)
    got, tm = FM.varyings(renderer, cu, su, projection=ORTHO, shadow=m)
    assert (base["visible"] == 1).all() and tm["n_visible"] == 2
    _same_fields(got, base, np.array([True, False]), GEOMETRY + ("rgba",), "upper")
    _same_fields(got, base, np.array([False, True]), GEOMETRY, "lower")
    assert np.array_equal(_codes(got["rgba"][1:])[0], np.rint(_codes(base["rgba"][1:])[0] * 0.4))     # all four texels shadow it
    assert got["rgba"][1, 3] == base["rgba"][1, 3]


# ---- 5. image, depth and pick over the GPU's own records ------------------------------------------------------------------------------------
@pytest.mark.parametrize("bg", [False, True], ids=["clear", "bg"])
@pytest.mark.parametrize("order_mode", [0, 1], ids=["reference", "depth"])
@pytest.mark.parametrize("cam", ["persp", "oblique"])
def test_image_depth_and_pick_match_the_references(renderer, cam, order_mode, bg):
    c = FM.image_case(renderer, cam, order_mode, bg, OR.SPLAT_SCALE, dict(antialias=0.0, shadow=MAPS["a"]), "shadow")
    on = c["again"](depth=True, pick=True)
    off = c["again"](depth=True, pick=True, shadow=shadows.OFF)
    assert FM.same(on[0], c["img"]) and not FM.same(on[0], off[0])
    assert FM.same(on[1], off[1]) and FM.same(on[2], off[2])                # depth and pick: the frame's without the map, byte for byte
    assert renderer.timings()["n_pairs"] == c["t"]["n_pairs"] > 0


# ---- 6. the same bits every way ------------------------------------------------------------------------------------------------------------
def _set_map(renderer, name):
    renderer.set_shadow_map(MAPS[name])


MODE = FM.Mode({name: (None, dict(shadow=m)) for name, m in MAPS.items()}, _set_map, on="a")


@pytest.fixture()
def plain(renderer):
    """The plane case bound under its perspective camera, depth order over a background, and the plain synchronous frames (colour,
    depth, pick) without a map and under each of the two maps."""
    g, cu, su, proj, _ = FM.view("case_plane", "persp")
    s = FM.plain_frames(renderer, MODE, g, su, cu)
    renderer.set_shadow_map(None)
    assert len({bytes(np.ascontiguousarray(f[0])) for f in s["frames"].values()}) == len(MAPS)
    assert s["pairs"]["a"] == s["pairs"]["b"] == s["pairs"]["off"]
    for name in ("a", "b"):
        assert FM.same(s["frames"][name][1], s["frames"]["off"][1]) and FM.same(s["frames"][name][2], s["frames"]["off"][2])
    return s


def test_graph_replay_with_alternating_maps(renderer, plain):
    seq1 = ["off", "a", "b", "a", "off", "b"]
    seq2 = ["a", "off", "b", "a", "off", "b"]
    launches, rebuilds, updates = FM.check_graph_replay(renderer, plain, MODE, seq1, seq2)
    assert rebuilds >= 2 and updates >= 1           # on / off selects another k_project: a rebuild; another map updates the node


def test_async_frames_in_flight_keep_their_map(renderer, plain):
    assert renderer.frame_slots() >= 4
    FM.check_in_flight(renderer, plain, MODE, ["a", "off", "b", "a"], waves=4, then="b")


def test_frames_in_flight_keep_their_map_when_its_source_is_overwritten(renderer, plain):
    """The image is copied inside the call: the caller overwrites its buffers and sets another map while the frames are in flight."""
    za, zb = MAPS["a"].depth.copy(), MAPS["b"].depth.copy()
    kw = {"a": dict(shadow=shadows.ShadowMap(MAPS["a"].world_to_light, za, MAPS["a"].bias, MAPS["a"].strength, MAPS["a"].shade_color)),
          "b": dict(shadow=shadows.ShadowMap(MAPS["b"].world_to_light, zb, MAPS["b"].bias, MAPS["b"].strength, MAPS["b"].shade_color)),
          "off": dict(shadow=shadows.OFF)}

    def then(_wave):
        za[:] = 0.0
        zb[:] = 0.0
        renderer.set_shadow_map(shadows.ShadowMap(MAPS["b"].world_to_light, zb, 0.0, 1.0, (1.0, 1.0, 1.0)))

    seq = ["a", "b", "off", "a"]
    got = FM.device_frames(renderer, plain, seq, waves=4, submit_kw=lambda name: (plain["cu"], kw[name]), then=then)
    FM.assert_frames(got, seq, plain, "source overwritten")


def test_a_device_image_is_the_host_image(renderer, plain):
    import torch
    zd = torch.from_numpy(MAPS["a"].depth).cuda()
    torch.cuda.synchronize()
    m = shadows.ShadowMap(MAPS["a"].world_to_light, zd, MAPS["a"].bias, MAPS["a"].strength, MAPS["a"].shade_color)
    assert m.on_device and (m.width, m.height) == (32, 24)
    got = renderer.render(plain["cu"], plain["su"], W, Hh, depth=True, pick=True, shadow=m, **plain["kw"])
    FM.assert_frames([got], ["a"], plain, "device image")


@pytest.mark.parametrize("opt", [L.GSWT_OPT_NO_CHUNK_CULL], ids=["no_chunk_cull"])
def test_compositor_and_cull_variants(renderer, plain, opt):
    FM.check_with_option_on(renderer, plain, MODE, opt, ["a", "b"])


def test_pair_buffer_overflow_rerun_keeps_the_map(renderer, plain):
    FM.check_overflow_rerun(renderer, plain, MODE, MODE.on, then="b")


def test_output_formats(renderer, plain):
    FM.check_output_formats(renderer, plain, MODE, [MODE.on])


@pytest.mark.parametrize("n", [2, 3])
def test_row_shards_tile_the_frame(renderer, plain, n):
    FM.check_row_shards(renderer, plain, MODE, n, [MODE.on])


@pytest.mark.parametrize("n", [2, 3, 5])
def test_column_bands_unite_to_the_frame(renderer, plain, n):
    FM.check_column_bands(renderer, plain, MODE, n, [MODE.on])


def _null_map(r):
    r.set_shadow_map(None)
    return {}


@pytest.mark.parametrize("cam", ["persp", "oblique"])
def test_off_is_untouched(cam):
    FM.check_off_is_untouched(cam, dict(shadow=MAPS["a"]), [("NULL", _null_map), ("OFF", lambda r: dict(shadow=shadows.OFF))])


def test_sequence_v2_is_refused_at_submit(renderer, plain):
    FM.check_v2_refused_at_submit(renderer, plain, MODE, ("a", "b"), (b"GSWT_OPT_STRICT_VS", b"gswt_set_shadow_map"))


# ---- 7. tint, then the shadow, then the fog --------------------------------------------------------------------------------------------------
def test_tint_then_shadow_then_fog(renderer):
    g, cu, su, proj, unf = FM.view("case_plane", "persp")
    FM.bind(renderer, g)
    tint = (0, 255, 64, 160)
    table = ST.TileStyle(tint[:3], tint[3]).pack() * 4096             # every map cell
    atm = A.Atmosphere(fog=(0.15, 2.0, 0.9, (0.62, 0.71, 0.80)))
    m = MAPS["a"]
    p = SR.params(m)
    vis = unf["visible"] == 1
    sh = SR.lookup_f32(SR.centres_f32(su, g["pp"].tex, g["draws"]), p)[0][vis]
    dist = AR.dist_f32(_block(cu).cam_pos, su, g["pp"].tex, g["draws"]).astype(np.float64)[vis]
    base, _ = FM.varyings(renderer, cu, su, projection=proj, shadow=shadows.OFF)
    rgb = base["rgba"][vis][:, :3]
    fog_p = AR.params(atm)
    runs = {"shadow + fog": (None, dict(atmosphere=atm), fog_p), "tint + shadow": (tint, dict(tile_styles=table), None),
            "tint + shadow + fog": (tint, dict(tile_styles=table, atmosphere=atm), fog_p)}
    seen = {}
    for label, (tn, kw, fp) in runs.items():
        renderer.set_tile_styles(None)
        renderer.set_atmosphere(A.OFF)
        got, tm = FM.varyings(renderer, cu, su, projection=proj, shadow=m, **kw)
        assert np.array_equal(got["visible"] == 1, vis) and tm["n_visible"] == int(vis.sum()), label
        _same_fields(got, base, vis, GEOMETRY, label)
        assert FM.bits_equal(got["rgba"][vis][:, 3].copy(), base["rgba"][vis][:, 3].copy()), label
        want, near_half = AR.fog_bytes(SR.chain_codes_f64(rgb, tn, sh, p, dist, fp))
        have, off = _codes(got["rgba"][vis])
        print(f"{label}: {int(near_half.sum())} channels inside the margin, {int((have != want).sum())} bytes off the float64 rint")
        assert off < 1e-4 and near_half.mean() <= AR.MAX_MASKED, label
        assert np.abs(have - want).max() <= 1.0, label
        assert np.array_equal(have[~near_half], want[~near_half]), label
        seen[label] = have
    # the order matters and shows: shadow before tint, or fog before shadow, would be other bytes
    wrong = np.rint(SR.chain_codes_f64(SR.chain_codes_f64(rgb, None, sh, p) / 255.0, tint, np.zeros_like(sh), p, dist, fog_p))
    assert (np.abs(seen["tint + shadow + fog"] - wrong).max(1) > 1.0).mean() > 0.2
    assert not np.array_equal(seen["tint + shadow + fog"], seen["shadow + fog"])


# ---- 8. refusals ---------------------------------------------------------------------------------------------------------------------------
def _raw_params(m=None, **kw):
    f = dict(bias=0.002, strength=0.75, r=SHADE[0], g=SHADE[1], b=SHADE[2], pad=(0, 0, 0))
    f.update(kw)
    M = [float(x) for x in (MAPS["a"].world_to_light if m is None else m)]
    return (C.c_char * 96).from_buffer_copy(struct.pack("<16f2f3f3I", *M, f["bias"], f["strength"], f["r"], f["g"], f["b"], *f["pad"]))


def test_refused_maps_leave_the_map_in_force(renderer, plain):
    lib, h = renderer._lib, renderer._h
    nan, inf = float("nan"), float("inf")
    Z = np.ascontiguousarray(MAPS["a"].depth)
    zp = Z.ctypes.data_as(C.c_void_p)
    assert lib.gswt_set_shadow_map(h, _raw_params(), zp, 32, 24, 0) == L.GSWT_OK          # = MAPS["a"]
    M = MAPS["a"].world_to_light

    def mat(k, v):
        out = M.copy()
        out[k] = v
        return out

    bad = [("world_to_light[5]", dict(m=mat(5, nan))), ("world_to_light[12]", dict(m=mat(12, inf))), ("world_to_light[0]", dict(m=mat(0, -inf))),
           ("bottom row", dict(m=mat(3, 0.5))), ("bottom row", dict(m=mat(7, -1.0))), ("bottom row", dict(m=mat(11, 1e-30))), ("bottom row", dict(m=mat(15, 2.0))),
           ("bias", dict(bias=-0.001)), ("bias", dict(bias=nan)), ("bias", dict(bias=inf)),
           ("strength", dict(strength=0.0)), ("strength", dict(strength=-0.5)), ("strength", dict(strength=1.5)), ("strength", dict(strength=nan)),
           ("shade_color[0]", dict(r=1.5)), ("shade_color[1]", dict(g=-0.1)), ("shade_color[2]", dict(b=nan)), ("shade_color[2]", dict(b=inf)),
           ("_pad", dict(pad=(1, 0, 0))), ("_pad", dict(pad=(0, 0, 7)))]
    for field, kw in bad:
        assert lib.gswt_set_shadow_map(h, _raw_params(**kw), zp, 32, 24, 0) == L.GSWT_ERR_BAD_ARG, (field, kw)
        assert field.encode() in lib.gswt_last_error(h), (field, kw, lib.gswt_last_error(h))
    for field, (w, hh) in (("width", (0, 24)), ("width", (4097, 24)), ("width", (-3, 24)), ("height", (32, 0)), ("height", (32, 4097))):
        assert lib.gswt_set_shadow_map(h, _raw_params(), zp, w, hh, 0) == L.GSWT_ERR_BAD_ARG, (field, w, hh)
        assert field.encode() in lib.gswt_last_error(h), (field, lib.gswt_last_error(h))
    with pytest.raises(GSWTError):
        m = shadows.ShadowMap(M, Z)
        m.strength = 2.0                                             # (past the Python layer's own check)
        renderer.set_shadow_map(m)
    got = renderer.render(plain["cu"], plain["su"], W, Hh, depth=True, pick=True, **plain["kw"])
    FM.assert_frames([got], ["a"], plain, "after refused maps")
    # the edges of the ranges are accepted; NULL params or a NULL image switch shadows off
    for kw in (dict(bias=0.0), dict(strength=1.0), dict(r=0.0, g=1.0, b=1.0), dict(strength=1e-30)):
        assert lib.gswt_set_shadow_map(h, _raw_params(**kw), zp, 32, 24, 0) == L.GSWT_OK, kw
    one = np.ones(4096, F32)
    assert lib.gswt_set_shadow_map(h, _raw_params(), one.ctypes.data_as(C.c_void_p), 4096, 1, 0) == L.GSWT_OK
    assert lib.gswt_set_shadow_map(h, _raw_params(), one.ctypes.data_as(C.c_void_p), 1, 4096, 0) == L.GSWT_OK
    for args in ((None, zp), (_raw_params(), None)):
        assert lib.gswt_set_shadow_map(h, _raw_params(), zp, 32, 24, 0) == L.GSWT_OK
        assert lib.gswt_set_shadow_map(h, args[0], args[1], 32, 24, 0) == L.GSWT_OK
        got = renderer.render(plain["cu"], plain["su"], W, Hh, depth=True, pick=True, **plain["kw"])
        FM.assert_frames([got], ["off"], plain, "after NULL")


# ---- 9. the proxy passes -------------------------------------------------------------------------------------------------------------------
PROXY_SHADE = dict(bias=0.0, strength=0.8, shade_color=(0.05, 0.1, 0.3))


def _proxy(renderer, us, Wp, Hp, grid_dim, hm, mips, shadow, projection=PERSP, atm=A.OFF):
    import torch
    renderer.configure(hm)
    renderer.proxy_configure(mips, grid_dim=grid_dim)
    renderer.set_shadow_map(shadow)
    renderer.set_atmosphere(atm)
    rgba = torch.from_numpy(R.sky(Wp, Hp)).cuda()
    depth = torch.zeros((Hp, Wp), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    for k, u in enumerate(us):
        renderer.proxy_render(u, Wp, Hp, rgba.data_ptr(), depth.data_ptr(), clear_depth=(k == 0), projection=projection)
    renderer.synchronize()
    return depth.cpu().numpy(), rgba.cpu().numpy()


def _proxy_points_and_map(d0, cam_block, Wp, Hp):
    """(written pixels, their float64 unprojection pos and view depth z, a two-region map of a top-down light over the middle of what
    the pass drew) of the plain pass's depth image d0."""
    written = d0 < 1.0
    assert written.mean() > 0.05
    ys, xs = np.nonzero(written)
    ndc = np.stack([(xs + 0.5) / Wp * 2.0 - 1.0, 1.0 - (ys + 0.5) / Hp * 2.0], 1)
    pos, z = AR.unproject_f64(cam_block, ndc, d0[written])
    lo, hi = np.percentile(pos, 10, axis=0), np.percentile(pos, 90, axis=0)
    light = ortho.top_down(((lo[0] + hi[0]) / 2, (lo[1] + hi[1]) / 2), max(hi[1] - lo[1], (hi[0] - lo[0]) * 24 / 32) / 2,
                           float(pos[:, 2].max()) + 5.0, float(pos[:, 2].min()) - 5.0, 32, 24)
    return written, pos, z, shadows.from_ortho_camera(light, SR.two_region_map(32, 24), **PROXY_SHADE)


def _proxy_case(renderer, name, us, cam_block, grid_dim, hm, mips, projection, delta_of):
    """The pass without a map, then with a two-region map of a top-down light over the middle of what the pass drew: depth and unwritten
    pixels byte for byte, shaded pixels against the float64 lookup at the float64 unprojection of the proxy's own depth."""
    Wp, Hp = R.W0, R.H0
    d0, c0 = _proxy(renderer, us, Wp, Hp, grid_dim, hm, mips, shadows.OFF, projection)
    written, pos, z, m = _proxy_points_and_map(d0, cam_block, Wp, Hp)
    p = SR.params(m)
    d1, c1 = _proxy(renderer, us, Wp, Hp, grid_dim, hm, mips, m, projection)
    sky = R.sky(Wp, Hp)
    assert FM.same(d0, d1) and FM.same(c1[~written], sky[~written]) and FM.same(c0[~written], sky[~written])
    if name == "black_background":
        assert FM.same(c0, c1) and (c0[written] == np.array([0, 0, 0, 1], F32)).all()
        return
    sh, _, outside, (_, _, ld) = SR.lookup_f64([pos[:, 0], pos[:, 1], pos[:, 2]], p)
    tol_sh, tol_ld = SR.surface_tols(pos, delta_of(pos, z), p)
    assert not ((np.abs(ld) <= tol_ld) | (np.abs(ld - 1.0) <= tol_ld)).any()
    want = c0[written][:, :3].astype(np.float64) * (1.0 - sh[:, None]) + p["shade"].astype(np.float64)[None] * sh[:, None]
    err = np.abs(c1[written][:, :3].astype(np.float64) - want).max(1)
    tol = 2e-6 + tol_sh
    lit, dark, between = SR.shares(sh, p)
    print(f"{name}: {int(written.sum())} proxy pixels, lit {lit:.3f} shadowed {dark:.3f} between {between:.3f}, outside the image {outside.mean():.3f}, "
          f"max |colour error| / tolerance {np.max(err / tol):.3f}, largest tolerance {tol.max():.2e}")
    assert (err <= tol).all()
    assert (c1[written][:, 3] == 1.0).all()
    assert lit > 0.1 and dark > 0.1 and not FM.same(c0, c1)
    assert FM.same(c1[written][sh == 0], c0[written][sh == 0])


def _persp_scene(name):
    """What _proxy_case takes of the perspective scene `name` (tests/proxy_raster_ref.py) behind the test's own name."""
    cam_kw, draws, grid_dim, _ = R.SCENES[name]
    cam = R.scene_camera(cam_kw, R.W0, R.H0)
    cu = cam.uniforms()
    near = AR.near_of(cu)
    # (the kernel's own hit point o + t d, rounded at the world coordinates' magnitude, on top of the depth's share)
    return (R.scene_uniforms(cam, draws), cu, grid_dim, R.height_map(), R.mip_chain(), PERSP,
            lambda pos, z: SR.persp_delta(z, near) + 8.0 * SR.U * np.abs(pos).max(1))


def _ortho_scene(name):
    spec, draws, grid_dim, hm_n, _ = O.SCENES[name]
    cam = O.make_camera(spec, R.W0, R.H0)
    span = 2.0 / abs(float(cam.projection[10]))                      # far - near: the depth image's binary32 rounding times it, along the rays
    return (O.scene_uniforms(cam, draws), cam.uniforms(), grid_dim, R.height_map(n=hm_n), R.mip_chain(), ORTHO,
            lambda pos, z: AR.DEPTH_ROUNDINGS * SR.U * (span + np.abs(pos).max(1)))


@pytest.mark.parametrize("name", ["oblique", "flat_two_draws", "clip_two_draws", "black_background"])
def test_proxy_is_shaded(renderer, name):
    _proxy_case(renderer, name, *_persp_scene(name))


def test_orthographic_proxy_is_shaded(renderer):
    _proxy_case(renderer, "isometric (orthographic)", *_ortho_scene("isometric"))


# k_proxy<FOG = true, ., SHD = true>: the shadow, then the fog (the fogs of the two passes' own fog tests)
PROXY_FOGS = {"oblique": (_persp_scene, (0.15, 2.0, 0.9, (0.62, 0.71, 0.80))), "isometric": (_ortho_scene, (0.03, 5.0, 0.9, (0.6, 0.7, 0.8)))}


@pytest.mark.parametrize("name", list(PROXY_FOGS))
def test_proxy_is_shaded_then_fogged(renderer, name):
    """Both on: depth and unwritten pixels are the plain pass's byte for byte; a written pixel is (c0 (1 - sh) + shade sh) (1 - F) + fog F
    in float64, c0 the plain pass's own pixel, sh and F at the float64 unprojection of the proxy's depth.  The tolerance is the shaded
    pass's 2e-6 + tol_sh plus a fog term built the same way: |dc / dF| <= 1, |dF / d dist| <= fog_max density and the hit point is off by
    at most the same delta, so fog_max density delta."""
    scene, fog = PROXY_FOGS[name]
    us, cam_block, grid_dim, hm, mips, projection, delta_of = scene(name)
    Wp, Hp = R.W0, R.H0
    atm = A.Atmosphere(fog=fog)
    fp = AR.params(atm)
    d0, c0 = _proxy(renderer, us, Wp, Hp, grid_dim, hm, mips, shadows.OFF, projection)
    written, pos, z, m = _proxy_points_and_map(d0, cam_block, Wp, Hp)
    p = SR.params(m)
    d1, c1 = _proxy(renderer, us, Wp, Hp, grid_dim, hm, mips, m, projection, atm)
    sky = R.sky(Wp, Hp)
    assert FM.same(d0, d1) and FM.same(c1[~written], sky[~written]) and FM.same(c0[~written], sky[~written])
    sh, _, _, (_, _, ld) = SR.lookup_f64([pos[:, 0], pos[:, 1], pos[:, 2]], p)
    delta = delta_of(pos, z)
    tol_sh, tol_ld = SR.surface_tols(pos, delta, p)
    assert not ((np.abs(ld) <= tol_ld) | (np.abs(ld - 1.0) <= tol_ld)).any()
    cp = np.array([float(_block(cam_block).cam_pos[k]) for k in range(3)])
    F = AR.fog_amount_f64(np.sqrt(((pos - cp) ** 2).sum(1)), fp)[:, None]
    base = c0[written][:, :3].astype(np.float64)
    shade, fogc, s = p["shade"].astype(np.float64)[None], fp["fog_color"].astype(np.float64)[None], sh[:, None]
    want = (base * (1.0 - s) + shade * s) * (1.0 - F) + fogc * F
    have = c1[written][:, :3].astype(np.float64)
    err = np.abs(have - want).max(1)
    tol = 2e-6 + tol_sh + float(fp["fog_max"]) * float(fp["fog_density"]) * delta
    lit, dark, between = SR.shares(sh, p)
    print(f"{name}: {int(written.sum())} proxy pixels, lit {lit:.3f} shadowed {dark:.3f} between {between:.3f}, F {F.min():.3f} .. {F.max():.3f}, "
          f"max |colour error| / tolerance {np.max(err / tol):.3f}, largest tolerance {tol.max():.2e}")
    assert (err <= tol).all()
    assert (c1[written][:, 3] == 1.0).all()
    assert lit > 0.1 and dark > 0.1 and F.max() > 0.1
    # the order shows: the shadow behind the fog would be another colour on a good share of the shaded pixels
    wrong = (base * (1.0 - F) + fogc * F) * (1.0 - s) + shade * s
    shaded = sh > 0
    other = (np.abs(wrong - want).max(1) > tol)[shaded].mean()
    print(f"{name}: the shadow behind the fog differs beyond the tolerance on {other:.3f} of the {int(shaded.sum())} shaded pixels")
    assert other >= 0.1


# ---- 10. through the frame harness ---------------------------------------------------------------------------------------------------------
def test_pipeline_passes_shadow_through(renderer):
    from gswt_renderer_amd import host, synth
    from gswt_renderer_amd.pipeline import GSWTPipeline
    cfg = dict(tile_map_half_wh=(3, 3), surface_type=0, lod_max_dist=20.0, tile_sort_type=3, merge_type=2)
    pipe = GSWTPipeline(synth.make_tileset(n_lod=3, n_tile=16, lod0_count=800), host.user_data(**cfg), renderer=renderer)
    pos = (4.2, 1.0, 2.0)
    cu, vp = host.camera_uniforms(pos, (5.0, 3.0, 1.5), (0, 0, 1), 45.0, 0.1, 2400.0, W, Hh)
    pipe.update(pos, vp)
    off = pipe.render(cu, W, Hh)
    pairs_off = renderer.timings()["n_pairs"]
    m = shadows.from_ortho_camera(ortho.top_down((5.0, 4.0), 8.0, 6.0, -6.0, 17, 11), SR.two_region_map(17, 11), strength=0.7, shade_color=SHADE)
    on = pipe.render(cu, W, Hh, shadow=m)
    assert renderer.timings()["n_pairs"] == pairs_off > 0 and not FM.same(on, off)
    renderer.set_shadow_map(None)
    assert FM.same(renderer.render(cu, pipe.wang.scene_uniforms(), W, Hh, shadow=m), on)
    assert FM.same(pipe.render(cu, W, Hh), on)                   # (no argument: the context keeps the map)
    assert FM.same(pipe.render(cu, W, Hh, shadow=shadows.OFF), off)
