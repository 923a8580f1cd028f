"""gswt_proxy_render_ortho (k_proxy<., ORTHO>) against tests/proxy_ortho_ref.py, the float64 rasterisation of the proxy mesh under an affine
projection: the scenes and conditions of tests/test_proxy_ortho_cpu.py with the kernel in front of them.

Off the rounding bands coverage must be equal, depth within DEPTH_FACTOR (2) x the error of an f32 rasteriser emulation + 1e-6 -- for every
scene: orthographic depth is position / (far - near), so a fixed 1e-6 means nothing at a range of 1.2 -- and colour within 1e-4 (far from
the origin plus what the f32 rounding of uv ~ 1e4 allows).  Then: pixel centres exactly on lattice lines and vertices, the eye slid along
the view axis, fog, a depth-only ground on a fresh context, the perspective pass untouched, and the refusals."""
import ctypes as C

import numpy as np
import pytest

from gswt_renderer_amd import _lib as L
from gswt_renderer_amd import atmosphere as A
from gswt_renderer_amd import ortho
from tests import frame_modes as FM
from tests import proxy_ortho_ref as O
from tests import proxy_raster_ref as R

pytestmark = pytest.mark.gpu
W, H = O.W0, O.H0
FOG = A.Atmosphere(fog=(0.03, 5.0, 0.9, (0.6, 0.7, 0.8)))
FOG_POS = (5.0, 3.0, 2.0)
REVERSED_FACTOR = 9.84       # test_depth_falling_along_the_view_axis: its measured ratio 6.56 x 1.5


@pytest.fixture(autouse=True)
def _defaults(renderer):
    """Every test leaves the shared context as it found it."""
    yield
    renderer.set_option(L.GSWT_OPT_PROJECTION, L.GSWT_PROJECTION_PERSPECTIVE)
    renderer.set_atmosphere(A.OFF)
    renderer.configure(None)


def _draw(r, us, Wp, Hp, grid_dim, hm, mips, fog=A.OFF, projection=1):
    import torch
    r.configure(hm)
    if mips is not None:
        r.proxy_configure(mips, grid_dim=grid_dim)
    r.set_atmosphere(fog)
    rgba = torch.from_numpy(R.sky(Wp, Hp)).cuda()
    depth = torch.zeros((Hp, Wp), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    for k, u in enumerate(us):
        r.proxy_render(u, Wp, Hp, rgba.data_ptr(), depth.data_ptr(), clear_depth=(k == 0), projection=projection)
    r.synchronize()
    return depth.cpu().numpy(), rgba.cpu().numpy()


def _check(name, got_d, got_c, us, opt, ref, label=None, factor=O.DEPTH_FACTOR):
    ref_d, ref_c, amb, res, ctol = ref
    tol, emu = O.depth_tol(us, W, H, res, amb, factor)
    both = (got_d < 1.0) & (ref_d < 1.0) & ~amb
    err = np.where(both, np.abs(got_d.astype(np.float64) - ref_d), 0.0)
    derr = float(err.max())
    wy, wx = np.unravel_index(int(err.argmax()), err.shape)
    cerr = float((np.abs(got_c.astype(np.float64) - ref_c).max(-1) - (ctol if opt.get("colour") == "ulp" else 0.0))[~amb].max())
    print(f"{label or name}: coverage {(ref_d < 1.0).mean():.3f} bands {amb.mean():.3%} depth error {derr:.3e} = {derr / max(emu, 1e-30):.2f} x the f32 "
          f"emulation's {emu:.3e} (bound {tol:.3e}) at pixel ({wy}, {wx}), |cos| of the incidence there {O.incidence(us, res, wy, wx):.4f}; "
          f"colour error beyond the uv allowance {cerr:.3e}")
    assert (ref_d < 1.0).mean() > 0.05
    R.compare(got_d, got_c, ref_d, ref_c, amb, depth_tol=tol, colour=opt.get("colour", True), max_amb=opt.get("max_amb", 0.02), ulp_tol=ctol)
    return tol


@pytest.mark.parametrize("name", sorted(O.SCENES))
def test_kernel_matches_rasterised_mesh(renderer, name):
    us, grid_dim, hm, mips, opt, ref = O.scene_reference(name)
    got_d, got_c = _draw(renderer, us, W, H, grid_dim, hm, mips)
    _check(name, got_d, got_c, us, opt, ref)
    if name == "black_background":
        wr = got_d < 1.0
        assert (got_c[wr] == np.array([0.0, 0.0, 0.0, 1.0], np.float32)).all() and FM.same(got_c[~wr], R.sky(W, H)[~wr])
    if name == "top_down":          # wider than the map: the pixels off the footprint keep the incoming colour and depth 1
        off = ref[0] == 1.0
        assert 0.1 < off.mean() < 0.15 and (got_d[off] == 1.0).all() and FM.same(got_c[off], R.sky(W, H)[off])


def test_pixel_centres_on_lattice_lines_and_vertices(renderer):
    """256 x 128 at 4 px per world unit, every quantity dyadic: pixel column 16 k + 15 lies exactly on the lattice line x = 4 k - 24 and row
    16 m on y = 20 - 4 m, and the view lies inside the footprint.  Every pixel is written, none is exempt from the depth bound (depth is
    continuous across edges: only coverage could crack there), and at the lattice vertices the height field equals the vertex's height."""
    Wl, Hl = 256, 128
    cam = ortho.top_down((4.125, 4.125), 16.0, 10.0, -10.0, Wl, Hl)
    assert np.array_equal(cam.view, ortho.OrthoCamera(Wl, Hl, (4.125, 4.125, 10.0), (4.125, 4.125, 9.0), (0, 1, 0), 16.0, 0.0, 20.0).view)
    us = O.scene_uniforms(cam, [R._map()])
    hm, mips = R.height_map(), R.mip_chain()
    got_d, got_c = _draw(renderer, us, Wl, Hl, 24, hm, mips)
    ref_d, ref_c, amb, res, ctol = O.reference(us, Wl, Hl, grid_dim=24, hm=hm, mips=mips)
    none = np.zeros_like(amb)
    tol, emu = O.depth_tol(us, Wl, Hl, res, none)
    derr = float(np.abs(got_d.astype(np.float64) - ref_d).max())
    print(f"lattice: written {(got_d < 1.0).mean():.4f}, depth error {derr:.3e} = {derr / emu:.2f} x the f32 emulation's {emu:.3e} (bound {tol:.3e}), bands {amb.mean():.3%}")
    assert (ref_d < 1.0).all() and (got_d < 1.0).all()
    assert derr <= tol
    cerr = np.abs(got_c.astype(np.float64) - ref_c).max(-1)
    assert (cerr[~amb] <= 1e-4).all() and amb.mean() > 0.05          # (the lattice lines are all band: that is the point)
    X, Y, Z, _ = R.lattice(us[0], 24, hm)
    ks, ms = np.arange(Wl // 16), np.arange(Hl // 16)
    xs, ys = 16 * ks + 15, 16 * ms
    assert np.array_equal(X[ks + 4], (4.0 * ks - 24.0).astype(np.float32)) and np.array_equal(Y[15 - ms], (20.0 - 4.0 * ms).astype(np.float32))
    want = Z[np.ix_(ks + 4, 15 - ms)].astype(np.float64).T           # [row, column]
    got = ortho.height_from_depth(cam, got_d[np.ix_(ys, xs)])
    herr = float(np.abs(got - want).max())
    print(f"lattice vertices: {want.size} heights in {want.min():.2f} .. {want.max():.2f}, error {herr:.3e} (bound {20.0 * tol:.3e})")
    assert want.max() - want.min() > 1.0 and herr <= 20.0 * tol


def test_eye_slid_along_the_view_axis(renderer):
    """isometric again from 80 units further along the view direction -- the eye inside the terrain, the near plane 79 units behind it:
    the same planes, so the same frame."""
    spec, draws, grid_dim, hm_n, opt = O.SCENES["isometric"]
    us, _, hm, mips, _, ref = O.scene_reference("isometric")
    _, eye, target, up, hh, near, far = spec
    f = np.subtract(target, eye) / np.linalg.norm(np.subtract(target, eye))
    cam = ortho.OrthoCamera(W, H, np.add(eye, 80.0 * f), np.add(target, 80.0 * f), up, hh, near - 80.0, far - 80.0)
    assert cam.near == -79.0 and cam.far == 80.0
    us2 = O.scene_uniforms(cam, draws)
    d1, c1 = _draw(renderer, us, W, H, grid_dim, hm, mips)
    d2, c2 = _draw(renderer, us2, W, H, grid_dim, hm, mips)
    ref_d, _, amb, res, _ = ref
    tol, emu = O.depth_tol(us, W, H, res, amb)
    bad = ((d1 < 1.0) != (d2 < 1.0)) & ~amb
    both = (d1 < 1.0) & (d2 < 1.0) & ~amb
    derr = float(np.abs(d1.astype(np.float64) - d2)[both].max())
    print(f"eye slid: depth differs by {derr:.3e} (bound {tol:.3e}), coverage differs at {int(bad.sum())} pixels off the bands")
    assert not bad.any() and both.mean() > 0.4 and derr <= tol
    _check("isometric", d2, c2, us, opt, ref, label="eye slid against the reference of the original")


def test_depth_falling_along_the_view_axis(renderer):
    """grazing with p[10] and p[14] negated: depth' = 1 - depth, a legal affine matrix (ortho() with near and far swapped).  The nearest
    fragment in depth is now the LAST one along the view axis -- a ray this flat crosses the hills more than once -- so the rays have to run
    the other way.

    The one scene with a depth factor of its own ("The orthographic proxy pass"): measured 2.392e-06 against the f32 emulation's
    3.647e-07, ratio 6.56, so the factor is 6.56 x 1.5 = 9.84 in place of 2.  The worst pixel shows a back face at 0.42 degrees to the view
    axis (|cos| of the incidence 0.0073): a lateral move of the sample point by 2.4e-6 world units -- less than one binary32 ulp of the ray
    origin's coordinates, ~40 -- moves the depth that far.  The emulation rounds three vertices once and interpolates in float64; a per-pixel
    binary32 ray cannot place its origin more finely than that ulp."""
    spec, draws, grid_dim, hm_n, opt = O.SCENES["grazing"]
    us = O.scene_uniforms(O.make_camera(spec, W, H), draws)
    for k in (10, 14):
        us[0].projection[k] = -us[0].projection[k]
    hm, mips = R.height_map(n=hm_n), R.mip_chain()
    ref = O.reference(us, W, H, grid_dim=grid_dim, hm=hm, mips=mips)
    fwd, cov = O.scene_reference("grazing")[5], ref[0] < 1.0
    assert np.array_equal(cov, fwd[0] < 1.0) and (np.abs((1.0 - ref[0]) - fwd[0])[cov] > 0.01).mean() > 0.25       # another surface at a quarter of them
    got_d, got_c = _draw(renderer, us, W, H, grid_dim, hm, mips)
    _check("grazing, depth reversed", got_d, got_c, us, opt, ref, factor=REVERSED_FACTOR)


@pytest.mark.parametrize("name", ["isometric", "top_down"])
def test_fog(renderer, name):
    us0, grid_dim, hm, mips, opt, ref0 = O.scene_reference(name, lod_pos=FOG_POS)
    us, _, _, _, _, ref = O.scene_reference(name, fog=FOG, lod_pos=FOG_POS)
    assert tuple(us[0].cam_pos)[:3] == FOG_POS and bytes(us[0]) == bytes(us0[0])
    d0, c0 = _draw(renderer, us, W, H, grid_dim, hm, mips)
    d1, c1 = _draw(renderer, us, W, H, grid_dim, hm, mips, fog=FOG)
    wr = d0 < 1.0
    assert FM.same(d0, d1) and FM.same(c0[~wr], c1[~wr]) and not FM.same(c0[wr], c1[wr])
    moved = np.abs(ref[1] - ref0[1]).max(-1)[wr]
    assert moved.max() > 0.1                                           # the fog is not a detail of this frame
    _check(name, d0, c0, us, opt, ref0, label=name + " unfogged")
    _check(name, d1, c1, us, opt, ref, label=name + " fogged")


def test_depth_only_ground_on_a_fresh_context():
    """black_background before any gswt_proxy_configure: the height-field / shadow-map use needs no texture."""
    from gswt_renderer_amd.renderer import GSWTError, GSWTRenderer
    us, grid_dim, hm, mips, opt, ref = O.scene_reference("black_background")
    r = GSWTRenderer(0)
    try:
        got_d, got_c = _draw(r, us, W, H, grid_dim, hm, None)
        _check("black_background", got_d, got_c, us, opt, ref, label="fresh context, depth only")
        assert (got_c[got_d < 1.0] == np.array([0.0, 0.0, 0.0, 1.0], np.float32)).all()
        textured, _, _, _, _, _ = O.scene_reference("isometric")
        with pytest.raises(GSWTError) as e:
            _draw(r, textured, W, H, grid_dim, hm, None)
        assert e.value.code == L.GSWT_ERR_STATE
    finally:
        r.close()


def test_perspective_pass_untouched(renderer):
    """One gswt_proxy_render frame (proxy_raster_ref's `oblique`) is the same bits before and after a gswt_proxy_render_ortho call on the
    context, and with GSWT_OPT_PROJECTION at 1 and at 0."""
    cam_kw, draws, grid_dim, _ = R.SCENES["oblique"]
    us = R.scene_uniforms(R.scene_camera(cam_kw, W, H), draws)
    hm, mips = R.height_map(), R.mip_chain()
    before = _draw(renderer, us, W, H, grid_dim, hm, mips, projection=0)
    assert (before[0] < 1.0).mean() > 0.3
    ous, _, _, _, _, _ = O.scene_reference("isometric")
    _draw(renderer, ous, W, H, grid_dim, hm, mips)
    after = _draw(renderer, us, W, H, grid_dim, hm, mips, projection=0)
    renderer.set_option(L.GSWT_OPT_PROJECTION, L.GSWT_PROJECTION_ORTHO)
    with_opt = _draw(renderer, us, W, H, grid_dim, hm, mips, projection=0)
    renderer.set_option(L.GSWT_OPT_PROJECTION, L.GSWT_PROJECTION_PERSPECTIVE)
    without = _draw(renderer, us, W, H, grid_dim, hm, mips, projection=0)
    for other in (after, with_opt, without):
        assert FM.same(before[0], other[0]) and FM.same(before[1], other[1])
    # ... and the orthographic pass does not read the option either
    a = _draw(renderer, ous, W, H, grid_dim, hm, mips)
    renderer.set_option(L.GSWT_OPT_PROJECTION, L.GSWT_PROJECTION_ORTHO)
    b = _draw(renderer, ous, W, H, grid_dim, hm, mips)
    assert FM.same(a[0], b[0]) and FM.same(a[1], b[1])


def test_refusals(renderer):
    import torch
    lib, h = renderer._lib, renderer._h
    us, grid_dim, hm, mips, opt, ref = O.scene_reference("isometric")
    good = _draw(renderer, us, W, H, grid_dim, hm, mips)
    rgba = torch.from_numpy(R.sky(W, H)).cuda()
    depth = torch.full((H, W), 0.25, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()

    def block(edit=None, base=None):
        u = L.ProxyUniforms.from_buffer_copy(bytes(base if base is not None else us[0]))
        if edit:
            edit(u)
        return (C.c_char * 224).from_buffer_copy(bytes(u))

    def proj(k, v):
        def f(u):
            u.projection[k] = v
        return f

    def field(name, v):
        def f(u):
            setattr(u, name, v)
        return f

    nan, inf = float("nan"), float("inf")
    persp = R.scene_uniforms(R.scene_camera(R.SCENES["oblique"][0], W, H), R.SCENES["oblique"][1])[0]
    rp, dp = C.c_void_p(rgba.data_ptr()), C.c_void_p(depth.data_ptr())
    cases = [("null block", None, rp, dp, W, H, b"bad argument"), ("null colour", block(), None, dp, W, H, b"bad argument"),
             ("null depth", block(), rp, None, W, H, b"bad argument"), ("width 0", block(), rp, dp, 0, H, b"bad argument"),
             ("height -1", block(), rp, dp, W, -1, b"bad argument"),
             ("tile_width 0", block(field("tile_width", 0.0)), rp, dp, W, H, b"tile_width"),
             ("tile_width nan", block(field("tile_width", nan)), rp, dp, W, H, b"tile_width"),
             ("width_scale 0, full grid", block(lambda u: (setattr(u, "map_proxy", 0), setattr(u, "width_scale", 0.0))), rp, dp, W, H, b"width_scale"),
             ("perspective matrix", block(base=persp), rp, dp, W, H, b"projection")]
    cases += [(f"bottom row p[{k}] = {v}", block(proj(k, v)), rp, dp, W, H, b"bottom row") for k, v in ((3, 1e-9), (7, -1.0), (11, nan), (15, 0.5), (15, nan))]
    cases += [(f"shear p[{k}]", block(proj(k, 1e-9)), rp, dp, W, H, b"projection[%d]" % k) for k in (1, 2, 4, 6, 8, 9)]
    cases += [(f"p[{k}] = {v}", block(proj(k, v)), rp, dp, W, H, b"projection[%d]" % k) for k in (0, 5, 10) for v in (0.0, -0.0, nan, inf)]
    cases += [(f"p[{k}] = {v}", block(proj(k, v)), rp, dp, W, H, b"projection[%d]" % k) for k in (12, 13, 14) for v in (nan, inf, -inf)]
    cases += [("singular view", block(lambda u: [u.view.__setitem__(i, 0.0) for i in (0, 1, 2)]), rp, dp, W, H, b"view")]
    for what, u, r_, d_, w_, h_, word in cases:
        assert lib.gswt_proxy_render_ortho(h, u, w_, h_, r_, d_, 1) == L.GSWT_ERR_BAD_ARG, what
        assert word in lib.gswt_last_error(h) and b"gswt_proxy_render_ortho" in lib.gswt_last_error(h), (what, lib.gswt_last_error(h))
    renderer.synchronize()
    torch.cuda.synchronize()
    assert bool((depth == 0.25).all()) and FM.same(rgba.cpu().numpy(), R.sky(W, H))          # nothing enqueued, clear_depth not performed
    # a HeightMap surface without a height map is a state error, as in the perspective call
    renderer.configure(None)
    assert lib.gswt_proxy_render_ortho(h, block(), W, H, rp, dp, 1) == L.GSWT_ERR_STATE
    assert lib.gswt_proxy_render(h, block(base=persp), W, H, rp, dp, 1) == L.GSWT_ERR_STATE
    renderer.synchronize()
    assert bool((depth == 0.25).all())
    # the next valid call works
    again = _draw(renderer, us, W, H, grid_dim, hm, mips)
    assert FM.same(good[0], again[0]) and FM.same(good[1], again[1])
    with pytest.raises(ValueError):
        renderer.proxy_render(us[0], W, H, rgba.data_ptr(), depth.data_ptr(), True, projection=2)
