"""gswt_proxy_render_sphere (k_proxy_sphere) against tests/proxy_sphere_ref.py, the float64 statement of its definition: the scenes and
conditions of tests/test_proxy_sphere_cpu.py with the kernel in front of them.

Off the ambiguity mask coverage must be equal, depth within DEPTH_FACTOR (2) x the error of the binary32 restatement of the same operator
sequence + 1e-6, and colour within 1e-4 + what the reference colour moves when the plane position moves by 4 * 2^-23 * (2 half_w tile_width)
(2 ulp each for atan2f and asinf).  Then the refusals, one by one, and gswt_proxy_render on a surface_type = 2 block untouched."""
import ctypes as C

import numpy as np
import pytest

from gswt_renderer_amd import _lib as L
from gswt_renderer_amd import atmosphere as A
from tests import frame_modes as FM
from tests import proxy_raster_ref as R
from tests import proxy_sphere_ref as S

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _defaults(renderer):
    """Every test leaves the shared context as it found it."""
    yield
    renderer.set_atmosphere(A.OFF)
    renderer.set_shadow_map(None)


def _draw(r, u, projection, W, H, mips, fog=None, shadow=None, depth_in=None, radius=S.RADIUS):
    import torch
    if mips is not None:
        r.proxy_configure(mips, grid_dim=24)
    r.set_atmosphere(fog if fog is not None else A.OFF)
    r.set_shadow_map(shadow)
    rgba = torch.from_numpy(R.sky(W, H)).cuda()
    depth = torch.zeros((H, W), dtype=torch.float32, device="cuda") if depth_in is None else torch.from_numpy(np.ascontiguousarray(depth_in)).cuda()
    torch.cuda.synchronize()
    r.proxy_render_sphere(u, radius, W, H, rgba.data_ptr(), depth.data_ptr(), clear_depth=depth_in is None, projection=projection)
    r.synchronize()
    return depth.cpu().numpy(), rgba.cpu().numpy()


@pytest.mark.parametrize("name", sorted(S.SCENES))
def test_kernel_matches_reference(renderer, name):
    u, projection, W, H, mips, fog, shadow, depth_in, res = S.scene_reference(name)
    got_d, got_c = _draw(renderer, u, projection, W, H, mips, fog, shadow, depth_in)
    din = np.ones((H, W)) if depth_in is None else depth_in
    off = ~res["amb"]
    raw_c = float(np.abs(got_c.astype(np.float64) - res["rgba"]).max(-1)[off].max())
    both = (got_d != din) & res["written"] & off
    raw_d = float(np.abs(got_d.astype(np.float64) - res["depth"])[both].max()) if both.any() else 0.0
    share, cover = S.conditions(res)
    print(f"{name}: cover {cover:.3f} mask {share:.3%} depth error {raw_d:.3e} (restatement {res['emu']:.3e}, bound {S.DEPTH_FACTOR * res['emu'] + 1e-6:.3e}) "
          f"colour error {raw_c:.3e} (allowance 1e-4 + up to {res['col_tol'].max():.2e})")
    S.compare(got_d, got_c, res, depth_in)
    unwritten = ~res["written"] & off
    assert FM.same(got_c[unwritten], R.sky(W, H)[unwritten])                        # the colour is loaded, not cleared
    if name == "black_background":
        wr = res["written"] & off
        assert (got_c[wr] == np.array([0.0, 0.0, 0.0, 1.0], np.float32)).all()
    if name == "incoming_depth":
        left = np.zeros((H, W), bool)
        left[:, :W // 2] = True
        assert FM.same(got_d[left], depth_in[left]) and (got_d[~left & res["written"]] < 1.0).all()


def test_depth_does_not_depend_on_fog_or_shade(renderer):
    u, projection, W, H, mips, _, _, _, _ = S.scene_reference("oblique")
    d0, c0 = _draw(renderer, u, projection, W, H, mips)
    d1, c1 = _draw(renderer, u, projection, W, H, mips, fog=S.fog_block(), shadow=S.shadow_block())
    wr = d0 < 1.0
    assert FM.same(d0, d1) and FM.same(c0[~wr], c1[~wr]) and not FM.same(c0[wr], c1[wr])


_MODE_REFS = {}


def _mode_reference(name, fog, shade):
    """The float64 reference of scene `name` under S.fog_block() / S.shadow_block(), computed once per process; nobody writes into it."""
    if (name, fog, shade) not in _MODE_REFS:
        u, projection, W, H, mips, _, _, _, plain = S.scene_reference(name)
        _MODE_REFS[name, fog, shade] = plain if not (fog or shade) else S.render(
            u, S.RADIUS, W, H, projection=projection, mips=mips, rgba_in=R.sky(W, H), fog=S.fog_block() if fog else None,
            shadow=S.shadow_block() if shade else None)
    return _MODE_REFS[name, fog, shade]


@pytest.mark.parametrize("name", ["oblique", "ortho_planet"])
def test_every_fog_and_shade_instantiation(renderer, name):
    """k_proxy_sphere<FOG, ORTHO, SHD> for all four (fog, shade) settings under each camera -- the scenes above launch five of the eight:
    each against the reference by S.compare; depth bit-equal across the four and unwritten pixels the incoming sky; and each switch moves
    the colour of at least MOVED (10 %) of the written pixels by more than 0.01, so that one instantiation cannot stand in for another
    (the float64 reference alone moves 18 % / 81 % of them with the shade and 99.9 % with the fog)."""
    MOVED = 0.10
    u, projection, W, H, mips, _, _, _, _ = S.scene_reference(name)
    sky = R.sky(W, H)
    got = {}
    for fog in (False, True):
        for shade in (False, True):
            res = _mode_reference(name, fog, shade)
            d, c = _draw(renderer, u, projection, W, H, mips, S.fog_block() if fog else None, S.shadow_block() if shade else None)
            off = ~res["amb"]
            raw_c = float(np.abs(c.astype(np.float64) - res["rgba"]).max(-1)[off].max())
            share, cover = S.conditions(res)
            derr, tol, cerr = S.compare(d, c, res)
            print(f"{name} fog {int(fog)} shade {int(shade)}: cover {cover:.3f} mask {share:.3%} depth error {derr:.3e} (bound {tol:.3e}) "
                  f"colour error {raw_c:.3e} (allowance 1e-4 + up to {res['col_tol'].max():.2e}; beyond it by {cerr:.3e}, bound 0)")
            unwritten = ~res["written"] & off
            assert FM.same(c[unwritten], sky[unwritten])
            got[fog, shade] = (d, c)
    d0, c0 = got[False, False]
    assert all(FM.same(d, d0) for d, _ in got.values())
    wr = d0 < 1.0

    def moved(a, b):
        return float((np.abs(got[a][1][wr].astype(np.float64) - got[b][1][wr])[:, :3].max(-1) > 0.01).mean())

    switches = {"shade, fog off": moved((False, False), (False, True)), "shade, fog on": moved((True, False), (True, True)),
                "fog, shade off": moved((False, False), (True, False)), "fog, shade on": moved((False, True), (True, True))}
    print(f"{name}: written pixels moved by more than 0.01 (floor {MOVED:.0%}): " + ", ".join(f"{k} {v:.1%}" for k, v in switches.items()))
    assert min(switches.values()) >= MOVED, switches


def test_depth_only_ground_on_a_fresh_context():
    """black_background before any gswt_proxy_configure: a sun map's occluder needs no texture; a textured draw is a state error."""
    from gswt_renderer_amd.renderer import GSWTError, GSWTRenderer
    u, projection, W, H, mips, _, _, _, res = S.scene_reference("black_background")
    r = GSWTRenderer(0)
    try:
        got_d, got_c = _draw(r, u, projection, W, H, None)
        S.compare(got_d, got_c, res)
        textured = S.scene_reference("oblique")[0]
        with pytest.raises(GSWTError) as e:
            _draw(r, textured, projection, W, H, None)
        assert e.value.code == L.GSWT_ERR_STATE
    finally:
        r.close()


def test_refusals(renderer):
    import torch
    lib, h = renderer._lib, renderer._h
    u0, _, W, H, mips, _, _, _, _ = S.scene_reference("oblique")
    uo = S.scene_reference("ortho_planet")[0]
    good = _draw(renderer, u0, 0, W, H, mips)
    rgba = torch.from_numpy(R.sky(W, H)).cuda()
    depth = torch.full((H, W), 0.25, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()

    def block(edit=None, base=u0):
        u = L.ProxyUniforms.from_buffer_copy(bytes(base))
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
    rp, dp = C.c_void_p(rgba.data_ptr()), C.c_void_p(depth.data_ptr())
    Rr = S.RADIUS
    # (what, block, radius, projection, rgba, depth, width, height, word of the reason)
    cases = [("null block", None, Rr, 0, rp, dp, W, H, b"bad argument"), ("null colour", block(), Rr, 0, None, dp, W, H, b"bad argument"),
             ("null depth", block(), Rr, 0, rp, None, W, H, b"bad argument"), ("width 0", block(), Rr, 0, rp, dp, 0, H, b"bad argument"),
             ("height -1", block(), Rr, 0, rp, dp, W, -1, b"bad argument"),
             ("tile_width 0", block(field("tile_width", 0.0)), Rr, 0, rp, dp, W, H, b"tile_width"),
             ("tile_width nan", block(field("tile_width", nan)), Rr, 0, rp, dp, W, H, b"tile_width"),
             ("singular perspective p[0]", block(proj(0, 0.0)), Rr, 0, rp, dp, W, H, b"singular"),
             ("singular perspective p[5]", block(proj(5, 0.0)), Rr, 0, rp, dp, W, H, b"singular"),
             ("projection 2", block(), Rr, 2, rp, dp, W, H, b"projection 2"), ("projection -1", block(), Rr, -1, rp, dp, W, H, b"projection -1"),
             ("radius 0", block(), 0.0, 0, rp, dp, W, H, b"sphere_radius"), ("radius -1", block(), -1.0, 0, rp, dp, W, H, b"sphere_radius"),
             ("radius nan", block(), nan, 0, rp, dp, W, H, b"sphere_radius"), ("radius inf", block(), inf, 0, rp, dp, W, H, b"sphere_radius"),
             ("radius + offset 0", block(field("height_offset", -Rr)), Rr, 0, rp, dp, W, H, b"height_offset"),
             ("radius + offset < 0", block(field("height_offset", -7.0)), Rr, 0, rp, dp, W, H, b"height_offset"),
             ("offset nan", block(field("height_offset", nan)), Rr, 0, rp, dp, W, H, b"height_offset"),
             ("half_w 0", block(lambda u: u.map_half_wh.__setitem__(0, 0)), Rr, 0, rp, dp, W, H, b"map_half_wh"),
             ("perspective matrix as orthographic", block(), Rr, 1, rp, dp, W, H, b"projection")]
    ob = lambda e=None: block(e, base=uo)
    cases += [(f"ortho bottom row p[{k}] = {v}", ob(proj(k, v)), Rr, 1, rp, dp, W, H, b"bottom row") for k, v in ((3, 1e-9), (7, -1.0), (11, nan), (15, 0.5))]
    cases += [(f"ortho shear p[{k}]", ob(proj(k, 1e-9)), Rr, 1, rp, dp, W, H, b"projection[%d]" % k) for k in (1, 2, 4, 6, 8, 9)]
    cases += [(f"ortho p[{k}] = {v}", ob(proj(k, v)), Rr, 1, rp, dp, W, H, b"projection[%d]" % k) for k in (0, 5, 10) for v in (0.0, nan, inf)]
    cases += [(f"ortho p[{k}] = {v}", ob(proj(k, v)), Rr, 1, rp, dp, W, H, b"projection[%d]" % k) for k in (12, 13, 14) for v in (nan, -inf)]
    cases += [("ortho singular view", ob(lambda u: [u.view.__setitem__(i, 0.0) for i in (0, 1, 2)]), Rr, 1, rp, dp, W, H, b"view")]
    for what, u, rad, pr, r_, d_, w_, h_, word in cases:
        assert lib.gswt_proxy_render_sphere(h, u, rad, pr, w_, h_, r_, d_, 1) == L.GSWT_ERR_BAD_ARG, what
        err = lib.gswt_last_error(h)
        assert word in err and b"gswt_proxy_render_sphere" in err, (what, err)
        renderer.synchronize()
        torch.cuda.synchronize()
        assert bool((depth == 0.25).all()) and FM.same(rgba.cpu().numpy(), R.sky(W, H)), what       # nothing enqueued, clear_depth not performed
    with pytest.raises(ValueError):
        renderer.proxy_render_sphere(u0, Rr, W, H, rgba.data_ptr(), depth.data_ptr(), True, projection=2)
    # the fields the pass does not read may hold anything
    junk = block(lambda u: (setattr(u, "map_proxy", 0), setattr(u, "width_scale", 0.0), setattr(u, "surface_type", 7),
                            [u.height_map_scale.__setitem__(i, nan) for i in range(3)]))
    d2 = torch.zeros((H, W), dtype=torch.float32, device="cuda")
    c2 = torch.from_numpy(R.sky(W, H)).cuda()
    torch.cuda.synchronize()
    assert lib.gswt_proxy_render_sphere(h, junk, Rr, 0, W, H, C.c_void_p(c2.data_ptr()), C.c_void_p(d2.data_ptr()), 1) == L.GSWT_OK
    renderer.synchronize()
    assert FM.same(d2.cpu().numpy(), good[0]) and FM.same(c2.cpu().numpy(), good[1])


def test_plane_passes_still_draw_the_plane_on_a_sphere_block(renderer):
    """gswt_proxy_render (and its orthographic form) with surface_type = 2 write what they write with surface_type = 0 on the same block,
    before and after a sphere draw on the context."""
    import torch
    from tests import proxy_ortho_ref as O
    cam_kw, draws, grid_dim, _ = R.SCENES["flat_two_draws"]
    W, H = 96, 72
    mips = R.mip_chain()
    renderer.configure(None)
    renderer.proxy_configure(mips, grid_dim=grid_dim)

    def plane(us, surface, projection):
        rgba = torch.from_numpy(R.sky(W, H)).cuda()
        depth = torch.zeros((H, W), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        for k, u in enumerate(us):
            v = L.ProxyUniforms.from_buffer_copy(bytes(u))
            v.surface_type = surface
            renderer.proxy_render(v, W, H, rgba.data_ptr(), depth.data_ptr(), clear_depth=(k == 0), projection=projection)
        renderer.synchronize()
        return depth.cpu().numpy(), rgba.cpu().numpy()

    us = R.scene_uniforms(R.scene_camera(cam_kw, W, H), draws)
    spec, odraws, _, _, _ = O.SCENES["full_grid_flat"]
    ous = O.scene_uniforms(O.make_camera(spec, W, H), odraws)
    for blocks, projection in ((us, 0), (ous, 1)):
        d0, c0 = plane(blocks, 0, projection)
        assert (d0 < 1.0).mean() > 0.2
        d2, c2 = plane(blocks, 2, projection)
        su, sp, sw, sh, smips, _, _, _, _ = S.scene_reference("oblique")
        _draw(renderer, su, sp, sw, sh, None)
        d2b, c2b = plane(blocks, 2, projection)
        assert FM.same(d0, d2) and FM.same(c0, c2) and FM.same(d0, d2b) and FM.same(c0, c2b)
