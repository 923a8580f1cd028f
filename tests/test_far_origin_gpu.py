"""Rendering far from the world origin, where the reference's camera-centred Wang-tile map puts every position after a long
flight (wangtile.rs:1684): cameras at |x|, |y| of 1e3 to 1e5 against the oracle, the chunk frustum cull on and off there (it
promises the same image bit for bit), the device worker stages there, and depth-order keys of splats whose depth is -0.0."""
import numpy as np
import pytest

from gswt_renderer_amd import _lib as L
from oracle import gswt_oracle as orc
from tests import helpers as H
from tests.test_end_to_end_gpu import _run_case

pytestmark = pytest.mark.gpu
TOL = 1e-4
W, HH = 272, 176

PLANE = dict(tile_map_half_wh=(3, 3), surface_type=0, lod_max_dist=20.0, tile_sort_type=3, merge_type=2)
HMAP = dict(tile_map_half_wh=(3, 4), surface_type=1, lod_max_dist=24.0, tile_sort_type=3, merge_type=2, height_map_wh=(4, 4),
            height_map_scale=(1.0, 1.0, 0.3))
# the Sphere map never shifts (wangtile.rs:1721-1723): far from the origin means a large sphere
SPHERE = dict(tile_map_half_wh=(5, 2), surface_type=2, sphere_radius=1000.0, lod_max_dist=200.0, tile_sort_type=3, merge_type=2)

FAR = [(1e3, 1, -1), (1e4, -1, 1), (1e5, -1, -1)]


def _cam(scale, sx, sy, grazing):
    x, y = sx * scale + 0.3, sy * scale - 0.7
    if grazing:     # eye inside the splat layer (z in +-0.6), nearly level: near splats sit on the near and side planes
        return (x, y, 0.3), (x + 3.0, y + 8.0, 0.25)
    return (x, y, 3.0), (x + 1.0, y + 2.0, 2.5)


def _render(renderer, cfg, cam, order_mode, no_cull):
    with renderer.options(NO_CHUNK_CULL=no_cull):
        img, ref, kinds, st = _run_case(renderer, cfg, cam, W, HH, lod0=500, order_mode=order_mode)
    t = renderer.timings()
    return img, ref, kinds, st, (t["n_visible"], t["n_pairs"])


@pytest.mark.parametrize("grazing,order_mode", [(False, L.GSWT_ORDER_REFERENCE), (True, L.GSWT_ORDER_REFERENCE), (True, L.GSWT_ORDER_DEPTH)],
                         ids=["level-ref", "grazing-ref", "grazing-depth"])
@pytest.mark.parametrize("far", FAR, ids=lambda f: f"{f[0]:.0e}{'+' if f[1] > 0 else '-'}{'+' if f[2] > 0 else '-'}")
@pytest.mark.parametrize("surface", ["plane", "hmap"])
def test_far_camera_matches_oracle_with_and_without_chunk_cull(renderer, surface, far, grazing, order_mode):
    """Every draw class present; _run_case pins n_visible / n_pairs to the oracle's.  The chunk cull (on by default) must leave image
    and counts bit-identical to GSWT_OPT_NO_CHUNK_CULL: the rounding of V * p grows with |p| here while the cull's margin does not."""
    cfg = PLANE if surface == "plane" else HMAP
    cam = _cam(*far, grazing)
    img, ref, kinds, st, n = _render(renderer, cfg, cam, order_mode, 0)
    assert kinds["plain"] > 0 and kinds["blend"] > 0 and kinds["merged"] > 0, kinds
    assert st["n_visible"] > 500
    err = H.max_abs_diff(img, ref)
    print(f"{surface} {far} grazing={grazing} order={order_mode}: max|gpu-oracle| = {err:.3e}")
    assert err <= TOL
    img1, _, _, _, n1 = _render(renderer, cfg, cam, order_mode, 1)
    assert n1 == n
    assert np.array_equal(img1.view(np.uint32), img.view(np.uint32))


@pytest.mark.parametrize("order_mode", [L.GSWT_ORDER_REFERENCE, L.GSWT_ORDER_DEPTH])
@pytest.mark.parametrize("cam", [((-700.0, 720.0, 30.0), (-690.0, 705.0, 32.0)), ((30.0, -1010.0, 200.0), (0.0, -990.0, 195.0))])
def test_far_sphere_surface_matches_oracle(renderer, cam, order_mode):
    """Sphere mapping at world coordinates of about 1e3 (gswt.wgsl's c - (center - half) * tile_width on a radius-1000 sphere)."""
    img, ref, kinds, st = _run_case(renderer, SPHERE, cam, W, HH, lod0=500, order_mode=order_mode)
    assert kinds["plain"] > 0 and st["n_visible"] > 200
    err = H.max_abs_diff(img, ref)
    print(f"sphere {cam[0]} order={order_mode}: max|gpu-oracle| = {err:.3e}")
    assert err <= TOL


def test_device_worker_stages_far_from_origin():
    """The device k_w_* stages byte for byte against libgswt_host at cameras 1e3..1e5 from the origin, stepping across tile
    boundaries (so build_tiles recentres the map), flat and HeightMap."""
    from gswt_renderer_amd import host
    from gswt_renderer_amd.worker import DeviceWorker
    from tests.test_worker_gpu import _cam as wcam, _compare, _pipe
    cams = []
    for scale, sx, sy in FAR:
        x, y = sx * scale + 0.37, sy * scale - 0.61
        cams += [((x, y, 3.0), (x + 1.0, y + 2.0, 2.5)), ((x + 4.3, y - 0.2, 3.0), (x + 5.0, y + 1.5, 2.5))]
    rng = np.random.default_rng(5)
    for kw, tex in ((dict(surface_type=host.SURFACE_NONE), None),
                    (dict(surface_type=host.SURFACE_HEIGHTMAP, height_map_type=host.HMAP_TEXTURE if hasattr(host, "HMAP_TEXTURE") else 0,
                          height_map_wh=(32, 32), height_map_scale=(1.0, 1.0, 0.6)), rng.random((16, 16), dtype=np.float32))):
        pipe, _ = _pipe((4, 4), dict(tile_sort_type=host.SORT_GRAPH, merge_type=host.MERGE_EDGE, lod_blending=True,
                                     lod_transition_width_ratio=0.1, merge_topk=16, merge_dot_threshold=0.5, lod_max_dist=7.0, **kw),
                        height_tex=tex)
        dw = DeviceWorker(pipe.renderer, pipe.wang)
        try:
            for k, (pos, tgt) in enumerate(cams):
                cu, vp = wcam(pos, tgt)
                ref = _compare(pipe, dw, pos, vp, rebuild=True, tag=f"surface {kw['surface_type']} cam {k}")
                assert ref["n"][0] > 0
        finally:
            dw.close()


def _zero_depth_scene(W, Hh):
    """Twelve overlapping splats around the view axis at view depth 2, in one screen tile.  The projection's z row is -0.0 except
    P[10] = 1 (so GP[10] = 0.5 - 0.5 = +0, and GP[2] = GP[6] = GP[14] = -0.0) and w = -z: q[2] is then -0.0 for a splat with view
    x > 0 and y > 0 and +0.0 for every other one, and both depths pass vs_main's 0 <= depth <= 1."""
    rng = np.random.default_rng(7)
    n = 12
    v = np.zeros((n, 62), np.float32)
    sx = np.tile([1, -1, 1, -1], 3)
    sy = np.repeat([1, -1, 1], 4) * np.tile([1, 1, -1, -1], 3)
    v[:, 0] = sx * rng.uniform(0.01, 0.08, n)
    v[:, 1] = sy * rng.uniform(0.01, 0.08, n)
    v[:, 6:9] = rng.normal(0, 1.5, (n, 3))
    v[:, 54] = 2.0
    v[:, 55:58] = np.log(rng.uniform(0.08, 0.2, (n, 3)))
    q = rng.normal(size=(n, 4))
    v[:, 58:62] = q / np.linalg.norm(q, axis=1, keepdims=True)
    pp = orc.preprocess([[orc.scene_load(v)]])
    case = H.Case(pp)
    case.add_static(lod=0, tile=0, view=8, offset=(0.0, 0.0, -2.0), valid_lod_id=0)
    P = np.zeros(16, np.float32)
    P[0] = P[5] = P[10] = 1.0
    P[11] = -1.0
    P[[2, 3, 6, 7, 14, 15]] = -0.0
    cu = orc.Camera176()
    cu.projection[:] = [float(x) for x in P]
    cu.view[:] = [float(x) for x in np.eye(4, dtype=np.float32).ravel()]
    cu.focal[:] = [W / 2.0, Hh / 2.0]
    cu.viewport[:] = [float(W), float(Hh)]
    cu.htan_fov[:] = [1.0, 1.0, 0.0, 0.0]
    cu.cam_pos[:] = [0.0, 0.0, 0.0, 0.0]
    return pp, case, cu, orc.scene_uniforms(num_lod=1)


@pytest.mark.parametrize("depth_sort", [0, 1])
def test_negative_zero_depth_ties_with_positive_zero(renderer, depth_sort):
    """GSWT_ORDER_DEPTH keys are depth bits; the oracle compares depths as floats, so -0.0 ties with +0.0 and keeps list order.
    -0.0's bits (0x80000000) must not sort it as the farthest splat."""
    W_, Hh = 48, 48
    pp, case, cu, su = _zero_depth_scene(W_, Hh)
    pr = orc.project_draws(cu, su, pp.tex, case.orc_draws)
    neg = np.signbit(pr["depth"])
    assert pr["visible"].all() and (pr["depth"] == 0.0).all() and 0 < neg.sum() < len(neg)
    ref, st = orc.render(cu, su, pp.tex, case.orc_draws, W_, Hh, order_mode=1)
    assert st["n_pairs16"] == len(neg)                    # one screen tile: every splat overlaps every other's tile
    renderer.upload_scene(pp.tex, pp.gs_index, pp.gs_lod_id)
    renderer.configure(None)
    renderer.set_draws(case.draws)
    with renderer.options(DEPTH_SORT=depth_sort):
        img = renderer.render(cu, su, W_, Hh, order_mode=L.GSWT_ORDER_DEPTH)
    t = renderer.timings()
    assert t["n_visible"] == st["n_visible"] and t["n_pairs"] == st["n_pairs16"]
    assert H.max_abs_diff(img, ref) <= TOL
