"""What the sphere proxy pass (gswt_proxy_render_sphere) is for: the ground that hides the far hemisphere of a Sphere scene, and the
occluder of a sun map that makes the planet's night side dark."""

import numpy as np
import pytest

from gswt_renderer_amd import host, ortho, shadows, synth
from gswt_renderer_amd.pipeline import GSWTPipeline
from gswt_renderer_amd.renderer import PICK_NONE
from oracle import gswt_oracle as orc
from tests import proxy_raster_ref as R
from tests import proxy_sphere_ref as S

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _defaults(renderer):
    yield
    renderer.set_shadow_map(None)
    renderer.configure(None)


def test_far_hemisphere_is_hidden_behind_the_sphere_proxy(renderer):
    """The small Sphere scene of test_sphere_surface_end_to_end (half (5, 2), R 6.5, 320 x 240) with its pick image, over the cleared depth
    and over the sphere proxy's depth.  Without the ground some pixels pick a splat of the far hemisphere -- one whose depth lies behind
    the ground sphere at that pixel --; with it no pixel picks a splat at or behind the ground, and the ground fills the silhouette."""
    import torch
    W, H, RAD, OFFSET = 320, 240, 6.5, -0.3
    cfg = dict(tile_map_half_wh=(5, 2), surface_type=2, sphere_radius=RAD, lod_max_dist=60.0, tile_sort_type=3, merge_type=2)
    pos, tgt = (3.0, -19.0, 6.0), (0.0, 0.0, 0.0)
    verts = synth.make_tileset(n_lod=3, n_tile=16, lod0_count=700)
    cu, vp = host.camera_uniforms(pos, tgt, (0, 0, 1), 45.0, 0.1, 2400.0, W, H)
    pipe = GSWTPipeline(verts, host.user_data(**cfg), renderer=renderer)
    pipe.update(pos, vp)
    su = pipe.wang.scene_uniforms()
    u = orc.proxy_uniforms(orc.Camera(W, H, pos, tgt, [0, 0, 1]), surface_type=2, map_proxy=1, height_offset=OFFSET, tile_width=float(su.tile_width),
                           map_half_wh=tuple(su.map_half_wh), center_coord=tuple(su.center_coord))
    u.view[:] = list(cu.view)                      # the frame's own matrices: ground and splats are depth-tested in one clip space
    u.projection[:] = list(cu.projection)
    renderer.proxy_configure(R.mip_chain(), grid_dim=24)
    rgba = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
    depth = torch.zeros((H, W), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    renderer.proxy_render_sphere(u, RAD, W, H, rgba.data_ptr(), depth.data_ptr(), clear_depth=True)
    renderer.synchronize()
    ground_d, ground_c = depth.cpu().numpy(), rgba.cpu().numpy()
    # every pixel inside the silhouette is written
    geo = S.evaluate(u, RAD, W, H, 0, np.float64)
    inside = geo["hit"] & ~geo["amb"]
    assert 0.2 < inside.mean() < 0.8
    assert (ground_d[inside] < 1.0).all() and (ground_c[inside][:, 3] == 1.0).all() and (ground_d[~geo["hit"] & ~geo["amb"]] == 1.0).all()
    _, bare = pipe.render(cu, W, H, pick=True)
    img, covered = pipe.render(cu, W, H, pick=True, bg_rgba=ground_c, bg_depth=ground_d)
    on_planet = ground_d < 1.0
    far = on_planet & (bare["map_index"] != PICK_NONE) & (bare["depth"] >= ground_d)
    print(f"far-hemisphere picks without the ground: {int(far.sum())} of {int(on_planet.sum())} pixels on the planet; "
          f"picked with the ground: {int((covered['map_index'] != PICK_NONE).sum())}")
    assert far.sum() > 0, "the scene does not show the defect: no pixel picks a far-hemisphere splat without the ground"
    picked = covered["map_index"] != PICK_NONE
    assert picked[on_planet].mean() > 0.2                                     # the near hemisphere is still there
    assert not (picked & (covered["depth"] >= ground_d)).any()
    assert (covered["depth"][~picked] == ground_d[~picked]).all()             # an unpicked pixel reports the ground's depth
    assert (np.abs(img[on_planet][:, 3] - 1.0) <= 1e-5).all()


def _unit(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v)


# The sun test's geometry.  A 2 x 2 compare footprint at the map's limb reaches texels that hold no ground (depth 1: lit) up to sqrt(2)
# texels beyond a point, and on the day side texels up to sqrt(2) texels inward, nearer the sun.  With n.sun = c a point lies r (1 - sqrt(1 -
# c^2)) inside the limb: 0.005 r at |c| = 0.1.  So the band |c| < 0.1 can be left to the limb only by a map with texels under 0.005 r /
# sqrt(2) = 0.0035 r: a 128^2 map of the whole planet has r / 64.  The map is therefore a close-up of the terminator where the view looks,
# 2 world units wide (texel 1 / 64 = 0.0025 r at r = 6.25), as a host's cascade nearest the eye would be.
SUN = _unit((1.0, -0.5, 0.3))
ACROSS = _unit(np.cross(SUN, (0.0, 0.0, 1.0)))             # perpendicular to the sun: a point of the terminator lies along it
ALONG = np.cross(ACROSS, SUN)                              # the terminator's tangent there
SUN_HALF, SUN_NEAR, SUN_FAR, SUN_DIST = 1.0, 10.0, 30.0, 20.0
# day side: the compare's inward texels lie nearer the sun by at most sqrt(r^2 - (rho - d)^2) - sqrt(r^2 - rho^2), d = sqrt(2) / 64, largest
# at c = 0.1 (rho = 0.99499 r): 0.19 world units; 0.25 is the bias.  Night side at c = -0.1: the occluder is 2 r |c| = 1.25 nearer, less the
# same 0.19 at the outward texels: 1.06 > 0.25.
BIAS_WORLD = 0.25
STRENGTH, SHADE = 0.6, (0.05, 0.1, 0.3)


def test_sun_map_of_the_sphere_proxy_darkens_the_night_side(renderer):
    import torch
    RAD = S.RADIUS
    r = RAD + S.BLOCK["height_offset"]
    T = r * ACROSS
    sun_cam = ortho.OrthoCamera(128, 128, T + SUN_DIST * SUN, T, ALONG, SUN_HALF, SUN_NEAR, SUN_FAR)
    renderer.proxy_configure(R.mip_chain(), grid_dim=24)
    renderer.set_shadow_map(None)
    zmap = torch.zeros((128, 128), dtype=torch.float32, device="cuda")
    scratch = torch.zeros((128, 128, 4), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    su = sun_cam.proxy_uniforms(surface_type=2, map_proxy=1, black_background=1, **{k: v for k, v in S.BLOCK.items() if k != "brightness"})
    renderer.proxy_render_sphere(su, RAD, 128, 128, scratch.data_ptr(), zmap.data_ptr(), clear_depth=True, projection=1)
    renderer.synchronize()
    z = zmap.cpu().numpy()
    assert 0.3 < (z < 1.0).mean() < 0.7                                        # the limb runs through the map
    light = shadows.from_ortho_camera(sun_cam, z, bias=BIAS_WORLD / (SUN_FAR - SUN_NEAR), strength=STRENGTH, shade_color=SHADE)
    # the view: 2 world units above the terminator point, looking down at it, the sun to the right of the image
    W, H = 96, 72
    cam = orc.Camera(W, H, tuple(T * (1.0 + 2.0 / r)), (0.0, 0.0, 0.0), list(ALONG))
    u = orc.proxy_uniforms(cam, surface_type=2, map_proxy=1, **S.BLOCK)

    def draw(shadow):
        renderer.set_shadow_map(shadow)
        rgba = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
        depth = torch.zeros((H, W), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        renderer.proxy_render_sphere(u, RAD, W, H, rgba.data_ptr(), depth.data_ptr(), clear_depth=True)
        renderer.synchronize()
        return depth.cpu().numpy(), rgba.cpu().numpy().astype(np.float64)

    d0, plain = draw(None)
    d1, shaded = draw(light)
    assert np.array_equal(d0, d1) and (d0 < 1.0).all()                         # the ground fills this close-up
    geo = S.evaluate(u, RAD, W, H, 0, np.float64)
    c = (geo["pos"] / r) @ SUN
    night, day = c < -0.1, c > 0.1
    assert night.mean() > 0.1 and day.mean() > 0.1
    want = plain[..., :3] * (1.0 - STRENGTH) + np.array(SHADE) * STRENGTH
    nerr = np.abs(shaded[..., :3] - want)[night].max()
    derr = np.abs(shaded[..., :3] - plain[..., :3])[day].max()
    print(f"night side: {int(night.sum())} pixels, off the full shade by {nerr:.3e}; day side: {int(day.sum())} pixels, off the unshaded colour by {derr:.3e}")
    assert nerr <= 1e-6 and derr == 0.0
    assert (shaded[..., 3] == 1.0).all()
