#!/usr/bin/env python3
"""Bits of the background passes, one line per render: sha256 of the depth and of the colour image (of the faces, for the bake).  Run once
per library -- GSWT_HIP_LIB selects libgswt_hip.so -- and compare the two outputs line for line (profiles/proxy_core_ab.txt).

  every scene of tests/proxy_raster_ref.SCENES (gswt_proxy_render) and tests/proxy_ortho_ref.SCENES (gswt_proxy_render_ortho), plain, with
      fog, with a sun map and with both: all eight k_proxy instantiations;
  every scene of tests/proxy_sphere_ref.SCENES as the tests draw it, and `oblique` / `ortho_planet` under the four (fog, shade) settings:
      all eight k_proxy_sphere instantiations;
  gswt_skybox_render of a seeded cube map in both `equirectangular` settings;
  gswt_skybox_configure_equirect of a seeded panorama into 64-texel faces, downloaded, and one render of it.
usage: tools/proxy_core_bits.py > lines.txt"""
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from gswt_renderer_amd import atmosphere as A
from gswt_renderer_amd import host, ortho, shadows
from gswt_renderer_amd.renderer import GSWTRenderer
from tests import proxy_ortho_ref as O
from tests import proxy_raster_ref as R
from tests import proxy_sphere_ref as S
from tests import shadow_ref as SR

W, H = 96, 72
FOG = A.Atmosphere(fog=(0.03, 5.0, 0.9, (0.6, 0.7, 0.8)))
# a sun over the scenes about the origin (proxy_ortho_ref's `sun` camera), 32 x 32, half of it in shadow
SUN = shadows.from_ortho_camera(ortho.OrthoCamera(32, 32, (30.0, -60.0, 45.0), (0.0, 0.0, 0.0), (0.0, 0.0, 1.0), 45.0, 10.0, 140.0),
                                SR.two_region_map(32, 32), bias=0.01, strength=0.75, shade_color=(0.05, 0.1, 0.2))


def sha(t):
    return hashlib.sha256(np.ascontiguousarray(t.cpu().numpy()).tobytes()).hexdigest()[:32]


def targets(w, h, depth_in=None):
    rgba = torch.from_numpy(R.sky(w, h)).cuda()
    depth = torch.zeros((h, w), dtype=torch.float32, device="cuda") if depth_in is None else torch.from_numpy(np.ascontiguousarray(depth_in)).cuda()
    torch.cuda.synchronize()
    return rgba, depth


def modes(fog_on, sun_on):
    for fog in (None, fog_on):
        for sun in (None, sun_on):
            yield f"fog {int(fog is not None)} sun {int(sun is not None)}", fog, sun


def plane(r, what, us, projection, grid_dim, hm):
    r.configure(hm)
    r.proxy_configure(R.mip_chain(), grid_dim=grid_dim)
    for label, fog, sun in modes(FOG, SUN):
        r.set_atmosphere(fog if fog is not None else A.OFF)
        r.set_shadow_map(sun)
        rgba, depth = targets(W, H)
        for k, u in enumerate(us):
            r.proxy_render(u, W, H, rgba.data_ptr(), depth.data_ptr(), clear_depth=(k == 0), projection=projection)
        r.synchronize()
        print(f"{what} {label}: depth {sha(depth)} colour {sha(rgba)}")


def sphere(r, what, u, projection, w, h, mips, fog, sun, depth_in=None):
    r.proxy_configure(mips, grid_dim=24)
    r.set_atmosphere(fog if fog is not None else A.OFF)
    r.set_shadow_map(sun)
    rgba, depth = targets(w, h, depth_in)
    r.proxy_render_sphere(u, S.RADIUS, w, h, rgba.data_ptr(), depth.data_ptr(), clear_depth=depth_in is None, projection=projection)
    r.synchronize()
    print(f"{what}: depth {sha(depth)} colour {sha(rgba)}")


def main():
    r = GSWTRenderer(0)
    for name in sorted(R.SCENES):
        cam_kw, draws, grid_dim, _ = R.SCENES[name]
        plane(r, f"proxy {name}", R.scene_uniforms(R.scene_camera(cam_kw, W, H), draws), 0, grid_dim, R.height_map())
    for name in sorted(O.SCENES):
        spec, draws, grid_dim, hm_n, _ = O.SCENES[name]
        plane(r, f"proxy_ortho {name}", O.scene_uniforms(O.make_camera(spec, W, H), draws), 1, grid_dim, R.height_map(n=hm_n))
    r.configure(None)
    for name in sorted(S.SCENES):
        u, projection, w, h, opt = S.scene_block(name)
        depth_in = None
        if opt.get("depth_in") == "half":                  # an incoming depth nearer than the sphere on the left half of the frame
            depth_in = np.ones((h, w), np.float32)
            depth_in[:, :w // 2] = 0.5
        sphere(r, f"proxy_sphere {name}", u, projection, w, h, R.mip_chain(), S.fog_block() if opt.get("fog") else None,
               S.shadow_block() if opt.get("shadow") else None, depth_in)
    for name in ("oblique", "ortho_planet"):
        u, projection, w, h, _ = S.scene_block(name)
        for label, fog, sun in modes(S.fog_block(), S.shadow_block()):
            sphere(r, f"proxy_sphere {name} {label}", u, projection, w, h, R.mip_chain(), fog, sun)
    r.set_atmosphere(A.OFF)
    r.set_shadow_map(None)
    # skybox: a seeded cube map in both settings, then a baked one
    rng = np.random.default_rng(7)
    cu, _ = host.camera_uniforms((1.0, -2.0, 0.5), (4.0, 3.0, 1.5), (0.0, 0.0, 1.0), 0.9, 0.1, 100.0, W, H)
    out = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
    faces = rng.uniform(0.0, 1.0, (6, 16, 16, 4)).astype(np.float32)
    for equi in (False, True):
        r.skybox_configure(faces, equirectangular=equi)
        r.skybox_render(cu, W, H, out.data_ptr())
        r.synchronize()
        print(f"skybox equirectangular {int(equi)}: colour {sha(out)}")
    r.skybox_configure_equirect(rng.uniform(0.0, 4.0, (50, 101, 4)).astype(np.float32), face_size=64)
    baked = r.skybox_download()
    print(f"skybox bake 101 x 50 -> 64: faces {hashlib.sha256(baked.tobytes()).hexdigest()[:32]}")
    r.skybox_render(cu, W, H, out.data_ptr())
    r.synchronize()
    print(f"skybox baked: colour {sha(out)}")
    r.close()


if __name__ == "__main__":
    main()
