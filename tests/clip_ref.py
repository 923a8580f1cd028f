"""CPU reference of the clip volumes (gswt_set_clip_volumes, include/gswt_hip.h), in numpy.  No tests here: tests/test_clip_cpu.py pins
this module and the volume sets below without a GPU, tests/test_clip_gpu.py and tests/test_clip_proxy_gpu.py compare the device with it.

The test.  `inside_f32` restates the header's arithmetic operator by operator in np.float32 -- one rounding per written `*` and `+`,
the rows summed in the written order ((M0 c0 + M1 c1) + M2 c2) + M3, ordinary IEEE compares, so a NaN coordinate is not inside and a
point on the boundary is --, `inside_f64` is the same function in float64, and `hidden` applies the rule: a point stays exactly when
(there is no keep volume, or it is inside at least one) and it is inside no cut volume.  On the plain surface the tested point is
tests/shadow_ref.py's `centres_f32`, the device's own binary32 numbers, and every operation is correctly rounded on the device too: the
comparison is exact, no mask.

Where the centre is not restated (HeightMap and Sphere surfaces: the float64 unprojection of the splat's own unclipped record,
AR.unproject_f64; the proxy passes: the float64 hit point of their references) a point within a margin of a volume's boundary may
fall on either side and is masked.  The boundary function b is  max|u| - 1  (box),  u.u - 1  (ellipsoid),  u2  (half-space): inside
is b <= 0.  With the position off by at most `delta` world units (SR.persp_delta, or mode_stack_ref's orthographic form, `position_delta`)
  * u_r is off by at most  e_r = delta * sum_k |M_rk|  +  8 * 2^-24 * (sum_k |M_rk c_k| + |M_r3|):  the position's error pushed through the
    row's absolute values, plus the device's own evaluation (three products, three sums: 6 roundings of 2^-24 relative to the largest
    partial sum, which the sum of the absolute terms bounds; 8 leaves room for the float64 -> binary32 rounding of c itself);
  * box:        |max|u| - 1| moves by at most max_r e_r;
  * half-space: u2 moves by e_2;
  * ellipsoid:  u.u moves by at most sum_r (2 |u_r| e_r + e_r^2), and the device's three squares and two sums add 5 roundings relative
                to u.u: + 8 * 2^-24 * u.u.
`margins` is that bound per volume and point; `masked` is |b| <= margin for any volume of the set."""
from __future__ import annotations

import struct

import numpy as np

from gswt_renderer_amd import clip as CL
from tests import atmosphere_ref as AR
from tests import shadow_ref as SR

F32 = np.float32
U = 2.0 ** -24


def params(volumes) -> list:
    """The packed records as the library reads them: per volume dict(M [3, 4] binary32, shape, flags)."""
    raw = bytes(volumes) if isinstance(volumes, (bytes, bytearray)) else CL.pack(volumes)
    out = []
    for k in range(len(raw) // CL.VOLUME_BYTES):
        v = struct.unpack("<12f2I2I", raw[64 * k:64 * k + 64])
        out.append(dict(M=np.array(v[:12], F32).reshape(3, 4), shape=int(v[12]), flags=int(v[13])))
    return out


def _unit(v, c0, c1, c2, ft):
    """u0, u1, u2 in the float type ft, the header's sums."""
    M = v["M"].astype(ft)
    c0, c1, c2 = (np.asarray(x, ft) for x in (c0, c1, c2))
    with np.errstate(all="ignore"):
        return [((M[r, 0] * c0 + M[r, 1] * c1) + M[r, 2] * c2) + M[r, 3] for r in range(3)]


def _inside(v, c0, c1, c2, ft):
    u0, u1, u2 = _unit(v, c0, c1, c2, ft)
    with np.errstate(all="ignore"):
        if v["shape"] == CL.HALFSPACE:
            return u2 <= ft(0.0)
        if v["shape"] == CL.BOX:
            return (np.abs(u0) <= ft(1.0)) & (np.abs(u1) <= ft(1.0)) & (np.abs(u2) <= ft(1.0))
        return (u0 * u0 + u1 * u1) + u2 * u2 <= ft(1.0)


def inside_f32(volume, c0, c1, c2):
    return _inside(volume, c0, c1, c2, F32)


def inside_f64(volume, c0, c1, c2):
    return _inside(volume, c0, c1, c2, np.float64)


def hidden(volumes, c0, c1, c2, inside=inside_f32, ground_only=False):
    """The visibility rule over `volumes` (params(...)); ground_only: over the volumes flagged GROUND alone, as the proxy passes see them."""
    vols = [v for v in volumes if not ground_only or v["flags"] & CL.GROUND]
    n = np.asarray(c0).shape
    keeps = [v for v in vols if v["flags"] & CL.KEEP]
    in_keep = np.ones(n, bool) if not keeps else np.zeros(n, bool)
    in_cut = np.zeros(n, bool)
    for v in vols:
        ins = inside(v, c0, c1, c2)
        if v["flags"] & CL.KEEP:
            in_keep |= ins
        else:
            in_cut |= ins
    return ~in_keep | in_cut


def boundary_f64(volume, pos):
    """b [n] of the module docstring at the float64 points pos [n, 3]."""
    u0, u1, u2 = _unit(volume, pos[:, 0], pos[:, 1], pos[:, 2], np.float64)
    if volume["shape"] == CL.HALFSPACE:
        return u2
    if volume["shape"] == CL.BOX:
        return np.maximum(np.maximum(np.abs(u0), np.abs(u1)), np.abs(u2)) - 1.0
    return (u0 * u0 + u1 * u1) + u2 * u2 - 1.0


def margins(volume, pos, delta):
    """What b can be off by per point (module docstring), from the float64 position pos [n, 3] and its error bound delta."""
    M = volume["M"].astype(np.float64)
    pos = np.asarray(pos, np.float64)
    e = [delta * np.abs(M[r, :3]).sum() + 8.0 * U * (np.abs(pos * M[r, :3][None, :]).sum(1) + abs(M[r, 3])) for r in range(3)]
    if volume["shape"] == CL.HALFSPACE:
        return e[2]
    if volume["shape"] == CL.BOX:
        return np.maximum(np.maximum(e[0], e[1]), e[2])
    u = _unit(volume, pos[:, 0], pos[:, 1], pos[:, 2], np.float64)
    uu = (u[0] * u[0] + u[1] * u[1]) + u[2] * u[2]
    return sum(2.0 * np.abs(u[r]) * e[r] + e[r] * e[r] for r in range(3)) + 8.0 * U * uu


def masked(volumes, pos, delta, ground_only=False):
    """Points whose b lies within its margin of 0 for any volume of the set: they may fall on either side."""
    out = np.zeros(np.asarray(pos).shape[0], bool)
    for v in volumes:
        if not ground_only or v["flags"] & CL.GROUND:
            out |= np.abs(boundary_f64(v, pos)) <= margins(v, pos, delta)
    return out


def position_delta(block, ortho, pos, z):
    """The error bound of a position unprojected from a record's binary32 ndc and depth (tests/shadow_ref.py: persp_delta under the
    perspective camera; tests/mode_stack_ref.py's orthographic form, where depth is linear: its rounding times the depth range along the
    ray, plus the coordinates' own)."""
    if ortho:
        span = 2.0 / abs(float(block.projection[10]))
        return AR.DEPTH_ROUNDINGS * U * (span + np.abs(pos).max(1))
    return SR.persp_delta(z, AR.near_of(block))


def rot_z(deg):
    a = np.deg2rad(deg)
    return np.array([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]])


def rot_x(deg):
    a = np.deg2rad(deg)
    return np.array([[1.0, 0.0, 0.0], [0.0, np.cos(a), -np.sin(a)], [0.0, np.sin(a), np.cos(a)]])


# ---- the volume sets of the GPU tests -------------------------------------------------------------------------------------------------------
# One family of sets per golden case, placed by a centre C and a size S in the part of the world the case's frames show (the plane and the
# HeightMap case: a slab of +-0.5 about z = 0 over x, y of a few tile widths; the Sphere case: the planet of radius 6.8 about the origin, the
# cameras on its -y, +z side).  tests/test_clip_cpu.py holds the conditions they meet on every camera they are used with.
PLACES = {"case_plane": ((2.5, 6.5, 0.0), 4.0), "case_hmap": ((2.0, 4.0, 0.0), 3.0), "case_sphere": ((1.0, -4.5, 2.0), 5.5)}
CASE_CAMERAS = {"case_plane": ("persp", "oblique"), "case_hmap": ("persp",), "case_sphere": ("persp", "top")}
SET_NAMES = ("cut", "keep", "half", "eight")


def volume_sets(case, ground=False) -> dict:
    """name -> list of clip.ClipVolume: "cut" one rotated box as a cut, "keep" one ellipsoid as a keep, "half" a half-space aligned with no
    axis, "eight" two keeps and six cuts of mixed shapes; "all" hides everything (a cut half-space far above the world) and "none" nothing
    (a keep box of half extent 10^6).  ground: every volume carries GSWT_CLIP_GROUND too."""
    C, S = PLACES[case]
    C = np.array(C)
    at = lambda *f: C + S * np.array(f)
    V, kw = CL.ClipVolume, dict(ground=ground)
    rot = rot_z(30.0) @ rot_x(20.0)
    return {
        "cut": [V.box(at(-0.3, 0.4, 0.0), (0.8 * S, 0.6 * S, S), rot, **kw)],
        "keep": [V.ellipsoid(at(0.1, 0.1, 0.0), (1.1 * S, 0.8 * S, 1.2 * S), rot_z(-25.0), keep=True, **kw)],
        "half": [V.half_space(at(0.0, 0.1, 0.0), (1.0, 0.6, 0.3), **kw)],
        "eight": [V.ellipsoid(at(-0.2, 0.2, 0.0), (1.0 * S, 0.9 * S, 1.3 * S), rot_z(15.0), keep=True, **kw),
                  V.box(at(1.4, -0.3, 0.0), (0.5 * S, 0.7 * S, S), rot_z(20.0), keep=True, **kw),
                  V.box(at(-0.5, 0.5, 0.0), (0.3 * S, 0.25 * S, S), rot_z(45.0), **kw),
                  V.ellipsoid(at(0.3, -0.2, 0.0), (0.35 * S, 0.3 * S, S), rot_x(10.0), **kw),
                  V.half_space(at(0.0, -0.75, 0.0), (0.2, 1.0, 0.1), **kw),
                  V.box(at(1.5, -0.4, 0.1), (0.2 * S, 0.2 * S, 0.5 * S), rot, **kw),
                  V.ellipsoid(at(-0.9, 0.0, 0.0), (0.25 * S, 0.4 * S, S), **kw),
                  V.half_space(at(-1.15, 0.0, 0.0), (1.0, 0.1, 0.0), **kw)],
        "all": [V.half_space((0.0, 0.0, 1.0e6), (0.0, 0.0, 1.0), **kw)],
        "none": [V.box((0.0, 0.0, 0.0), (1.0e6, 1.0e6, 1.0e6), keep=True, **kw)],
    }


def centres_f64(case, cam):
    """(float64 position [n, 3] of every instance of the case's unclipped frame under the camera -- the device's own binary32 centre on
    the plain surface, the unprojection of the record elsewhere, NaN where the unclipped frame does not show the instance --, its error
    bound delta [n] (0 on the plain surface), the unclipped records)."""
    from oracle import gswt_oracle as orc
    from tests import frame_modes as FM
    g, cu, su, proj, unf = FM.view(case, cam)
    n = unf.shape[0]
    vis = unf["visible"] == 1
    if case == "case_plane":
        return np.stack(SR.centres_f32(su, g["pp"].tex, g["draws"]), 1).astype(np.float64), np.zeros(n), unf
    block = orc.Camera176.from_buffer_copy(bytes(cu))
    pos, delta = np.full((n, 3), np.nan), np.zeros(n)
    p, z = AR.unproject_f64(block, unf["ndc"][vis], unf["depth"][vis])
    pos[vis], delta[vis] = p, position_delta(block, proj == FM.ORTHO, p, z)
    return pos, delta, unf


def expected(case, cam, volumes):
    """(hidden [n], masked [n], unclipped records) of the case's instances under the packed or listed `volumes`: on the plain surface the
    binary32 restatement over every instance with an empty mask, elsewhere float64 with the margins' mask; there the rows the unclipped
    frame does not show have no position: not hidden, and masked."""
    pos, delta, unf = centres_f64(case, cam)
    vols = params(volumes)
    vis = unf["visible"] == 1
    if case == "case_plane":
        c = pos.astype(F32)
        return hidden(vols, c[:, 0], c[:, 1], c[:, 2]), np.zeros(vis.shape, bool), unf
    hid, msk = np.zeros(vis.shape, bool), ~vis
    hid[vis] = hidden(vols, pos[vis, 0], pos[vis, 1], pos[vis, 2], inside_f64)
    msk[vis] = masked(vols, pos[vis], delta[vis])
    return hid, msk, unf


def pair_counts(case, cam, aa_s=0.0):
    """Pairs per instance of the case's unclipped frame under the camera (the oracle's pair rectangles; aa_s: the pixel filter's s)."""
    from oracle import gswt_oracle as orc
    from tests import frame_modes as FM
    g, cu, su, proj, _ = FM.view(case, cam)
    with orc.frame_mode(ortho=int(proj == FM.ORTHO), aa_s=float(aa_s)):
        r = orc.pair_rects(orc.Camera176.from_buffer_copy(bytes(cu)), su, g["pp"].tex, g["draws"], FM.W, FM.Hh, height_map=g["hm"])
    n = (r["tx1"] - r["tx0"] + 1).astype(np.int64) * (r["ty1"] - r["ty0"] + 1)
    return np.where((r["visible"] == 1) & (r["tx1"] >= r["tx0"]) & (r["ty1"] >= r["ty0"]), n, 0)


# ---- the proxy passes ---------------------------------------------------------------------------------------------------------------------------
# The float64 hit point of every pixel of four scenes of the proxy references -- tests/proxy_raster_ref.py "oblique" (plane, perspective),
# tests/proxy_ortho_ref.py "isometric" (plane, orthographic), tests/proxy_sphere_ref.py "oblique" and "ortho_planet" (sphere, both
# projections) -- and what it can be off by against the kernel's own: the reference's stated depth bound (DEPTH_FACTOR x its binary32
# emulation's error + 1e-6) times what a unit of depth is in world units along the ray (z^2 / near under the perspective camera,
# far - near under the orthographic one), plus 8 * 2^-24 * max|pos| for the kernel's o + t d at the world coordinates' magnitude
# (tests/test_shadow_gpu.py's proxy cases).  A pixel's status under a GROUND set follows from its hit point, the boundary functions and
# `margins`: hidden beyond the margin, kept beyond it, or undecided; the reference's own ambiguous pixels are undecided too.
PROXY_SCENES = ("plane_persp", "plane_ortho", "sphere_persp", "sphere_ortho")


def _pixel_ndc(W, H):
    ys, xs = np.mgrid[0:H, 0:W]
    return np.stack([((xs + 0.5) / W * 2.0 - 1.0).ravel(), (1.0 - (ys + 0.5) / H * 2.0).ravel()], 1)


def _depth_unit(block, ortho, z):
    """World units along the ray per unit of depth."""
    if ortho:
        return np.full(np.shape(z), 2.0 / abs(float(block.projection[10])))
    return np.asarray(z, np.float64) ** 2 / AR.near_of(block)


_PROXY = {}


def proxy_scene(kind) -> dict:
    """dict(kind, u or us, W, H, projection, grid_dim, hm, mips, radius; hit [H, W], amb [H, W], pos [H, W, 3] float64 (NaN off the hits),
    delta [H, W]); the sphere scenes also carry cand: per candidate root (alive [H, W], pos, dep, delta)."""
    if kind in _PROXY:
        return _PROXY[kind]
    from tests import proxy_ortho_ref as O
    from tests import proxy_raster_ref as R
    from tests import proxy_sphere_ref as S
    ortho = kind.endswith("ortho")
    if kind.startswith("plane"):
        if ortho:
            us, grid_dim, hm, mips, _, (depth, _, amb, res, _) = O.scene_reference("isometric")
            W, H = O.W0, O.H0
            tol = O.depth_tol(us, W, H, res, amb)[0]
        else:
            cam_kw, draws, grid_dim, _ = R.SCENES["oblique"]
            W, H = R.W0, R.H0
            us = R.scene_uniforms(R.scene_camera(cam_kw, W, H), draws)
            hm, mips = R.height_map(), R.mip_chain()
            depth, _, amb, res, _ = R.reference(us, W, H, grid_dim=grid_dim, hm=hm, mips=mips)
            tol = O.DEPTH_FACTOR * R.emulated_error(us, W, H, res, amb) + 1e-6
        assert len(us) == 1
        hit = depth < 1.0
        pos, z = AR.unproject_f64(us[0], _pixel_ndc(W, H), depth.ravel())
        pos, z = pos.reshape(H, W, 3), z.reshape(H, W)
        pos[~hit] = np.nan
        with np.errstate(invalid="ignore"):
            delta = tol * _depth_unit(us[0], ortho, z) + 8.0 * U * np.abs(pos).max(-1)
        out = dict(kind=kind, us=us, W=W, H=H, projection=int(ortho), grid_dim=grid_dim, hm=hm, mips=mips, hit=hit, amb=amb, pos=pos, delta=delta)
    else:
        u, projection, W, H, mips, _, _, _, res = S.scene_reference("ortho_planet" if ortho else "oblique")
        assert projection == int(ortho)
        tol = S.DEPTH_FACTOR * res["emu"] + 1e-6
        ys, xs = np.mgrid[0:H, 0:W]
        o, d = S.rays(u, W, H, projection, np.float64, xs.ravel(), ys.ravel())
        r = float(F32(S.RADIUS)) + float(F32(u.height_offset))
        tc, h, _, disc = S.cut(o, d, r, np.float64)
        cand = []
        for sgn in (-1.0, 1.0):
            t = tc + sgn * h
            p = o + t[..., None] * d
            dep, qw = S._depth(u, p, np.float64)
            with np.errstate(invalid="ignore"):
                alive = (disc >= 0) & (t > 0) & (qw > 0) & (dep >= 0) & (dep <= 1)
                delta = tol * _depth_unit(u, ortho, qw) + 8.0 * U * np.abs(p).max(-1)
            cand.append(dict(alive=alive.reshape(H, W), pos=p.reshape(H, W, 3), dep=np.asarray(dep, np.float64).reshape(H, W), delta=delta.reshape(H, W)))
        g = res["geo"]
        assert int(u.use_clip) == 0 and np.array_equal(g["hit"], cand[0]["alive"] | cand[1]["alive"])
        first = cand[0]["alive"]
        pos = np.where(first[..., None], cand[0]["pos"], cand[1]["pos"])
        pos[~g["hit"]] = np.nan
        out = dict(kind=kind, u=u, W=W, H=H, projection=projection, mips=mips, radius=S.RADIUS, hit=g["hit"], amb=res["amb"], pos=pos,
                   delta=np.where(first, cand[0]["delta"], cand[1]["delta"]), cand=cand, depth_tol=tol)
    _PROXY[kind] = out
    return out


def proxy_volumes(sc, near_cap=False) -> dict:
    """The GROUND sets of a proxy scene, placed over the middle of what the unclipped pass draws: "cut" a rotated box as a cut, "keep" an
    ellipsoid as a keep, and their twins without the flag ("unflagged").  near_cap (sphere): one cut ellipsoid about the sphere's point
    nearest the eye, which removes the near surface of the pixels around the frame's middle and leaves the far surface in sight."""
    p = sc["pos"][sc["hit"]]
    lo, mid, hi = np.percentile(p, 15, axis=0), np.percentile(p, 50, axis=0), np.percentile(p, 85, axis=0)
    ext = np.maximum(hi - lo, 1e-3)
    V = CL.ClipVolume
    if near_cap:
        y, x = sc["H"] // 2, sc["W"] // 2
        c = sc["cand"][0]["pos"][y, x]
        return {"near_cap": [V.ellipsoid(c, (3.0, 3.0, 3.0), ground=True)]}
    big = float(np.abs(p - mid).max()) + 1.0
    box = dict(center=mid + 0.1 * ext, half_extents=(0.45 * ext[0], 0.45 * ext[1], big), rotation=rot_z(30.0))
    ell = dict(center=mid - 0.05 * ext, radii=(0.8 * ext[0], 0.8 * ext[1], 2.0 * big), rotation=rot_z(-20.0))
    if sc["kind"].startswith("sphere"):         # a planet: volumes of the hits' own extent in every direction
        box["half_extents"] = tuple(0.45 * ext)
        ell["radii"] = tuple(0.8 * ext)
    return {"cut": [V.box(box["center"], box["half_extents"], box["rotation"], ground=True)],
            "keep": [V.ellipsoid(ell["center"], ell["radii"], ell["rotation"], keep=True, ground=True)],
            "unflagged": [V.box(box["center"], box["half_extents"], box["rotation"]), V.ellipsoid(ell["center"], ell["radii"], ell["rotation"], keep=True)]}


def point_status(volumes, pos, delta):
    """(hidden beyond the margin, kept beyond the margin) of the float64 points pos [..., 3] under the GROUND volumes of the set; NaN points
    are neither."""
    vols = params(volumes)
    shape = pos.shape[:-1]
    p, dl = pos.reshape(-1, 3), np.asarray(delta, np.float64).reshape(-1)
    ok = np.isfinite(p).all(1)
    hid, und = np.zeros(p.shape[0], bool), np.ones(p.shape[0], bool)
    hid[ok] = hidden(vols, p[ok, 0], p[ok, 1], p[ok, 2], inside_f64, ground_only=True)
    und[ok] = masked(vols, p[ok], dl[ok], ground_only=True)
    return (hid & ~und & ok).reshape(shape), (~hid & ~und & ok).reshape(shape)


def proxy_expect(sc, volumes) -> dict:
    """Per pixel of the scene under the set: `clear` (holds the clear colour and depth exactly), `same` (equals the unclipped pass bit
    for bit), `far` (sphere: the near candidate is hidden and the far one kept: its depth is `far_depth`), and `undecided` (the rest)."""
    amb, hit = sc["amb"], sc["hit"]
    if "cand" not in sc:
        hid, kept = point_status(volumes, sc["pos"], sc["delta"])
        clear, same, far, far_depth = hid & ~amb, (kept | ~hit) & ~amb, np.zeros(hit.shape, bool), None
    else:
        c0, c1 = sc["cand"]
        h0, k0 = point_status(volumes, c0["pos"], c0["delta"])
        h1, k1 = point_status(volumes, c1["pos"], c1["delta"])
        a0, a1 = c0["alive"], c1["alive"]
        gone0 = ~a0 | h0                                          # the near candidate is out: not alive, or hidden beyond the margin
        same = (~hit | (a0 & k0) | (~a0 & a1 & k1)) & ~amb
        far = a0 & h0 & a1 & k1 & ~amb
        clear = hit & gone0 & (~a1 | h1) & ~amb
        far_depth = c1["dep"]
    return dict(clear=clear, same=same, far=far, far_depth=far_depth, undecided=~(clear | same | far))
