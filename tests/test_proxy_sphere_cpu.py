"""The sphere proxy pass's float64 reference (tests/proxy_sphere_ref.py) and the shared inverse of the sphere unfolding (host/gswt_surface.h:
sphere_plane_pos), without a GPU.

  * the reference's inverse composed with the oracle's restatement of sphere_get_uv / sphere_uv_to_pos (wangtile_oracle.WangTile._sphere_point)
    is the identity on each of the twenty pieces of the unfolding, and on random directions;
  * sphere_plane_pos, compiled for the host with the address and undefined-behaviour sanitizers into a stand-alone program
    (tools/sphere_plane_pos_main.cpp), agrees with the float64 inverse on poles, seam points, block corners and the u wrap;
  * known answers of the whole pass; and the GPU test's scenes satisfy its conditions on the reference alone."""
import math
import os
import subprocess

import numpy as np
import pytest

from oracle import wangtile_oracle as wo
from tests import proxy_raster_ref as R
from tests import proxy_sphere_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
BW = 8.0                       # (2 * 5 * 4) / 5: the block width of the scenes' map


class _Forward:
    """wangtile_oracle's sphere unfolding without a configured WangTile: _sphere_point reads nothing of the instance but _sincos."""
    _sincos = staticmethod(wo.WangTile._sincos)
    point = wo.WangTile._sphere_point


def _pieces():
    """(bidx, bidy, lower): five blocks by two rows, each cut by its diagonal by < bx -- caps and band halves, twenty in all."""
    return [(i, j, low) for i in range(5) for j in range(2) for low in (False, True)]


def _points_in_piece(rng, n, lower, margin=0.06):
    """n points (bx, by) / bw of the triangle by < bx (lower) or by > bx, at least `margin` from its three edges."""
    out = []
    while len(out) < n:
        a, b = rng.uniform(margin, 1.0 - margin, 2)
        if abs(a - b) < margin:
            continue
        if (b < a) == lower:
            out.append((a, b))
    return np.array(out)


@pytest.mark.parametrize("piece", _pieces())
def test_inverse_undoes_the_oracles_unfolding_on_every_piece(piece):
    """Forward in binary32 by the oracle, back in float64 by the reference.  The forward map's angles are binary32 numbers up to 2 pi
    (ulp 4.8e-7) through a sin / cos good to an ulp, so a direction is off by about 1e-6; at least 0.06 bw from the seams the inverse
    stretches that by no more than 1 / 0.06 in f (the caps' pinch) times bw 5 / (2 pi): 1e-6 * 17 * 0.8 bw = 1.4e-5 bw, bound 3e-5 bw."""
    bidx, bidy, lower = piece
    rng = np.random.default_rng(100 + 4 * bidx + 2 * bidy + int(lower))
    pts = _points_in_piece(rng, 24, lower) * BW
    fw = _Forward()
    worst = 0.0
    for bx, by in pts:
        n = fw.point(F32(BW), F32(bidx), F32(bidy), F32(bx), F32(by)).astype(np.float64)
        px, py, info = S.inverse_unfold(n[None, :], BW)
        assert int(info["bidx"][0]) == bidx and int(info["bidy"][0]) == bidy
        worst = max(worst, abs(px[0] - (bidx * BW + float(F32(bx)))), abs(py[0] - (bidy * BW + float(F32(by)))))
    assert worst <= 3e-5 * BW, worst
    # ... and against the float64 forward map (exact sin / cos) the round trip closes to rounding
    pts = _points_in_piece(rng, 2000, lower) * BW
    n = S.forward_unfold(BW, float(bidx), float(bidy), pts[:, 0], pts[:, 1])
    px, py, info = S.inverse_unfold(n, BW)
    assert (info["bidx"] == bidx).all() and (info["bidy"] == bidy).all()
    assert np.abs(px - (bidx * BW + pts[:, 0])).max() <= 1e-11 * BW and np.abs(py - (bidy * BW + pts[:, 1])).max() <= 1e-11 * BW


def _forward_of_plane(px, py, bw=BW):
    """Directions of plane positions (float64 forward map); a position on a block boundary belongs to either side: both are tried by the
    caller through `nudge`."""
    bidx = np.clip(np.floor(px / bw), 0, 4)
    bidy = np.clip(np.floor(py / bw), 0, 1)
    return S.forward_unfold(bw, bidx, bidy, px - bidx * bw, py - bidy * bw)


def test_random_directions_round_trip():
    rng = np.random.default_rng(7)
    n = rng.normal(size=(20000, 3))
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    px, py, info = S.inverse_unfold(n, BW)
    assert (px >= 0).all() and (px <= 5 * BW).all() and (py >= 0).all() and (py <= 2 * BW).all()
    assert set(np.unique(info["band"])) == {0, 1, 2} and set(np.unique(info["bidx"])) == {0.0, 1.0, 2.0, 3.0, 4.0}
    back = S.forward_unfold(BW, info["bidx"], info["bidy"], info["bx"], info["by"])
    assert np.abs(back - n).max() <= 1e-12


# ---- the shared GSWT_HD inverse under the host sanitizers -------------------------------------------------------------------------
def _fixed_directions():
    """Poles, seam points (v = 1/3 and 2/3 to the last bit either side, block boundaries f = 0, the mid bands' diagonal f = 1 - w), block
    corners, the u wrap (y = -0 and y a hair below 0 at x > 0), and a handful of ordinary directions."""
    def at(u, v):
        lon, lat = 2.0 * math.pi * u, (v - 0.5) * math.pi
        return (math.cos(lat) * math.cos(lon), math.cos(lat) * math.sin(lon), math.sin(lat))
    d = [(0.0, 0.0, 1.0), (0.0, 0.0, -1.0), (1.0, 0.0, 0.0), (-1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, -1.0, 0.0)]
    d += [(1.0, -0.0, 0.0), (1.0, -1e-9, 0.0), (1.0, 1e-9, 0.0), (0.6, -1e-12, 0.8)]                      # u wrap
    for v in (1.0 / 3.0, 2.0 / 3.0):
        d += [at(u, v + e) for u in (0.03, 0.31, 0.77) for e in (-1e-7, 0.0, 1e-7)]                      # band seams
    d += [at(k / 5.0, 0.2) for k in range(5)] + [at(k / 5.0 + 0.1, 0.8) for k in range(5)]              # cap block boundaries, f = 0
    d += [at(k / 5.0 + 0.05, 0.5) for k in range(5)]                                                     # mid bands: f = 0 at w = 0.5
    d += [at((k + 0.5 + 0.25) / 5.0, 0.5) for k in range(5)]                                             # mid bands: f = 1 - w
    d += [at(k / 5.0, 1.0 / 3.0) for k in range(5)] + [at(k / 5.0 + 0.1, 2.0 / 3.0) for k in range(5)]   # block corners
    rng = np.random.default_rng(3)
    r = rng.normal(size=(12, 3))
    d += [tuple(x) for x in r / np.linalg.norm(r, axis=1, keepdims=True)]
    return np.array(d, np.float64).astype(F32)


def test_shared_inverse_under_host_sanitizers(tmp_path):
    """sphere_plane_pos as the kernel calls it, on the host with -fsanitize=address,undefined in a program of its own.  Every result must
    be a plane position whose float64 forward image is the direction again (a seam point may land on either side of its seam: the sphere
    point is the same), and off the seams it must be the float64 inverse's position.

    Bounds: v and u carry asinf's / atan2f's rounding and two more operations, under 4 ulp of 1 = 2.4e-7 of a turn: 1.5e-6 in direction;
    with the 1e-6 bw nudge across a block boundary (4e-6 of a turn in the caps' pinch at s = 0.8) the bound is 1e-5.  In position that is plane_delta's 4 * 2^-23 * 5 bw = 2.4e-6 bw, times the caps' pinch 1 / (1 - s) <= 1 / 0.3 for the
    ordinary directions tested here: 8e-6 bw, bound 2e-5 bw."""
    exe = tmp_path / "sphere_plane_pos"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fno-fast-math", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-static-libasan", "-static-libubsan", "-I", os.path.join(ROOT, "gswt_renderer_amd", "csrc"), os.path.join(ROOT, "tools", "sphere_plane_pos_main.cpp"), "-o", str(exe)]
    subprocess.run(cmd, check=True)
    dirs = _fixed_directions()
    text = "".join(f"{BW!r} {float(x)!r} {float(y)!r} {float(z)!r}\n" for x, y, z in dirs)
    out = subprocess.run([str(exe)], input=text, capture_output=True, text=True)
    assert out.returncode == 0 and not out.stderr, out.stderr[-2000:]
    got = np.array([[float(t) for t in line.split()] for line in out.stdout.splitlines()])
    assert got.shape == (len(dirs), 2) and np.isfinite(got).all()
    assert (got[:, 0] >= 0).all() and (got[:, 0] <= 5 * BW).all() and (got[:, 1] >= 0).all() and (got[:, 1] <= 2 * BW).all()
    n = dirs.astype(np.float64)
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    # forward image: a position on a block boundary is tried a hair to either side of it
    err = np.full(len(dirs), np.inf)
    for ex in (-1e-6, 0.0, 1e-6):
        for ey in (-1e-6, 0.0, 1e-6):
            back = _forward_of_plane(np.clip(got[:, 0] + ex * BW, 0, 5 * BW), np.clip(got[:, 1] + ey * BW, 0, 2 * BW))
            err = np.minimum(err, np.abs(back - n).max(1))
    assert err.max() <= 1e-5, (err.max(), dirs[err.argmax()])
    px, py, info = S.inverse_unfold(n, BW)
    v, f, w = info["v"], info["f"], info["w"]
    with np.errstate(invalid="ignore"):
        seam = (np.abs(v - 1 / 3) < 1e-5) | (np.abs(v - 2 / 3) < 1e-5) | (f < 1e-5) | (f > 1 - 1e-5) | (np.abs(f - (1 - w)) < 1e-5) | \
               (np.abs(np.abs(n[:, 2]) - 1.0) < 1e-9)
    assert (~seam).sum() >= 12
    perr = np.maximum(np.abs(got[:, 0] - px), np.abs(got[:, 1] - py))[~seam]
    assert perr.max() <= 2e-5 * BW, perr.max()
    # the poles and the equator at longitude 0, exactly
    named = {(0.0, 0.0, 1.0): (4 * BW, 2 * BW), (0.0, 0.0, -1.0): (BW, 0.0), (1.0, 0.0, 0.0): (4.75 * BW, 1.25 * BW)}
    for k, (x, y, z) in enumerate(dirs[:3]):
        assert tuple(got[k]) == named[(float(x), float(y), float(z))]


# ---- known answers ------------------------------------------------------------------------------------------------------------------
def _axis_view(W=97, H=73, dist=20.0):
    from oracle import gswt_oracle as orc
    cam = orc.Camera(W, H, (dist, 0.0, 0.0), (0.0, 0.0, 0.0), [0, 0, 1])
    return orc.proxy_uniforms(cam, surface_type=2, map_proxy=1, **S.BLOCK), W, H


def test_centre_pixel_depth_on_the_x_axis():
    """97 x 73: the centre pixel's ndc is (0, 0), its ray the -x axis, its hit (r, 0, 0): depth = GP V (r, 0, 0, 1)."""
    u, W, H = _axis_view()
    res = S.render(u, S.RADIUS, W, H, mips=R.mip_chain())
    r = float(F32(S.RADIUS)) + float(F32(u.height_offset))
    V = np.asarray(u.view[:], np.float64).reshape(4, 4).T
    q = S._gp(u, np.float64) @ (V @ np.array([r, 0.0, 0.0, 1.0]))
    assert res["written"][H // 2, W // 2]
    assert abs(res["depth"][H // 2, W // 2] - q[2] / q[3]) <= 1e-12
    assert np.abs(res["geo"]["pos"][H // 2, W // 2] - (r, 0.0, 0.0)).max() <= 1e-9


def test_silhouette_radius():
    """From distance D the silhouette is the cone of half angle asin(r / D): on the centre row it spans tan(asin(r / D)) * P00 * W / 2
    pixels to either side of the centre."""
    u, W, H = _axis_view()
    res = S.render(u, S.RADIUS, W, H, mips=R.mip_chain())
    r = float(F32(S.RADIUS)) + float(F32(u.height_offset))
    want = math.tan(math.asin(r / 20.0)) * float(u.projection[0]) * W / 2.0
    row = res["geo"]["hit"][H // 2]
    assert abs((row.sum() - 1) / 2.0 - want) <= 1.0 and row[W // 2]
    col = res["geo"]["hit"][:, W // 2]
    assert abs((col.sum() - 1) / 2.0 - math.tan(math.asin(r / 20.0)) * float(u.projection[5]) * H / 2.0) <= 1.0


def test_equator_and_poles_land_where_the_forward_map_puts_them():
    fw = _Forward()
    for n, (px, py) in (((1.0, 0.0, 0.0), (4.75 * BW, 1.25 * BW)), ((0.0, 0.0, 1.0), (4 * BW, 2 * BW)), ((0.0, 0.0, -1.0), (BW, 0.0))):
        gx, gy, info = S.inverse_unfold(np.array([n]), BW)
        assert abs(gx[0] - px) <= 1e-12 and abs(gy[0] - py) <= 1e-12
        bidx, bidy = float(info["bidx"][0]), float(info["bidy"][0])
        back = fw.point(F32(BW), F32(bidx), F32(bidy), F32(px - bidx * BW), F32(py - bidy * BW)).astype(np.float64)
        assert np.abs(back - n).max() <= 2e-6, (n, back)
        assert np.abs(S.forward_unfold(BW, bidx, bidy, px - bidx * BW, py - bidy * BW) - n).max() <= 1e-15 * 4


# ---- the GPU test's scenes, on the reference alone -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(S.SCENES))
def test_scene_conditions(name):
    u, projection, W, H, mips, fog, shadow, depth_in, res = S.scene_reference(name)
    share, cover = S.conditions(res)
    assert share <= S.MAX_AMB and cover >= S.MIN_COVER, (share, cover)
    g = res["geo"]
    if name in ("inside", "clip_cap", "ortho_near_negative"):
        assert (g["root"][g["hit"]] == 1).mean() > 0.3           # the inside of the far surface shows
    if name == "incoming_depth":
        assert 0.3 < res["written"].sum() / g["hit"].sum() < 0.7
    if name == "grazing_horizon":
        o = np.linalg.norm(np.asarray(u.cam_pos[:3], np.float64))
        assert 0.0 < o - float(g["r"]) < 0.2
    # the binary32 restatement passes the bounds it scales: coverage equal off the mask, depth within its own error by construction
    g32 = res["geo32"]
    assert not ((g32["hit"] != g["hit"]) & ~res["amb"]).any()
