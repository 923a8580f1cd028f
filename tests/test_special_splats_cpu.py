"""Host library vs oracle on splat records outside the benign region (tests/special_splats.py): loader rows and their importance
order, texture halves, the 9-view presort and the tile-zip round trip, bit for bit; every half pattern through the oracle's decode
against an independent float64 statement of gswt.wgsl:478-494; the column-band cull's covariance bound (gswt_upload_scene) on
decoded covariances that are not positive semi-definite.  CPU only."""
import math

import numpy as np
import pytest

from gswt_renderer_amd import host, synth
from oracle import gswt_oracle as orc
from tests import special_splats as S


@pytest.fixture(scope="module", params=[0, 1])
def hostile(request):
    verts, labels = S.hostile_tileset(seed=request.param)
    rows_o = [[orc.scene_load(v) for v in lod] for lod in verts]
    return verts, labels, rows_o


def _classes(labels, l, t):
    return sorted({c for _, c in labels[l][t]})


def test_hostile_tileset_holds_every_class(hostile):
    verts, labels, _ = hostile
    seen = {c for lod in labels for tile in lod for _, c in tile}
    assert seen == set(S.CLASSES)
    v = verts[1][3]
    assert not np.isfinite(v[:, :3]).all() and np.isnan(v[:, 6:9]).any()
    assert all(np.isfinite(verts[0][t][:, :3]).all() for t in range(len(verts[0])))


def test_scene_load_rows_and_order_bit_exact(hostile):
    verts, labels, rows_o = hostile
    ts = host.TileSet.from_vertices(verts)
    for l in range(len(verts)):
        for t in range(len(verts[l])):
            got = ts.rows(l, t)
            assert np.array_equal(got, rows_o[l][t]), (l, t, np.flatnonzero((got != rows_o[l][t]).any(axis=1))[:8], _classes(labels, l, t))
    # the saturating casts did happen: bytes 255 / 0 from f_dc = +-100, rotation bytes 0 from the zero quaternion
    allrows = np.concatenate([r for lod in rows_o for r in lod])
    assert (allrows[:, 24:27] == 255).any() and (allrows[:, 24:27] == 0).any()
    assert (allrows[:, 28:32] == 0).all(axis=1).any()
    assert {0, 1, 254, 255} <= set(allrows[:, 27].tolist())


def test_generate_texture_bit_exact(hostile):
    _, _, rows_o = hostile
    rows = np.concatenate([r for lod in rows_o for r in lod])
    want = orc.generate_texture(rows)
    got = host.generate_texture(rows)
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, (bad[:8], got[bad[:4]], want[bad[:4]])
    halves = np.concatenate([want[:, 4:7] & 0xFFFF, want[:, 4:7] >> 16], axis=1)
    assert (((halves >> 10) & 0x1F) == 0).any() and (halves & 0x7FFF != 0)[((halves >> 10) & 0x1F) == 0].any()   # subnormal halves
    assert ((halves & 0x7FFF) == 0x7C00).any()                                                                   # overflow to Inf


def test_preprocess_bit_exact(hostile):
    verts, labels, rows_o = hostile
    pp = orc.preprocess(rows_o)
    w = host.WangTile(host.TileSet.from_vertices(verts))
    tex, gi, li = w.preload()
    assert np.array_equal(tex, pp.tex)
    assert np.array_equal(w.lod_avg_scale(), pp.lod_avg_scale)
    for t in range(pp.n_tile):
        c, a = w.tile_base(t)
        assert np.array_equal(c, pp.tile_center[t]) and np.array_equal(a, pp.aabb[t])
    nan_depth = False
    for l in range(pp.n_lod):
        for t in range(pp.n_tile):
            assert w.merge_offset(l, t) == pp.merge_offset[l, t]
            for v in range(pp.n_view):
                assert np.array_equal(w.raw_depth(l, t, v), pp.raw_depth[l][t][v]), (l, t, v, _classes(labels, l, t))
                assert np.array_equal(gi[l][t][v], pp.gs_index[l][t][v]), (l, t, v, _classes(labels, l, t))
                assert np.array_equal(li[l][t][v], pp.gs_lod_id[l][t][v]), (l, t, v)
            nan_depth |= not np.isfinite(orc.rows_positions(pp.rows[l][t])).all()
    assert nan_depth                                     # non-finite positions reached the presort (test_k5 semantics)


def test_tile_zip_round_trip(hostile, tmp_path):
    verts, _, rows_o = hostile
    zbytes = synth.tile_zip_bytes(verts)
    p = tmp_path / "hostile.zip"
    p.write_bytes(zbytes)
    ts = host.TileSet.from_zip(zbytes)
    assert ts.dims() == (len(verts), len(verts[0]))
    orows = orc.load_scene_zip(str(p))
    for l in range(len(verts)):
        for t in range(len(verts[l])):
            assert np.array_equal(ts.rows(l, t), rows_o[l][t]), (l, t)
            assert np.array_equal(orows[l][t], rows_o[l][t]), (l, t)


# ---- halves ---------------------------------------------------------------------------------------------------------
def shader_half_f64(h):
    """gswt.wgsl:478-494 from the bit fields, in float64: exponent 0 -> fraction / 1024 * 2^-15 (not IEEE's 2^-14), exponent 31
    (Inf, NaN) -> 0, otherwise (1 + fraction / 1024) * 2^(exponent - 15)."""
    h = np.asarray(h, dtype=np.int64)
    sign = np.where(h & 0x8000, -1.0, 1.0)
    e = (h >> 10) & 0x1F
    fr = (h & 0x3FF).astype(np.float64)
    normal = np.ldexp(1.0 + fr / 1024.0, (e - 15).astype(np.int32))
    sub = fr / 1024.0 * 2.0 ** -15
    return np.where(e == 31, 0.0, sign * np.where(e == 0, sub, normal))


ALL_HALVES = np.arange(65536, dtype=np.int64)


def test_every_half_pattern_decodes_as_the_shader():
    want = shader_half_f64(ALL_HALVES)
    got = np.array([orc.half_to_float(int(h)) for h in ALL_HALVES], dtype=np.float64)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, [(hex(int(h)), got[h], want[h]) for h in bad[:8]]
    # the edges the decode has to get right
    assert want[0x0400] == 2.0 ** -14 and want[0x03FF] == 1023 / 1024 * 2.0 ** -15 and want[0x7BFF] == 65504.0
    assert want[0x7C00] == want[0xFC00] == want[0x7E00] == want[0xFFFF] == 0.0


def band_half_val(h):
    """Python restatement of half_to_float (host/gswt_math.h: the decode of gswt_upload_scene's and k_scene_tex's band-cull bound), in
    float32 like the C++."""
    h = int(h)
    e, fr = (h >> 10) & 0x1F, h & 0x3FF
    if e == 31:
        return np.float32(0.0)
    m = np.float32(fr) * np.float32(2.98023223876953125e-08) if e == 0 else np.float32(math.ldexp(1.0 + fr / 1024.0, e - 15))
    return -m if h & 0x8000 else m


def test_band_cull_half_val_never_below_the_shader():
    want = shader_half_f64(ALL_HALVES)
    got = np.array([band_half_val(h) for h in ALL_HALVES], dtype=np.float64)
    assert (got >= want).all(), [hex(int(h)) for h in np.flatnonzero(got < want)[:8]]
    assert np.array_equal(got, want)                       # it is in fact the shader's decode, exactly


def band_cov_bound(halves6):
    """Python restatement of the per-record bound of gswt_upload_scene (cov_extent_bound, host/gswt_math.h): the sum of the positive
    eigenvalues of the decoded covariance, bounded from above -- the trace when the decoded matrix is positive semi-definite (every principal minor >= 0),
    otherwise (trace + sqrt(3) |S|_F) / 2 (the nuclear norm is at most sqrt(3) times the Frobenius norm)."""
    xx, xy, xz, yy, yz, zz = [float(band_half_val(h)) for h in halves6]
    tr = xx + yy + zz
    psd = (xx >= 0 and yy >= 0 and zz >= 0 and xx * yy - xy * xy >= 0 and xx * zz - xz * xz >= 0 and yy * zz - yz * yz >= 0
           and xx * (yy * zz - yz * yz) - xy * (xy * zz - yz * xz) + xz * (xy * yz - yy * xz) >= 0)
    if psd:
        return tr
    fro = math.sqrt(xx * xx + yy * yy + zz * zz + 2.0 * (xy * xy + xz * xz + yz * yz))
    return 0.5 * (tr + math.sqrt(3.0) * fro) * (1.0 + 1e-6)


def _decoded(h6):
    xx, xy, xz, yy, yz, zz = shader_half_f64(np.array(h6))
    return np.array([[xx, xy, xz], [xy, yy, yz], [xz, yz, zz]])


def test_band_cull_bound_on_indefinite_decoded_covariances():
    """The decode makes stored covariances indefinite in two ways.  A needle (one scale ~ e^-12 .. e^-20) stores a subnormal diagonal
    that the decode halves while its off-diagonals stay: lambda_1 exceeds the trace by a few 1e-5 relative, inside the band cull's 25 %
    slack.  A floater whose stored diagonal overflowed to Inf reads that diagonal as 0 beside finite off-diagonals: lambda_1 is then
    several times the trace, which the slack does not cover -- so the bound is the sum of the positive eigenvalues, not the trace
    (tests/test_special_splats_gpu.py renders such rows in column bands).  Raw rows with a negative diagonal exceed the trace without
    limit."""
    rng = np.random.default_rng(11)
    n = 4000
    v = np.zeros((n, 62), dtype=np.float32)
    v[:, 55:58] = rng.normal(math.log(0.05), 1.0, size=(n, 3))
    v[np.arange(n), 55 + rng.integers(0, 3, n)] = rng.uniform(-20.0, -6.0, n)
    v[:, 55 + rng.integers(0, 3)] += rng.uniform(0.0, 6.0, n).astype(np.float32)
    q = rng.normal(size=(n, 4))
    v[:, 58:62] = q / np.linalg.norm(q, axis=1, keepdims=True)
    v[:, 54] = 3.0
    tex = orc.generate_texture(orc.scene_load(v))
    worst = {"subnormal": 0.0, "overflow": 0.0}
    n_indef = 0
    for r in tex:
        h6 = [int(r[4] & 0xFFFF), int(r[4] >> 16), int(r[5] & 0xFFFF), int(r[5] >> 16), int(r[6] & 0xFFFF), int(r[6] >> 16)]
        Sd = _decoded(h6)
        ev = np.linalg.eigvalsh(Sd)
        assert band_cov_bound(h6) >= ev[ev > 0].sum() * (1.0 - 1e-12), (h6, ev)
        if ev[0] < 0:
            n_indef += 1
            kind = "overflow" if any(h & 0x7C00 == 0x7C00 for h in h6) else "subnormal"
            worst[kind] = max(worst[kind], ev[-1] / np.trace(Sd) - 1.0)
    assert n_indef > 100                                  # the decode made many stored covariances indefinite
    assert 0.0 < worst["subnormal"] < 1e-3, worst         # halved subnormal diagonals: inside the 25 % slack
    assert worst["overflow"] > 1.0, worst                 # overflowed diagonals: lambda_1 > 2 x trace
    # raw rows: a negative diagonal, an indefinite 2x2 block, Inf / NaN halves (decode to 0)
    for h6 in (S.cov_halves(xx=10.0, yy=-19.0, zz=10.0), S.cov_halves(xx=1000.0, yy=-1999.0, zz=1000.0), S.cov_halves(xy=300.0, zz=1.0),
               [0x7C00, 0x4900, 0, 0x7C00, 0, 0x3C00], [0xFC00, 0x3C00, 0, 0x7E01, 0, 0x3C00]):
        ev = np.linalg.eigvalsh(_decoded(h6))
        assert band_cov_bound(h6) >= ev[ev > 0].sum(), (h6, ev)
    h6 = S.cov_halves(xx=1000.0, yy=-1999.0, zz=1000.0)
    assert np.linalg.eigvalsh(_decoded(h6))[-1] > 50 * np.trace(_decoded(h6))       # the trace alone is far below lambda_1
