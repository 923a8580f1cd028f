"""CPU reference of the pick image (gswt_render_pick, include/gswt_hip.h), in numpy.

Walks the projected instances of orc.project_draws exactly as tests/depth_ref.py does -- the oracle's blend order in both order modes, its
fragment sequence F1..F4 in binary32, its depth test against bg_depth (1.0 without one) -- and keeps, for every pixel, EVERY covering
instance with its blend weight w_i = T_i e_i.  The coverage decisions are binary32; the weights are binary64, computed from the binary32
r^2 and alpha: e = exp(-r2) alpha, T_i = prod over the instances in front (1 - e_j).  From those: the arg-max per pixel (front-most of
equal weights), the runner-up's weight, and per instance its identity (map_index, entry, depth) from the draw list.

It is only trusted because its colour reproduces orc.render (tests/test_pick_cpu.py)."""
from __future__ import annotations

import numpy as np

from tests import depth_ref as DR

F32 = np.float32
NONE = 0xFFFFFFFF
TOL = 1e-4            # the image contract: a weight is a colour contribution with c = 1


def identities(draws, *, merged_lod: str = "zero"):
    """(map_index, entry) of every instance of the oracle draw list `draws` (orc.Draw), in draw order.  entry is the list word
    gs_index | lod_id << 28.  A static draw's instances carry the draw's TileUniforms.map_index, a merged draw's their own map id.
    A merged draw without per-splat LOD ids: merged_lod = "zero" -- gswt_set_draws uploads the word without LOD bits --, "single" -- the
    device-built lists of gswt_set_draws_merge_groups carry the member's LOD, the draw's single_lod_id."""
    mi, en = [], []
    for d in draws:
        gs = np.asarray(d.gs_index, dtype=np.uint32)
        if d.lod_id is not None:
            lod = np.asarray(d.lod_id, dtype=np.uint32)
        elif merged_lod == "single" and d.tile.single_draw == 1:
            lod = np.full(gs.shape, max(int(d.tile.single_lod_id), 0), np.uint32)
        else:
            lod = np.zeros(gs.shape, np.uint32)
        en.append(gs | (lod << np.uint32(28)))
        mi.append(np.asarray(d.map_id, dtype=np.uint32) if d.tile.single_draw == 1 else np.full(gs.shape, d.tile.map_index, np.uint32))
    return np.concatenate(mi), np.concatenate(en)


def composite(sp, W: int, H: int, *, splat_scale: float = 1.0, order_mode: int = 0, bg_rgba=None, bg_depth=None):
    """The covering events of the frame, sorted by pixel and, inside a pixel, FRONT TO BACK:
    dict(img [H, W, 4] f32 (the colour, as depth_ref composites it), zbg [H, W] f32,
         pix, inst, e (binary64), w (binary64), rank (position in the pixel's front-to-back list), start [H*W + 1] (events of pixel p =
         start[p] .. start[p + 1]))."""
    fs = DR._frag_setup(sp, splat_scale, W, H)
    vis = (sp["visible"] == 1) & fs["ok"]
    idx = np.nonzero(vis)[0]
    if order_mode == 1:
        idx = idx[np.argsort(-sp["depth"][idx].astype(np.float64), kind="stable")]
    img = np.zeros((H, W, 4), F32) if bg_rgba is None else np.array(bg_rgba, F32).reshape(H, W, 4)
    zbg = np.ones((H, W), F32) if bg_depth is None else np.array(bg_depth, F32).reshape(H, W)
    hW, hH = F32(0.5) * F32(W), F32(0.5) * F32(H)
    ev_pix, ev_inst, ev_seq, ev_e = [], [], [], []
    for seq, k in enumerate(idx):               # back to front
        fx0, fx1, fy0, fy1 = fs["fx0"][k], fs["fx1"][k], fs["fy0"][k], fs["fy1"][k]
        if not (fx1 >= fx0 and fy1 >= fy0 and fx1 >= 0 and fy1 >= 0 and fx0 <= W - 1 and fy0 <= H - 1):
            continue
        x0, x1 = (0 if fx0 < 0 else int(fx0)), (W - 1 if fx1 > W - 1 else int(fx1))
        y0, y1 = (0 if fy0 < 0 else int(fy0)), (H - 1 if fy1 > H - 1 else int(fy1))
        xs = np.arange(x0, x1 + 1, dtype=np.int64)[None, :]
        ys = np.arange(y0, y1 + 1, dtype=np.int64)[:, None]
        bx, by = (xs & ~15).astype(F32), (ys & ~15).astype(F32)
        iux, iuy, ivx, ivy = fs["iux"][k], fs["iuy"][k], fs["ivx"][k], fs["ivy"][k]
        ox = DR._fma(hW, sp["ndc"][k, 0], hW - bx)
        oy = DR._fma(-hH, sp["ndc"][k, 1], hH - by)
        nku = -DR._fma(iux, ox, iuy * oy)
        nkv = -DR._fma(ivx, ox, ivy * oy)
        ly = (ys.astype(F32) - by) + F32(0.5)
        lx = (xs.astype(F32) - bx) + F32(0.5)
        px = DR._fma(iux, lx, DR._fma(iuy, ly, nku))
        py = DR._fma(ivx, lx, DR._fma(ivy, ly, nkv))
        r2 = DR._fma(py, py, px * px)
        dk = F32(sp["depth"][k])
        cover = (r2 <= F32(4.0)) & (dk < zbg[y0:y1 + 1, x0:x1 + 1])
        if not cover.any():
            continue
        cy, cx = np.nonzero(cover)
        cy, cx = cy + y0, cx + x0
        alpha = F32(sp["rgba"][k, 3])
        B = np.exp(-r2[cover]).astype(F32) * alpha
        om = F32(1.0) - B
        d = img[cy, cx]
        rgba = sp["rgba"][k].astype(F32)
        d[:, 0] = B * rgba[0] + d[:, 0] * om
        d[:, 1] = B * rgba[1] + d[:, 1] * om
        d[:, 2] = B * rgba[2] + d[:, 2] * om
        d[:, 3] = B + d[:, 3] * om
        img[cy, cx] = d
        ev_pix.append(cy * W + cx)
        ev_inst.append(np.full(cy.shape, k, np.int64))
        ev_seq.append(np.full(cy.shape, seq, np.int64))
        ev_e.append(np.exp(-r2[cover].astype(np.float64)) * np.float64(alpha))
    cat = lambda a, t: np.concatenate(a) if a else np.zeros(0, t)
    pix, inst, seq, e = cat(ev_pix, np.int64), cat(ev_inst, np.int64), cat(ev_seq, np.int64), cat(ev_e, np.float64)
    o = np.lexsort((-seq, pix))                 # by pixel; the later in blend order, the nearer: front to back
    pix, inst, e = pix[o], inst[o], e[o]
    start = np.searchsorted(pix, np.arange(W * H + 1))
    rank = np.arange(pix.size) - start[pix]
    w = np.zeros(pix.size, np.float64)
    T = np.ones(W * H, np.float64)
    for r in range(int(rank.max()) + 1 if pix.size else 0):
        s = np.nonzero(rank == r)[0]
        w[s] = T[pix[s]] * e[s]
        T[pix[s]] *= 1.0 - e[s]
    return dict(img=img, zbg=zbg, W=W, H=H, pix=pix, inst=inst, e=e, w=w, rank=rank, start=start, T_final=T.reshape(H, W))


def winners(ev):
    """Per pixel [H, W]: best (event index of the largest weight, the front-most of equal ones; -1: no splat covers the pixel), w1 (its
    weight, 0 without one), w2 (the largest weight of any OTHER event of the pixel, 0 without one), n (covering events)."""
    W, H, pix, w, start = ev["W"], ev["H"], ev["pix"], ev["w"], ev["start"]
    n = np.diff(start)
    best = np.full(W * H, -1, np.int64)
    w1, w2 = np.zeros(W * H), np.zeros(W * H)
    if pix.size:
        o = np.lexsort((np.arange(pix.size), -w, pix))          # per pixel: descending weight, then front to back
        first = o[start[:-1][n > 0]]
        best[n > 0] = first
        w1[n > 0] = w[first]
        two = n > 1
        w2[two] = w[o[start[:-1][two] + 1]]
    return dict(best=best.reshape(H, W), w1=w1.reshape(H, W), w2=w2.reshape(H, W), n=n.reshape(H, W))


def indecisive_share(win, tol: float = TOL):
    """Share of the covered pixels whose leader leads the runner-up by <= 2 tol (the exact-identity check leaves them out)."""
    cov = win["n"] > 0
    ind = cov & (win["w1"] - win["w2"] <= 2.0 * tol)
    return float(ind.sum()) / max(int(cov.sum()), 1), ind


def fold_segments(ev, seg_len: int):
    """The pick as the segmented compositor computes it, on the reference's events: every pixel's front-to-back list is cut into
    segments of seg_len events, each walked from T = 1 in binary32 (local weights w' = T' e, local winner with a strict >, the
    segment's transmittance), and the segments folded front to back: candidate T_prefix * w'_max, strict >.  Returns the winning
    event per pixel [H, W] (-1: none)."""
    W, H, pix, rank, e = ev["W"], ev["H"], ev["pix"], ev["rank"], ev["e"].astype(F32)
    best = np.full(W * H, -1, np.int64)
    wbest = np.zeros(W * H, F32)
    Tpre = np.ones(W * H, F32)            # transmittance in front of the current segment
    Tloc = np.ones(W * H, F32)
    lbest = np.full(W * H, -1, np.int64)
    lw = np.zeros(W * H, F32)

    def close(p):                          # fold the finished segment of pixels p
        c = Tpre[p] * lw[p]
        up = c > wbest[p]
        best[p[up]] = lbest[p[up]]
        wbest[p[up]] = c[up]
        Tpre[p] = Tpre[p] * Tloc[p]
        Tloc[p] = F32(1.0)
        lw[p] = F32(0.0)
        lbest[p] = -1

    for r in range(int(rank.max()) + 1 if pix.size else 0):
        s = np.nonzero(rank == r)[0]
        p = pix[s]
        if r > 0 and r % seg_len == 0:
            close(p)
        wl = Tloc[p] * e[s]
        up = wl > lw[p]
        lbest[p[up]] = s[up]
        lw[p[up]] = wl[up]
        Tloc[p] = Tloc[p] - wl
    close(np.arange(W * H))
    return best.reshape(H, W)


def check_pick(pick, ev, sp, map_index, entry, *, tol: float = TOL, label: str = ""):
    """The checks of a pick image [H, W] (PICK_DTYPE) against the reference events `ev` of instances `sp` with identities (map_index,
    entry); prints the figures, then asserts.  Returns the largest |weight - w_ref|."""
    W, H = ev["W"], ev["H"]
    win = winners(ev)
    cov = win["n"] > 0
    share, ind = indecisive_share(win)
    pk = np.ascontiguousarray(pick).reshape(H * W)
    covf = cov.reshape(-1)
    # uncovered pixels: the no-hit record with z_bg exactly
    free = ~covf
    ok_free = ((pk["map_index"][free] == NONE) & (pk["entry"][free] == NONE) & (pk["weight"][free] == 0.0) &
               (pk["depth"][free].view(np.uint32) == ev["zbg"].reshape(-1)[free].view(np.uint32)))
    # covered pixels: the returned identity names an event of the pixel
    key = (map_index.astype(np.uint64) << np.uint64(32)) | entry.astype(np.uint64)
    uk, kid = np.unique(key, return_inverse=True)
    nk = np.uint64(uk.size + 1)
    ev_key = ev["pix"].astype(np.uint64) * nk + kid[ev["inst"]].astype(np.uint64)
    eo = np.lexsort((-ev["w"], ev_key))                       # equal (pixel, identity) twice: the heavier instance first
    ev_key_s = ev_key[eo]
    pc = np.nonzero(covf)[0]
    gk = (pk["map_index"][pc].astype(np.uint64) << np.uint64(32)) | pk["entry"][pc].astype(np.uint64)
    gi = np.searchsorted(uk, gk)
    known = (gi < uk.size) & (uk[np.minimum(gi, uk.size - 1)] == gk)
    want_key = pc.astype(np.uint64) * nk + gi.astype(np.uint64)
    at = np.searchsorted(ev_key_s, want_key)
    named = known & (at < ev_key_s.size) & (ev_key_s[np.minimum(at, ev_key_s.size - 1)] == want_key)
    evi = eo[np.minimum(at, ev_key_s.size - 1)]               # the named event
    dup = int((np.diff(ev_key_s) == 0).sum())
    w_ref = ev["w"][evi]
    w1 = win["w1"].reshape(-1)[pc]
    dw = np.abs(pk["weight"][pc].astype(np.float64) - w_ref)
    short = w1 - w_ref
    depth_ok = pk["depth"][pc].view(np.uint32) == sp["depth"][ev["inst"][evi]].astype(F32).view(np.uint32)
    decisive = ~ind.reshape(-1)[pc]
    same = evi == win["best"].reshape(-1)[pc]
    in_range = (pk["weight"][pc] > 0.0) & (pk["weight"][pc] <= 1.0)
    print(f"pick_check {label}: covered={pc.size} free={int(free.sum())} indecisive={share:.4f} dup_events={dup} named={int(named.sum())} "
          f"max|w-w_ref|={float(dw[named].max()) if named.any() else 0.0:.3e} max(w1-w_ref)={float(short[named].max()) if named.any() else 0.0:.3e} "
          f"depth_bit_equal={int((depth_ok & named).sum())} decisive_same={int((same & decisive & named).sum())}/{int(decisive.sum())} "
          f"free_ok={int(ok_free.sum())}")
    assert ok_free.all(), "no-hit record"
    assert named.all(), "identity names no covering instance"
    assert in_range.all(), "weight outside (0, 1]"
    assert (short <= tol).all(), float(short.max())
    assert (dw <= tol).all(), float(dw.max())
    assert depth_ok.all(), "depth is not the instance's vertex-stage depth"
    assert same[decisive].all(), "identity differs from the reference arg-max on a decisive pixel"
    return float(dw.max()) if pc.size else 0.0
