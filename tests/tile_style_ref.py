"""The tile-instance styles of include/gswt_hip.h (gswt_set_tile_styles) restated in np.float32, one rounding per written operator,
over the records of the unstyled frame and a per-entry cell id -- `tile.map_index` for a static draw, the draw's `map_id` array for a
merged one (tests/pick_ref.identities).

    hide  s.dim == 255            the splat is not visible
    dim   0 < s.dim < 255         a_s = (float)(255 - s.dim) / 255.0f;  alpha = alpha * a_s
    tint  s.tint_strength > 0     k = (float)s.tint_strength / 255.0f;  tc = (float)s.tint[c] / 255.0f
                                  c_t = c * (1.0f - k) + tc * k;  byte' = (uint32_t)rintf(fminf(fmaxf(c_t, 0), 1) * 255.0f)
                                  and the record reports (float)byte' / 255.0f

Every operator is a correctly rounded binary32 operation, so dim and tint compare bit for bit with the GPU's records; with the fog on
the tinted floats `tinted_rgb` go through tests/atmosphere_ref.fog_codes_f64 instead (the fog's exponential is not correctly rounded)."""
import numpy as np

F32 = np.float32
NEUTRAL = (0, 0, 0, 0, 0)            # (r, g, b, strength, dim)


def entry(tint=(0, 0, 0), strength=0, dim=0):
    return (int(tint[0]), int(tint[1]), int(tint[2]), int(strength), int(dim))


HIDE = entry(dim=255)
# The main table of the issue, on case_plane (n_styles = 25); cells 9 and 14 are the two members of the case's one merged draw.
MAIN_N = 25
MAIN = {8: HIDE, 9: HIDE, 14: entry((0, 255, 64), 160, 96), 18: entry(dim=128), 19: entry((255, 64, 0), 160), 24: entry((10, 20, 250), 255)}


def entries(cells: dict, n: int) -> np.ndarray:
    """[n, 5] uint8 (r, g, b, strength, dim) of a {cell: entry} table of length n."""
    e = np.zeros((n, 5), np.uint8)
    for c, s in cells.items():
        e[c] = s
    return e


def pack(e: np.ndarray) -> bytes:
    """The table as gswt_set_tile_styles takes it: 8 bytes per cell, the last three zero."""
    out = np.zeros((e.shape[0], 8), np.uint8)
    out[:, :5] = e
    return out.tobytes()


def lookup(e: np.ndarray, cell_ids) -> np.ndarray:
    """The style of every instance: e[id], neutral for id >= len(e)."""
    ids = np.asarray(cell_ids, np.int64)
    out = np.zeros((ids.shape[0], 5), np.uint8)
    ok = ids < e.shape[0]
    out[ok] = e[ids[ok]]
    return out


def classes(sty):
    """(hidden, dimmed only, tinted, neutral) masks of per-instance styles."""
    hidden = sty[:, 4] == 255
    tinted = ~hidden & (sty[:, 3] > 0)
    dimmed = ~hidden & ~tinted & (sty[:, 4] > 0)
    return hidden, dimmed, tinted, ~(hidden | dimmed | tinted)


def requantise(c):
    """(bytes as float32 integers, the float colours the record reports) of float colours c, by the fog's own expression."""
    c = np.asarray(c, F32)
    b = np.rint((np.fmin(np.fmax(c, F32(0.0)), F32(1.0)) * F32(255.0)).astype(F32)).astype(F32)
    return b, (b / F32(255.0)).astype(F32)


def tinted_rgb(rgb, sty):
    """c_t per channel in binary32 (the unquantised tinted floats; rows without a tint are returned as they are)."""
    rgb = np.asarray(rgb, F32)
    k = (sty[:, 3].astype(F32) / F32(255.0)).astype(F32)[:, None]
    tc = (sty[:, :3].astype(F32) / F32(255.0)).astype(F32)
    ct = ((rgb * (F32(1.0) - k)).astype(F32) + (tc * k).astype(F32)).astype(F32)
    return np.where((sty[:, 3] > 0)[:, None], ct, rgb).astype(F32)


def dimmed_alpha(alpha, sty):
    """alpha * a_s in binary32 where 0 < dim < 255, alpha itself elsewhere."""
    alpha = np.asarray(alpha, F32)
    a_s = ((F32(255.0) - sty[:, 4].astype(F32)) / F32(255.0)).astype(F32)         # (float)(255 - dim): exact
    on = (sty[:, 4] > 0) & (sty[:, 4] < 255)
    return np.where(on, (alpha * a_s).astype(F32), alpha).astype(F32)


def apply(base_rgba, base_visible, sty):
    """(visible mask, rgba [n, 4] float32) of the styled records, without fog: what gswt_debug_read_projected reports."""
    base_rgba = np.asarray(base_rgba, F32)
    hidden, _, tinted, _ = classes(sty)
    out = base_rgba.copy()
    _, q = requantise(tinted_rgb(base_rgba[:, :3], sty))
    out[tinted, :3] = q[tinted]
    out[:, 3] = dimmed_alpha(base_rgba[:, 3], sty)
    return (np.asarray(base_visible) == 1) & ~hidden, out
