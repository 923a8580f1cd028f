"""CPU restatement of the reference's proxy-texture mip chain (upload_proxy_texture, proxy.rs:513-554), float64 arithmetic on
the crate's f32 tap geometry.

Level n of the chain is image::imageops::resize(original, n, n, Lanczos3) followed by to_rgba32f (image 0.25).  For an 8- or
16-bit RGBA image (MAX = 255 / 65535):
  * (n, n) == (w, h): an exact copy, so the level is x / MAX;
  * otherwise a vertical pass (h -> n rows) kept unclamped in source units, then a horizontal pass (w -> n columns); each output
    is round_half_away_from_zero(clamp(t, 0, MAX)), divided by MAX in f32.
  * per axis (in -> out), in f32: ratio = in / out, sratio = max(ratio, 1), support = 3 sratio; output o has the centre
    c = (o + 0.5) ratio and the taps i in [left, right), left = clamp(floor(c - support), 0, in - 1),
    right = clamp(ceil(c + support), left + 1, in); weight L((i - (c - 0.5)) / sratio), normalised by the sum over the taps
    (the window is clipped at the image edges and renormalised, never replicated or wrapped).
  * L(x) = sinc(x) sinc(x / 3) for |x| < 3, else 0; sinc(t) = sin(pi t) / (pi t), sinc(0) = 1.
The channels are resampled independently (no premultiplication).

Here the window (left, count) and the centre c are computed in f32 exactly as the crate does; the weights, their
normalisation and both passes are float64.  `resize_level` returns the quantised level and the pre-rounding value t.
"""
import numpy as np

F32 = np.float32


def maxval(dtype):
    return float(np.iinfo(np.dtype(dtype)).max)


def lanczos3(x):
    x = np.asarray(x, np.float64)
    return np.where(np.abs(x) < 3.0, np.sinc(x) * np.sinc(x / 3.0), 0.0)


def axis_taps(n_in, n_out):
    """(left [n_out] int64, count [n_out] int64, weights [n_out, max count] float64 (zero past each count))."""
    ratio = F32(n_in) / F32(n_out)
    sratio = ratio if ratio >= F32(1.0) else F32(1.0)
    support = F32(3.0) * sratio
    c = (np.arange(n_out, dtype=F32) + F32(0.5)) * ratio
    left = np.clip(np.floor(c - support).astype(np.int64), 0, n_in - 1)
    right = np.clip(np.ceil(c + support).astype(np.int64), left + 1, n_in)
    count = right - left
    k = np.arange(int(count.max()))
    i = left[:, None] + k[None, :]
    cc = (c - F32(0.5)).astype(np.float64)
    w = np.where(k[None, :] < count[:, None], lanczos3((i - cc[:, None]) / np.float64(sratio)), 0.0)
    return left, count, w / w.sum(axis=1, keepdims=True)


def _gather(src, left, w, axis):
    """sum_k w[o, k] * src[left[o] + k] along `axis` (0: rows, 1: columns) -> float64."""
    out = 0.0
    n_in = src.shape[axis]
    for k in range(w.shape[1]):
        idx = np.minimum(left + k, n_in - 1)                 # past a count the weight is 0; keep the index in range
        taken = np.take(src, idx, axis=axis).astype(np.float64)
        wk = w[:, k][:, None, None] if axis == 0 else w[:, k][None, :, None]
        out = out + wk * taken
    return out


def resize_level(img, n, rows=None):
    """Level n (n x n) of the chain of img [h, w, 4] uint8 / uint16.  rows: the output rows to evaluate (all by default).
    Returns (level f32 [len(rows), n, 4], q integer codes, t float64 pre-rounding values in source units)."""
    img = np.asarray(img)
    h, w = img.shape[:2]
    mx = maxval(img.dtype)
    rows = np.arange(n) if rows is None else np.asarray(rows, np.int64)
    if (n, n) == (w, h):
        t = img[rows].astype(np.float64)
        q = img[rows].astype(np.int64)
    else:
        lv, _, wv = axis_taps(h, n)
        lh, _, wh = axis_taps(w, n)
        tmp = _gather(img, lv[rows], wv[rows], 0)            # [len(rows), w, 4], unclamped
        t = _gather(tmp, lh, wh, 1)                          # [len(rows), n, 4]
        q = quantise(t, mx)
    return (q.astype(F32) / F32(mx)), q, t


def quantise(t, mx):
    """clamp to [0, MAX], round half away from zero (FloatNearest)."""
    c = np.clip(t, 0.0, mx)
    return np.floor(c + 0.5).astype(np.int64)                # c >= 0: half away from zero == floor(c + 0.5)


def chain(img, tex_size):
    """The whole chain tex_size, tex_size / 2, ..., 1 as a list of f32 levels."""
    out, n = [], tex_size
    while n >= 1:
        out.append(resize_level(img, n)[0])
        n //= 2
    return out


def default_tex_size(width):
    """The largest power of two <= width, in integers."""
    return 1 << (int(width).bit_length() - 1)


def reference_max_size(width, log):
    """proxy.rs: max_size = 2^floor(ln(w) / ln(2)) evaluated in f32, with `log` the f32 natural log used."""
    q = F32(log(F32(width))) / F32(log(F32(2.0)))
    return 1 << int(np.floor(q))
