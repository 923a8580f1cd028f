"""The 4:2:0 video formats (GSWT_VIDEO_NV12 / GSWT_VIDEO_I420, include/gswt_hip.h) on the test side: the header's definition in numpy
float32, operation for operation -- every intermediate is a binary32 array, so numpy rounds each product, sum and difference once, as the
kernel's unfused operations do --, and a float64 evaluation of BT.709 (limited range, block-mean chroma) that shares nothing with it but
the standard's constants: the independent bound of the float32 definition (one code)."""
import numpy as np

_F = np.float32
KR, KG, KB = 0.2126, 0.7152, 0.0722            # BT.709 luma coefficients
CB_DIV, CR_DIV = 1.8556, 1.5748                # 2 (1 - KB), 2 (1 - KR)


def _even(img):
    img = np.asarray(img)
    assert img.ndim == 3 and img.shape[2] >= 3 and img.shape[0] % 2 == 0 and img.shape[1] % 2 == 0, img.shape
    return img


def _clamp01(x):
    """fminf(fmaxf(x, 0), 1): a NaN becomes 0 (fmaxf returns its other argument)."""
    with np.errstate(invalid="ignore"):
        return np.fmin(np.fmax(np.asarray(x, dtype=_F), _F(0.0)), _F(1.0))


def _rint_u8(x):
    return np.rint(x).astype(np.uint8)          # np.rint: half to even, as v_rndne_f32


def _samples(img):
    """(Y, Cb, Cr) of a float32 image [rows, w, >= 3], rows and w even: uint8 [rows, w], [rows / 2, w / 2], [rows / 2, w / 2]."""
    img = _even(img)
    assert img.dtype == np.float32
    r, g, b = _clamp01(img[..., 0]), _clamp01(img[..., 1]), _clamp01(img[..., 2])
    yl = (_F(KR) * r + _F(KG) * g) + _F(KB) * b
    y = _rint_u8(_F(16.0) + _F(219.0) * yl)
    out = [y]
    for c, div in ((b, CB_DIV), (r, CR_DIV)):
        d = (c - yl) * _F(1.0 / div)                                   # fl(1 / div): the double quotient rounded to binary32
        m = ((d[0::2, 0::2] + d[0::2, 1::2]) + (d[1::2, 0::2] + d[1::2, 1::2])) * _F(0.25)
        out.append(_rint_u8(_F(128.0) + _F(224.0) * m))
    assert all(a.dtype == np.uint8 for a in out)
    return tuple(out)


def i420(img):
    """(y, cb, cr): the planes of GSWT_VIDEO_I420 of the RGBA f32 image img."""
    return _samples(img)


def nv12(img):
    """(y, cbcr): the planes of GSWT_VIDEO_NV12, cbcr [rows / 2, w / 2, 2] with Cb first."""
    y, cb, cr = _samples(img)
    return y, np.stack([cb, cr], axis=-1)


def nv12_bytes(img):
    """The NV12 image as the flat byte string the library writes (planes back to back)."""
    y, cbcr = nv12(img)
    return np.concatenate([y.reshape(-1), cbcr.reshape(-1)])


def i420_bytes(img):
    y, cb, cr = i420(img)
    return np.concatenate([y.reshape(-1), cb.reshape(-1), cr.reshape(-1)])


def yuv_f64(img):
    """BT.709 limited-range (Y, Cb, Cr) BEFORE rounding, in float64: real-valued codes, Y [rows, w], Cb / Cr [rows / 2, w / 2] as the mean
    of the block's four chroma samples.  NaN counts as 0, +-inf clamp to 1 / 0."""
    img = _even(img)
    x = np.nan_to_num(np.asarray(img[..., :3], dtype=np.float64), nan=0.0, posinf=1.0, neginf=0.0)
    x = np.clip(x, 0.0, 1.0)
    yl = KR * x[..., 0] + KG * x[..., 1] + KB * x[..., 2]
    cb, cr = (x[..., 2] - yl) / CB_DIV, (x[..., 0] - yl) / CR_DIV
    mean = lambda c: c.reshape(c.shape[0] // 2, 2, c.shape[1] // 2, 2).mean(axis=(1, 3))
    return 16.0 + 219.0 * yl, 128.0 + 224.0 * mean(cb), 128.0 + 224.0 * mean(cr)
