"""tests/frame_modes.py's pure helpers on known answers: the two shard assemblers rebuild a labelled frame whose last screen tile and
last band are partial, and notice one altered element; `same` and `bits_equal` compare bytes, not values.  This is what "byte-identical"
means in the GPU battery of the per-frame modes."""
import numpy as np
import pytest

from tests import frame_modes as FM

H_, W_ = 40, 36            # 16-pixel tiles: 2.5 tile rows, 2.25 tile columns


def _labelled():
    """A frame (colour, depth, pick) in which every element of every output has a value of its own."""
    out = FM.new_outputs(H_, W_)
    assert [o.shape for o in out] == [(H_, W_, 4), (H_, W_), (H_, W_)] and not any(FM._raw(o).any() for o in out)
    out[0][...] = np.arange(H_ * W_ * 4, dtype=np.float32).reshape(H_, W_, 4) + 1.0
    out[1][...] = -1.0 - np.arange(H_ * W_, dtype=np.float32).reshape(H_, W_)
    ids = np.arange(H_ * W_, dtype=np.uint32).reshape(H_, W_)
    out[2]["map_index"], out[2]["entry"], out[2]["depth"], out[2]["weight"] = ids + 1, ids * 3 + 7, out[1] * 0.5, out[1] * 0.25 - 2.0
    return out


def _row_shards(frame, n):
    """What rank r of n renders: its tile rows one below the other, padded with rows of another value to the largest rank's height."""
    tile_rows = (H_ + 15) // 16
    rows = 16 * ((tile_rows + n - 1) // n)
    parts = []
    for r in range(n):
        part = [np.full((rows,) + a.shape[1:], 9, a.dtype) if a.dtype.names is None else np.zeros((rows,) + a.shape[1:], a.dtype) for a in frame]
        for k, ty in enumerate(range(r, tile_rows, n)):
            for dst, src in zip(part, frame):
                got = src[ty * 16:ty * 16 + 16]
                dst[k * 16:k * 16 + got.shape[0]] = got
        parts.append(part)
    return parts


def _column_bands(frame, band_w, n):
    parts = []
    for r in range(n):
        part = [np.full((H_, band_w) + a.shape[2:], 9, a.dtype) if a.dtype.names is None else np.zeros((H_, band_w) + a.shape[2:], a.dtype) for a in frame]
        for dst, src in zip(part, frame):
            got = src[:, r * band_w:(r + 1) * band_w]
            dst[:, :got.shape[1]] = got
        parts.append(part)
    return parts


def _equal(a, b):
    return all(FM.same(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("n", [2, 3, 5])
def test_row_shards_rebuild_the_frame(n):
    frame = _labelled()
    parts = _row_shards(frame, n)
    assert _equal(FM.assemble_row_shards(parts, H_, n), frame)
    # one element of one rank's part: the last row the frame has, in the partial tile row
    r = ((H_ + 15) // 16 - 1) % n
    k = len(range(r, (H_ + 15) // 16, n)) - 1
    for which, edit in ((0, lambda a: a.__setitem__((k * 16 + H_ % 16 - 1, W_ - 1, 3), -5.0)), (1, lambda a: a.__setitem__((k * 16 + H_ % 16 - 1, 0), 5.0)),
                        (2, lambda a: a["entry"].__setitem__((k * 16, 17), 0xFFFFFFFF))):
        parts = _row_shards(frame, n)
        edit(parts[r][which])
        got = FM.assemble_row_shards(parts, H_, n)
        assert [FM.same(x, y) for x, y in zip(got, frame)] == [i != which for i in range(3)], which


@pytest.mark.parametrize("n", [2, 3, 5])
def test_column_bands_rebuild_the_frame(n):
    frame = _labelled()
    band_w = {2: 32, 3: 16, 5: 8}[n]                          # (the last band: 4 columns of 32, 4 of 16, 4 of 8)
    assert (n - 1) * band_w < W_ < n * band_w
    parts = _column_bands(frame, band_w, n)
    assert _equal(FM.assemble_column_bands(parts, W_, band_w), frame)
    last = W_ - (n - 1) * band_w - 1                           # the frame's last column, in the partial band
    for which, edit in ((0, lambda a: a.__setitem__((H_ - 1, last, 0), -5.0)), (1, lambda a: a.__setitem__((0, last), 5.0)),
                        (2, lambda a: a["weight"].__setitem__((H_ // 2, 0), 0.5))):
        parts = _column_bands(frame, band_w, n)
        edit(parts[n - 1][which])
        got = FM.assemble_column_bands(parts, W_, band_w)
        assert [FM.same(x, y) for x, y in zip(got, frame)] == [i != which for i in range(3)], which


def test_padding_is_left_out():
    """What a rank holds beyond its share -- the rows under a partial tile row, the columns right of the partial band -- does not reach the frame."""
    frame = _labelled()
    parts = _row_shards(frame, 2)
    parts[0][0][16 + H_ % 16:] = -77.0                         # rank 0 of 2: tile rows 0 and 2, the second one 8 rows high
    assert _equal(FM.assemble_row_shards(parts, H_, 2), frame)
    parts = _column_bands(frame, 16, 3)
    parts[2][1][:, W_ - 32:] = -77.0
    assert _equal(FM.assemble_column_bands(parts, W_, 16), frame)


def _f32(bits):
    return np.array(bits, np.uint32).view(np.float32)


def test_same_compares_bytes():
    zero, minus_zero = _f32([0x00000000]), _f32([0x80000000])
    assert zero[0] == minus_zero[0] and not FM.same(zero, minus_zero) and FM.same(minus_zero, minus_zero.copy())
    nan_a, nan_b = _f32([0x7FC00000]), _f32([0x7FC00001])
    assert np.isnan(nan_a[0]) and np.isnan(nan_b[0])
    assert FM.same(nan_a, nan_a.copy()) and not FM.same(nan_a, nan_b)            # (a NaN equals itself here, unlike ==)
    # ... of any dtype and layout: a pick record, a view that is not contiguous
    a, b = FM.new_outputs(2, 3)[2], FM.new_outputs(2, 3)[2]
    assert FM.same(a, b)
    b["depth"][1, 2] = minus_zero[0]
    assert not FM.same(a, b) and (a["depth"] == b["depth"]).all()
    grid = np.arange(12, dtype=np.float32).reshape(3, 4)
    assert FM.same(grid[:, ::2], np.array([[0, 2], [4, 6], [8, 10]], np.float32)) and not FM.same(grid[:, ::2], grid[:, 1::2])
    assert not FM.same(np.zeros(4, np.float32), np.zeros(5, np.float32))


def test_bits_equal_compares_bits():
    a = _f32([0x00000000, 0x7FC00000, 0x3F800000])
    assert FM.bits_equal(a, a.copy())
    assert not FM.bits_equal(a, _f32([0x80000000, 0x7FC00000, 0x3F800000]))      # -0.0 == 0.0, other bits
    assert not FM.bits_equal(a, _f32([0x00000000, 0x7FC00001, 0x3F800000]))      # another NaN payload
    assert not np.array_equal(a, a.copy())                                        # (== would call the equal arrays different: NaN)
    cols = np.stack([a, a], 1)
    assert FM.bits_equal(cols[:, 0], a) and not FM.bits_equal(a, a[:2])
