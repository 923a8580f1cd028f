"""tests/frame_outputs.py's pure helpers on known answers: `same_planes` notices a wrong shape, type, byte or plane count;
`hostile_bg` holds what its name promises and is a function of its seed; `split_guard` cuts where it is told; a format's
`zero_pad` zeroes bytes, not pixels."""
import numpy as np
import pytest

from tests import frame_outputs as FO


def _planes():
    return (np.arange(48, dtype=np.uint8).reshape(6, 8), np.arange(24, dtype=np.uint8).reshape(3, 4, 2) + 100)


def test_same_planes_accepts_equal_planes():
    assert FO.same_planes(_planes(), _planes()) and FO.same_planes(list(_planes()), _planes())
    assert FO.same_image(_planes()[0], _planes()[0])


WRONG = {
    "shape": lambda y, c: (y.reshape(8, 6), c),
    "chroma_shape": lambda y, c: (y, c.reshape(3, 8)),
    "dtype": lambda y, c: (y.astype(np.int8), c),
    "wider_dtype": lambda y, c: (y, c.astype(np.uint16)),
    "last_byte": lambda y, c: (y, np.where(np.arange(24).reshape(3, 4, 2) == 23, 0, c).astype(np.uint8)),
    "first_byte": lambda y, c: (np.where(np.arange(48).reshape(6, 8) == 0, 1, y).astype(np.uint8), c),
    "a_plane_short": lambda y, c: (y,),
    "a_plane_more": lambda y, c: (y, c, c),
}


@pytest.mark.parametrize("what", list(WRONG))
def test_same_planes_rejects(what):
    with pytest.raises(AssertionError):
        FO.same_planes(WRONG[what](*_planes()), _planes())


def test_same_image_rejects_one_wrong_byte_and_a_float_image():
    a = np.zeros((4, 5, 4), np.uint8)
    b = a.copy()
    b[3, 4, 3] = 1
    with pytest.raises(AssertionError):
        FO.same_image(b, a)
    with pytest.raises(AssertionError):
        FO.same_image(a.astype(np.float32), a)


def test_hostile_bg_is_hostile_and_a_function_of_its_seed():
    bg, depth = FO.hostile_bg(40, 24)
    assert bg.shape == (24, 40, 4) and bg.dtype == np.float32 and depth.shape == (24, 40) and depth.dtype == np.float32
    assert np.isnan(bg).sum() == 16 and (bg == np.inf).sum() == 16 and (bg == -np.inf).sum() == 16
    finite = bg[np.isfinite(bg)]
    assert (finite < 0).any() and (finite > 1).any() and ((finite >= 0) & (finite <= 1)).any()
    assert (bg == np.float32(1.0 + 1e-7)).sum() >= 16              # just above 1: clamps to code 255, not past it
    assert depth.min() >= 0.0 and depth.max() <= 1.0
    again, depth_again = FO.hostile_bg(40, 24)
    assert FO.FM.same(bg, again) and FO.FM.same(depth, depth_again)
    other, _ = FO.hostile_bg(40, 24, seed=3)
    assert not FO.FM.same(bg, other)
    assert FO.FM.same(FO.bg_depth(40, 24), FO.bg_depth(40, 24)) and FO.bg_depth(40, 24).min() >= 0.99


def test_split_guard_on_ten_bytes():
    buf = np.arange(10, dtype=np.uint8)
    image, guard = FO.split_guard(buf, 6)
    assert image.tolist() == [0, 1, 2, 3, 4, 5] and guard.tolist() == [6, 7, 8, 9]
    assert FO.split_guard(buf, 10)[1].size == 0 and FO.split_guard(buf, 0)[0].size == 0
    for bad in (11, -1):
        with pytest.raises(AssertionError):
            FO.split_guard(buf, bad)
    with pytest.raises(AssertionError):
        FO.split_guard(buf.reshape(2, 5), 4)


def test_formats_know_their_sizes_and_pad_with_zero_bytes():
    assert [FO.BY_ID[f].name for f in sorted(FO.BY_ID)] == ["f32", "rgba8", "bgra8", "nv12", "i420"]
    assert (FO.F32.nbytes(6, 8), FO.RGBA8.nbytes(6, 8), FO.BGRA8.nbytes(6, 8), FO.NV12.nbytes(6, 8), FO.I420.nbytes(6, 8)) == (768, 192, 192, 72, 72)
    f32 = np.random.default_rng(0).uniform(0.2, 1.0, size=(6, 8, 4)).astype(np.float32)
    for cf in (FO.RGBA8, FO.BGRA8, FO.NV12, FO.I420):
        frame = cf.ref(f32)
        cf.check_shape(frame, 6, 8)
        assert cf.bytes_of(frame).size == cf.nbytes(6, 8) and np.array_equal(cf.bytes_of(frame), cf.flat(f32))
        assert cf.same(cf.unflat(cf.flat(f32), 6, 8), frame)
        padded = cf.zero_pad(frame, 4, 6)
        planes = padded if isinstance(padded, list) else [padded]
        assert not planes[0][4:].any() and not planes[0][:, 6:].any() and planes[0][:4, :6].all()
        assert all(not p[2:].any() and not p[:, 3:].any() and p[:2, :3].all() for p in planes[1:])
        assert cf.same(cf.zero_pad(frame, 6, 8), frame)
    with pytest.raises(AssertionError):
        FO.NV12.zero_pad(FO.NV12.ref(f32), 3, 8)                   # a video shard owns whole chroma samples
