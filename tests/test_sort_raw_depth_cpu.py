"""The C oracle's Scene::sort_raw_depth_vec (orc.sort_raw_depth_vec, which tests/test_merge_groups_gpu.py holds the device's merged
lists to) and libgswt_host's copy of it, against a plain-Python restatement of scene.rs:655-698 on the inputs where it is easy to
get wrong: equal depths (max == min: 0 * inf = NaN, which `as i32` makes 0), negative depths, depths at INT32_MIN / INT32_MAX, and
spans beyond 2^31 - 1, where Rust's release-build i32 subtraction wraps."""
import numpy as np
import pytest

from oracle import gswt_oracle as orc

I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1


def _wrap_i32(v):
    v &= 0xFFFFFFFF
    return v - 2 ** 32 if v >= 2 ** 31 else v


def _f32_as_i32(v):
    """Rust's saturating `f32 as i32`: NaN -> 0."""
    if np.isnan(v):
        return 0
    if v >= 2.0 ** 31:
        return I32_MAX
    if v <= -2.0 ** 31:
        return I32_MIN
    return int(v)


def rust_sort_raw_depth_vec(vecs):
    """scene.rs:655-698 statement by statement -> [(segment, index)]."""
    cat, displ = [], [0]
    for v in vecs:
        cat += [int(x) for x in v]
        displ.append(len(cat))
    mn, mx = min(cat), max(cat)
    size16 = 65536
    with np.errstate(all="ignore"):
        depth_inv = np.float32(size16 - 1) / np.float32(_wrap_i32(mx - mn))          # (max - min) as f32, f32 division
        bucket = []
        for d in cat:
            v = np.floor(np.float32(_wrap_i32(d - mn)) * depth_inv)                 # f32 product, floor, as i32
            bucket.append(min(max(_f32_as_i32(v), 0), size16 - 1))
    counts = [0] * size16
    for b in bucket:
        counts[b] += 1
    starts = [0] * size16
    for i in range(1, size16):
        starts[i] = starts[i - 1] + counts[i - 1]
    out = [None] * len(cat)
    for s in range(len(vecs)):
        for i in range(displ[s], displ[s + 1]):
            out[starts[bucket[i]]] = (s, i - displ[s])
            starts[bucket[i]] += 1
    out.reverse()
    return out


def _cases():
    rng = np.random.default_rng(17)
    r = lambda lo, hi, n: rng.integers(lo, hi, n, endpoint=True).astype(np.int64)
    return {
        "single": [[42]],
        "all-equal": [[7] * 5, [7] * 3],
        "all-equal-min": [[I32_MIN] * 4],
        "all-equal-max": [[I32_MAX] * 2, [I32_MAX]],
        "negative": [r(-5000, -1, 300), r(-90000, -60000, 200)],
        "min-and-max": [[I32_MIN, 0, I32_MAX, -1, 1], [I32_MAX, I32_MIN]],
        "span-2^31-1": [[0, I32_MAX, 5, 2 ** 30], [I32_MAX - 1]],
        "span-2^31": [[-1, I32_MAX, 0], [2 ** 30]],
        "span-wraps": [r(-2 ** 30 - 100, -2 ** 30, 150), r(2 ** 30, 2 ** 30 + 100, 150), [0]],
        "random-full-range": [r(I32_MIN, I32_MAX, 700), r(I32_MIN, I32_MAX, 300)],
        "ties-and-empty-segment": [r(-3, 3, 400), [], r(-3, 3, 100)],
        "one-outlier": [[0] * 100 + [I32_MAX], r(0, 10, 50)],
        "many-per-bucket": [r(0, 40, 3000)],
    }


@pytest.mark.parametrize("name", list(_cases()))
def test_oracle_sort_raw_depth_matches_rust_restatement(name):
    vecs = _cases()[name]
    want = rust_sort_raw_depth_vec(vecs)
    seg, idx = orc.sort_raw_depth_vec([np.asarray(v, dtype=np.int64).astype(np.int32) for v in vecs])
    assert list(zip(seg.tolist(), idx.tolist())) == want, name


@pytest.mark.parametrize("name", list(_cases()))
def test_host_sort_raw_depth_matches_rust_restatement(name):
    from gswt_renderer_amd import host
    vecs = _cases()[name]
    want = rust_sort_raw_depth_vec(vecs)
    displ = np.concatenate([[0], np.cumsum([len(v) for v in vecs])])
    cat = np.concatenate([np.asarray(v, dtype=np.int64) for v in vecs]).astype(np.int32)
    got = [int(displ[s]) + i for s, i in want]
    assert host.sort_raw_depth(cat).tolist() == got, name


def test_restatement_on_hand_worked_cases():
    """The restatement itself, on answers worked out by hand."""
    # depth_inv = 65535 / 8: buckets 0, 65535, 32767 (3 * 8191.875 floors to 24575 for d = 3); stable scatter then reverse
    assert rust_sort_raw_depth_vec([[0, 8, 3]]) == [(0, 1), (0, 2), (0, 0)]
    # max == min: every bucket is 0 (NaN -> 0); the stable order reversed
    assert rust_sort_raw_depth_vec([[5, 5], [5]]) == [(1, 0), (0, 1), (0, 0)]
    # span 2^32 - 1 wraps to -1: depth_inv = -65535; d - min wraps to -1 for INT32_MAX, giving bucket 65535; 0 -> 2^31 wraps to
    # -2^31 -> +2^31 * 65535 -> saturates to INT32_MAX -> 65535 as well; INT32_MIN -> 0
    assert rust_sort_raw_depth_vec([[I32_MAX, I32_MIN, 0]]) == [(0, 2), (0, 0), (0, 1)]
