"""The frame's device bookkeeping as gswt_renderer_amd/csrc/gswt_frame_layout.h lays it out -- the counter block, the radix sort's count record
and workspace, k_project's super-group sums, the live-chunk table and the per-tile range words -- on the host: tools/frame_layout_main.cpp built
with the host compiler alone (the header needs nothing of HIP) and run once.

The known answers are the formulae the kernels, launch_sort, plan_frame_buffers and the test hooks each wrote out by hand before the header
existed: a layout that moves a word here moves it under every kernel of the frame chain."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def layout(tmp_path_factory):
    exe = tmp_path_factory.mktemp("frame_layout") / "frame_layout"
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "gswt_renderer_amd", "csrc"),
           os.path.join(ROOT, "tools", "frame_layout_main.cpp"), "-o", str(exe)]
    subprocess.run(cmd, check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0 and not out.stderr, out.stderr[-2000:]
    rows = {}
    for line in out.stdout.splitlines():
        tag, *fields = line.split()
        rows.setdefault(tag, []).append({k: int(v) for k, v in (f.split("=") for f in fields)})
    return rows


def test_counter_block_word_map(layout):
    (c,) = layout["counters"]
    # 64-bit words [0] visible, [1] pairs, [2] lo / hi passes needed / longest tile list, [3] re-run, [4] longest live list, [5] key range
    assert c == dict(size=64, n_visible=0, n_pairs=8, depth_passes_needed=16, max_tile_len=20, rerun=24, live_longest=32, krange=40, reserved=48,
                     result_size=40, result_words64=5, counter_words=16)
    (r,) = layout["result"]                                  # the word-by-word copy k_combine makes carries every result field
    assert r == dict(n_visible=1, n_pairs=123456789012, depth_passes_needed=3, max_tile_len=4, rerun=7, live_longest=5)


def test_sort_count_is_the_view_of_a_counter_block(layout):
    (s,) = layout["sortcount"]
    assert (s["size"], s["n"], s["refused"]) == (32, 0, 16)  # the 16-byte gap is the device contract
    assert (s["view_n"], s["view_refused"]) == (123456789012, 7)      # n_pairs / rerun of the block, read through the view
    assert (s["staged_n"], s["staged_refused"], s["plain_n"], s["plain_refused"]) == (42, 1, 43, 0)


RADIX = {(1, 1): (768, 512), (4096, 8): (768, 512), (4097, 9): (2048, 1024), (131072, 32): (35840, 3072), (131073, 16): (18432, 1536)}


def test_radix_workspace(layout):
    rows = {(r["n_cap"], r["key_bits"]): r for r in layout["radix"]}
    for key, (total, zero) in RADIX.items():
        r = rows[key]
        assert (r["total"], r["zero"]) == (total, zero), key
        nblk, nsup, passes = r["nblk"], r["nsup"], r["passes"]
        assert nblk == (key[0] + 4095) // 4096 and nsup == nblk // 32 + 1 and passes == (key[1] + 7) // 8, key
        regions = []
        for p in range(passes):
            assert r[f"gsup{p}"] == p * (256 * nsup + 256), (key, p)
            assert r[f"gtot{p}"] == r[f"gsup{p}"] + 256 * nsup, (key, p)
            assert r[f"ghist{p}"] == zero + p * 256 * nblk, (key, p)
            regions += [(r[f"gsup{p}"], 256 * nsup), (r[f"gtot{p}"], 256), (r[f"ghist{p}"], 256 * nblk)]
        at = 0
        for start, words in sorted(regions):                 # the regions tile [0, total): no gap, no overlap
            assert start == at, (key, start, at)
            at += words
        assert at == total, key
        # the zeroed part is exactly the group rows and digit totals: every per-workgroup row lies behind it
        assert all(r[f"gtot{p}"] + 256 <= zero <= r[f"ghist{p}"] for p in range(passes)), key
    assert rows[(131073, 16)]["nblk"] == 33 and rows[(131073, 16)]["nsup"] == 2
    none = rows[(131073, 0)]                                 # no key bits (a frame without global depth passes): no passes, no words
    assert (none["passes"], none["zero"], none["total"]) == (0, 0, 0)


def test_super_sums(layout):
    rows = {r["n_chunks"]: r for r in layout["super"]}
    assert (rows[0]["n_super"], rows[0]["words"]) == (1, 33)
    assert (rows[255]["n_super"], rows[255]["words"]) == (1, 33)
    assert (rows[256]["n_super"], rows[256]["words"]) == (2, 66)
    assert (rows[1000]["n_super"], rows[1000]["words"], rows[1000]["super_of_last"]) == (4, 132, 3)
    for r in rows.values():
        for j in (0, 1, 5):
            assert r[f"pair{j}"] == 16 * j and r[f"visible{j}"] == 16 * (r["n_super"] + j) and r[f"prefix{j}"] == 32 * r["n_super"] + j, (r, j)


def test_live_table(layout):
    (t,) = layout["live"]
    # rows 0..7 the per-XCD counts, rows 8..15 k_totals' copy for k_emit, 16 words (a cache line) per row
    assert t == dict(count0=0, count3=48, copy0=128, copy3=176, words=256, lists=8)


def test_tile_range_codec(layout):
    rows = {(r["start"], r["end"]): r for r in layout["range"]}
    inv = lambda v: v ^ 0xFFFFFFFF
    r = rows[(3, 7)]
    assert (r["x"], r["y"], r["dec_start"], r["dec_end"], r["start_word"]) == (inv(3), 7, 3, 7, inv(3))
    for empty in ((0, 0), (5, 5)):                           # a tile without pairs is (0, 0) and reads as start 0
        r = rows[empty]
        assert (r["x"], r["y"], r["dec_start"], r["dec_end"]) == (0, 0, 0, 0), empty
    r = rows[(0, 1)]
    assert (r["x"], r["y"], r["dec_start"], r["dec_end"]) == (0xFFFFFFFF, 1, 0, 1)
    r = rows[(0xFFFFFF00, 0xFFFFFFFF)]
    assert (r["x"], r["y"], r["dec_start"], r["dec_end"]) == (0xFF, 0xFFFFFFFF, 0xFFFFFF00, 0xFFFFFFFF)
    (k,) = layout["krange"]
    assert k == dict(min_word_of_9=inv(9), back=9)
