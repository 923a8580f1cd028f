"""bench.py's command line without a GPU: the options the driver passes exist, and the documented ones parse."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_help_lists_the_contract_options():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    for opt in ("--gpus", "--steps", "--warmup", "--workload", "--mode", "--graph", "--no-graph", "--segment", "--in-flight", "--device-worker",
                "--timing-every", "--static-steps", "--no-cpu-baseline", "--dump-outputs"):
        assert opt in r.stdout, opt


def test_run_scripts_reference_existing_tools():
    for script in ("tools/profile_c3.sh", "tools/run_bench_lines.sh", "tools/run_round_check.sh"):
        text = open(os.path.join(ROOT, script)).read()
        for tok in text.replace("$", " ").split():
            if tok.startswith("tools/") and tok.endswith(".py"):
                assert os.path.exists(os.path.join(ROOT, tok)), (script, tok)


def test_auto_segment_fills_the_chip_and_keeps_dense_frames_long():
    """bench.py's rule for GSWT_OPT_SEGMENT (pairs per compositor work item): the dense-frame length (4 x pairs per screen tile, at least the
    library's default) unless that leaves fewer than ~2 048 work items -- one rank's band of a sharded frame."""
    sys.path.insert(0, ROOT)
    import bench
    from gswt_renderer_amd import _lib as L
    assert L.GSWT_DEFAULT_SEGMENT == 1536
    cases = {  # name: (pairs, screen tiles) -> segment
        "c3": (2.66e6, 8160, 1536), "c3d": (8.2e6, 8160, 4096), "c5": (21.4e6, 32400, 2816), "c3s": (5.3e6, 8160, 2816),
        "one of 8 column bands of c3": (345e3, 1020, 256), "one of 4": (690e3, 2040, 512), "one of 2": (1.35e6, 4080, 768), "c1": (3e4, 1200, 256),
    }
    for name, (pairs, tiles, want) in cases.items():
        seg = bench.auto_segment(pairs / tiles, pairs)
        assert seg == want and seg % 256 == 0 and 256 <= seg <= 4096, (name, seg, want)
    for p in (1.0, 2047.0, 2049.0 * 256, 1e9):
        for ppt in (0.0, 1.0, 1e4):
            seg = bench.auto_segment(ppt, p)
            assert seg % 256 == 0 and 256 <= seg <= 4096
    # the options the round's A/B lines use exist
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True, timeout=120)
    for opt in ("--order", "--depth-sort", "--item-order", "--no-chunk-cull", "--vertex-stage", "--composite"):
        assert opt in r.stdout, opt


def test_dump_outputs_writes_float_arrays_within_the_size_limit(tmp_path):
    """bench.py --dump-outputs: a small image is written whole, a large one as a fixed seeded pixel sample (with the flat pixel indices),
    both with the frame counts, all float32 / float64 and 64 MB at most."""
    import numpy as np
    sys.path.insert(0, ROOT)
    import bench
    counts = {"n_draws": 3, "n_instanced": 70, "n_visible": 50, "n_pairs": 900}
    small = np.random.default_rng(1).random((24, 32, 4), dtype=np.float32)
    shapes = bench.dump_outputs(str(tmp_path / "small"), small, counts)
    assert shapes == {"image": [24, 32, 4], "frame_counts": [4]}
    assert np.array_equal(np.load(tmp_path / "small" / "image.npy"), small)
    fc = np.load(tmp_path / "small" / "frame_counts.npy")
    assert fc.dtype == np.float64 and fc.tolist() == [3.0, 70.0, 50.0, 900.0]

    big = np.zeros((2160, 3840, 4), dtype=np.float32)                # c5's frame: 133 MB
    big[..., 0] = np.arange(2160 * 3840, dtype=np.float32).reshape(2160, 3840)
    written = []
    for k in range(2):
        d = tmp_path / f"big{k}"
        bench.dump_outputs(str(d), big, counts)
        files = sorted(os.listdir(d))
        assert files == ["frame_counts.npy", "image_sample.npy", "image_sample_pixel.npy"]
        assert sum(os.path.getsize(d / f) for f in files) <= 64 << 20
        written.append({f: np.load(d / f) for f in files})
    smp, pix = written[0]["image_sample.npy"], written[0]["image_sample_pixel.npy"]
    assert smp.dtype == np.float32 and pix.dtype == np.float64 and smp.shape == (pix.shape[0], 4)
    assert np.all(np.diff(pix) > 0) and smp.shape[0] > 1_000_000
    assert np.array_equal(smp[:, 0], pix.astype(np.float32))       # the sample holds the pixels its indices name
    for f in written[0]:
        assert np.array_equal(written[0][f], written[1][f]), f       # the same sample every run
