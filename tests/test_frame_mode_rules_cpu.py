"""The two pure rules behind the frame modes (gswt_renderer_amd/csrc/gswt_frame_modes.h), on the host: tools/frame_modes_main.cpp built
with the host compiler alone (the header needs nothing of HIP) and run once.

free_version, over every state of (current version, the five frame slots' versions), each in -1 .. 6: a version is always found, it is
never the current one nor a slot's, and it is the lowest such index.  project_modes, over all 64 inputs (strict_vs, ortho, filter on,
atmosphere on, styles on, shadows on): strict = strict_vs or ortho, every other mode = its input and strict, ortho passes through, and
all 32 instantiations of the strict sequence are reached.  The program checks; this test runs it and reads its counts."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_free_version_and_project_modes_hold_over_every_input(tmp_path):
    exe = tmp_path / "frame_modes"
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "gswt_renderer_amd", "csrc"),
           os.path.join(ROOT, "tools", "frame_modes_main.cpp"), "-o", str(exe)]
    subprocess.run(cmd, check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0 and not out.stderr, (out.stdout[-2000:], out.stderr[-2000:])
    lines = out.stdout.splitlines()
    assert not [ln for ln in lines if ln.startswith("FAIL")], lines[:20]
    assert lines == ["free_version: %d states" % 8 ** 6, "project_modes: 64 inputs, 32 strict outputs"]
