"""with_variant / OneOf (gswt_renderer_amd/csrc/gswt_variant.h), the one way a launch wrapper of libgswt_hip.so picks its kernel
instantiation, on the host: tools/with_variant_main.cpp built with the host compiler alone (the header needs nothing of HIP) and run once.

For the selectors (bool, bool, OneOf<0, 1, 2>, bool) every combination of runtime values must reach the lambda exactly once, with the
compile-time constants in the selectors' order, and an out-of-list OneOf value must land on the list's last alternative.  A swap of two
selectors is what would launch a kernel's SHD instantiation with a null map."""
import itertools
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_every_combination_lands_once_in_selector_order(tmp_path):
    exe = tmp_path / "with_variant"
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "gswt_renderer_amd", "csrc"),
           os.path.join(ROOT, "tools", "with_variant_main.cpp"), "-o", str(exe)]
    subprocess.run(cmd, check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0 and not out.stderr, out.stderr[-2000:]
    lines = out.stdout.splitlines()
    assert lines[-1].split() == ["in", "->"]                                       # no selector: the lambda ran, once
    calls = {}
    for line in lines[:-1]:
        left, right = line.split("->")
        key, got = tuple(int(t) for t in left.split()[1:]), tuple(int(t) for t in right.split())
        assert len(key) == 4 and len(got) == 4, line
        calls.setdefault(key, []).append(got)
    values = (0, 1, 2, -1, 3, 7)
    want = set(itertools.product((0, 1), (0, 1), values, (0, 1)))
    assert set(calls) == want and len(lines) - 1 == len(want) == 48                # every combination, none twice
    landed = set()
    for (a, b, v, c), got in calls.items():
        assert got == [(a, b, v if v in (0, 1, 2) else 2, c)], ((a, b, v, c), got)   # selector order; out of list -> the last alternative
        landed.add(got[0])
    assert landed == set(itertools.product((0, 1), (0, 1), (0, 1, 2), (0, 1)))     # all 24 instantiations are reachable
