#!/usr/bin/env python3
"""Compares two gfx950 assembly listings function by function, for changes that add a template parameter or a trailing kernel argument
and claim to leave the existing instantiations' code alone (profiles/clip_volumes_ab.txt).

    hipcc <Makefile HIPFLAGS> --cuda-device-only -S gswt_kernels.hip -o parent.s      (at the parent commit)
    hipcc <Makefile HIPFLAGS> --cuda-device-only -S gswt_kernels.hip -o head.s
    python tools/asm_function_diff.py parent.s head.s --rename 'REGEX=REPLACEMENT' ...

A function's text is every line from its label to its kernel descriptor (or, for a device function, its `.Lfunc_end` label):
instructions, local labels and the compiler's own comments.
Each --rename is applied to the HEAD's symbol names and text (a new template argument in its off state, a new trailing argument type),
after which a head function is matched with the parent function of the same name; local labels lose the function's ordinal
(`.LBB12_3` -> `.LBB_3`) and the padding in front of a comment with it (the ordinal's digits shift the comment's column).  Prints how
many functions are identical, which differ (with the first differing line), which exist on one side only, and exits 1 when a matched function differs or a parent function has no counterpart.  The `.amdhsa_*` descriptor and the
metadata behind the functions are not compared: a new trailing kernel argument grows the kernarg segment of every instantiation.
"""
import argparse
import re
import sys


def functions(path, renames):
    out, name, body = {}, None, []
    label = re.compile(r"^(_Z\w+|\.L_Z\w+|[A-Za-z_]\w*):\s*(;.*)?$")
    for line in open(path):
        line = line.rstrip("\n")
        if name is None:
            m = label.match(line)
            if m and not m.group(1).startswith((".LBB", "__hip_cuid_")):      # (the per-file marker carries a hash of the source)
                name, body = m.group(1), []
            continue
        if line.startswith(".Lfunc_end") or line.lstrip().startswith((".amdhsa_kernel", ".section")):
            text = "\n".join(body)
            for pat, rep in renames:
                name, text = pat.sub(rep, name), pat.sub(rep, text)
            out[name] = re.sub(r"[ \t]+;", " ;", re.sub(r"BB\d+_(?=\d)", "BB_", text)).split("\n")
            name = None
            continue
        body.append(line)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("parent")
    ap.add_argument("head")
    ap.add_argument("--rename", action="append", default=[], help="REGEX=REPLACEMENT on the head's names and text")
    a = ap.parse_args()
    renames = [(re.compile(r.split("=", 1)[0]), r.split("=", 1)[1]) for r in a.rename]
    P, H = functions(a.parent, []), functions(a.head, renames)
    same = [n for n in P if n in H and P[n] == H[n]]
    diff = [n for n in P if n in H and P[n] != H[n]]
    gone = [n for n in P if n not in H]
    new = [n for n in H if n not in P]
    print(f"parent: {len(P)} functions, head: {len(H)}; identical: {len(same)}, different: {len(diff)}, "
          f"parent only: {len(gone)}, head only: {len(new)}")
    for n in diff:
        k = next((i for i, (x, y) in enumerate(zip(P[n], H[n])) if x != y), min(len(P[n]), len(H[n])))
        print(f"DIFFERENT {n}: {len(P[n])} / {len(H[n])} lines, first at {k}:\n  - {P[n][k] if k < len(P[n]) else ''}\n  + {H[n][k] if k < len(H[n]) else ''}")
    for n in gone:
        print(f"PARENT ONLY {n}")
    return 1 if diff or gone else 0


if __name__ == "__main__":
    sys.exit(main())
