#!/usr/bin/env python3
"""Scene build: host path against the device path, wall time and bytes moved.

    host path : gswt_wang_new + gswt_upload_scene(preload) + gswt_upload_raw_depth(raw_depth_tables)
    rows path : gswt_wang_new_rows + gswt_upload_scene_rows (texture, raw depths, base lists, static arena on the device)

Tile-set construction (synth.make_tileset + gswt_tileset_set_vertices) is not timed.  Each call is timed with a host clock; the
upload calls return when the device has finished.  Each path gets a fresh GSWTRenderer (a context's scene buffers are allocated
inside the timed calls of both); the rows path runs once on a small set in a context of its own first (code-object load).
One JSON line per set.  Per-kernel times: run this under
`rocprofv3 --kernel-trace --stats -d <dir> -- python tools/scene_build_probe.py ...`.

    python tools/scene_build_probe.py --set c3 --set 81x3x100000
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from gswt_renderer_amd import host, synth  # noqa: E402
from gswt_renderer_amd.renderer import GSWTRenderer  # noqa: E402

SETS = {"c3": (3, 16, 9800), "81x3x100000": (3, 81, 100000), "c1": (3, 16, 50000)}


def bytes_moved(counts, n_lod, n_tile, n_view):
    n = sum(counts)
    cnt = lambda l, t: counts[l * n_tile + t]
    list_len = lambda l, t: cnt(l, t) + (cnt(l + 1, t) if l + 1 < n_lod else 0)
    pair = n_view * sum(list_len(l, t) for l in range(n_lod) for t in range(n_tile))
    arena = pair + n_view * n
    chunks = lambda k: (k + 255) // 256
    boxes = n_view * sum(chunks(list_len(l, t)) + chunks(cnt(l, t)) for l in range(n_lod) for t in range(n_tile))
    return {
        # host path: texture + arena + boxes + raw depths cross PCIe; the host also builds base lists (gs_index + gs_lod_id, 8 B / entry)
        "host_h2d_bytes": 32 * n + 4 * arena + 24 * boxes + 4 * n_view * n,
        "host_base_list_bytes": 8 * pair,
        "host_raw_depth_bytes": 4 * n_view * n,
        # rows path: the 32-byte rows and the small tables only
        "rows_h2d_bytes": 32 * n,
    }


def run(name):
    n_lod, n_tile, lod0 = SETS[name]
    verts = synth.make_tileset(n_lod=n_lod, n_tile=n_tile, lod0_count=lod0)
    out = {"set": name, "n_lod": n_lod, "n_tile": n_tile, "lod0": lod0}
    # host path
    ts = host.TileSet.from_vertices(verts)
    r = GSWTRenderer(0)
    t0 = time.perf_counter()
    w = host.WangTile(ts)
    t1 = time.perf_counter()
    w.upload_to(r)
    t2 = time.perf_counter()
    w.upload_raw_depth_to(r)
    t3 = time.perf_counter()
    out.update(host_wang_new_s=t1 - t0, host_upload_scene_s=t2 - t1, host_upload_raw_depth_s=t3 - t2, host_total_s=t3 - t0)
    w.close()
    r.close()
    # rows path
    ts = host.TileSet.from_vertices(verts)
    del verts
    r = GSWTRenderer(0)
    t0 = time.perf_counter()
    w = host.WangTile(ts, rows_only=True)
    t1 = time.perf_counter()
    r.upload_scene_rows(w)
    t2 = time.perf_counter()
    out.update(rows_wang_new_s=t1 - t0, rows_upload_scene_rows_s=t2 - t1, rows_total_s=t2 - t0)
    _, cnts, _ = w.rows_tables()
    out["n_splats"] = int(sum(cnts))
    out.update(bytes_moved(list(cnts), n_lod, n_tile, w.n_tiles[2]))
    out["speedup_end_to_end"] = out["host_total_s"] / out["rows_total_s"]
    w.close()
    r.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--set", action="append", choices=sorted(SETS), help="tile set(s) to measure (default: c3)")
    a = ap.parse_args()
    r = GSWTRenderer(0)                    # warm-up context
    warm = host.WangTile(host.TileSet.from_vertices(synth.make_tileset(n_lod=2, n_tile=16, lod0_count=500)), rows_only=True)
    r.upload_scene_rows(warm)
    warm.close()
    r.close()
    for name in a.set or ["c3"]:
        print(json.dumps(run(name)), flush=True)


if __name__ == "__main__":
    main()
