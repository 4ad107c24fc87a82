#!/usr/bin/env python3
"""bvh_bench.py -- render Inline on BVH scenes (ptmi_set_scene_bvh): 1920 x 1080, 8 samples per pixel, bounce limit 8, on scene S16
(16 primitives) and the random sphere fields of world.sphere_field (1k, 16k, 256k and 1M spheres, 4 planes), and -- wherever the scene
fits the linear path (S16; 1020 spheres + 4 planes = 1024 primitives, its limit) -- the same scene through ptmi_set_scene.  Prints one line per scene and a JSON summary: Msamples/s,
ms per launch (device time, median of --reps launches after --warmup), host build time of the hierarchy and its node count.
Usage: tools/bvh_bench.py [--reps 5] [--warmup 2] [--sizes s16,1020,16000,256000,1000000] [--out FILE]  (profiles/bvh_bench.json: the
DESIGN.md 5.7 table's run)"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as graft  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sizes", default="s16,1020,16000,256000,1000000", help="sphere counts of world.sphere_field; s16: scene S16 (14 spheres + 2 planes)")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--spp", type=int, default=8)
    ap.add_argument("--limit", type=int, default=8)
    ap.add_argument("--out")
    a = ap.parse_args()
    pkg = graft.load_package()
    B = pkg.binding
    cam = pkg.world.initial_camera()
    rows = []
    with pkg.Context(0) as c:
        c.set_timing(True)
        c.resize(a.width, a.height)
        for size in a.sizes.split(","):
            if size == "s16":
                spheres, planes = pkg.world.scene16()
            else:
                spheres, planes = pkg.world.sphere_field(int(size), seed=int(size))
            n = len(spheres)
            t0 = time.perf_counter()
            nodes, _ = B.bvh_layout(spheres)
            build_s = time.perf_counter() - t0
            kinds = ["bvh"] + (["linear"] if n + len(planes) <= B.MAX_PRIMITIVES else [])
            for kind in kinds:
                (c.set_scene_bvh if kind == "bvh" else c.set_scene)(spheres, planes)
                c.init_output(1)
                ms = []
                for k in range(a.warmup + a.reps):
                    c.render(cam, a.limit, a.spp, B.INLINE)
                    c.synchronize()
                    if k >= a.warmup:
                        ms.append(c.stats()["last_render_ms"])
                med = float(np.median(ms))
                row = {"scene_name": "S16" if size == "s16" else "sphere_field", "spheres": n, "planes": len(planes), "scene": kind, "ms_per_launch": round(med, 3), "ms_min": round(min(ms), 3),
                       "msamples_per_s": round(a.width * a.height * a.spp / med / 1e3, 2),
                       "bvh_build_s": round(build_s, 3) if kind == "bvh" else None, "bvh_nodes": int(len(nodes)) if kind == "bvh" else None}
                rows.append(row)
                print("%-4s %8d spheres %-6s %9.3f ms/launch (min %.3f)  %8.2f Msamples/s  build %s  nodes %s" % (
                    "S16" if size == "s16" else "", n, kind, med, min(ms), row["msamples_per_s"], row["bvh_build_s"], row["bvh_nodes"]), flush=True)
    res = {"tool": "bvh_bench", "build_id": B.load_library().build_id, "shape": [a.width, a.height], "spp": a.spp, "limit": a.limit, "rows": rows}
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
