#!/usr/bin/env python3
"""mesh_bench.py -- render Inline on mesh scenes (ptmi_set_scene_mesh): 1920 x 1080, 8 samples per pixel, bounce limit 8, on
world.mesh_room at icosphere subdivisions 3, 5, 6 and 8 (~1.3k, 20k, 82k and 1.3M triangles, 8 spheres), the same room's spheres
alone through ptmi_set_scene_bvh, and a sphere BVH of about a million primitives (world.sphere_field(1000000)) for comparison.
Prints one line per scene and a JSON summary: ms per launch (device time, median of --reps launches after --warmup), Msamples/s,
host build time of the triangle hierarchy and its node count.
Usage: tools/mesh_bench.py [--reps 5] [--warmup 2] [--subdivisions 3,5,6,8] [--out FILE]  (profiles/mesh_bench.json: the DESIGN.md
5.8 table's run)"""
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
    ap.add_argument("--subdivisions", default="3,5,6,8")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--spp", type=int, default=8)
    ap.add_argument("--limit", type=int, default=8)
    ap.add_argument("--out")
    a = ap.parse_args()
    pkg = graft.load_package()
    B, W = pkg.binding, pkg.world
    cam = W.initial_camera()
    rows = []

    def timed(c):
        c.init_output(1)
        ms = []
        for k in range(a.warmup + a.reps):
            c.render(cam, a.limit, a.spp, B.INLINE)
            c.synchronize()
            if k >= a.warmup:
                ms.append(c.stats()["last_render_ms"])
        return float(np.median(ms)), min(ms)

    with pkg.Context(0) as c:
        c.set_timing(True)
        c.resize(a.width, a.height)
        cases = [("mesh_room", int(s)) for s in a.subdivisions.split(",")] + [("room_spheres_bvh", 0), ("sphere_field_bvh", 1000000)]
        for name, k in cases:
            build_s, nodes = None, None
            if name == "mesh_room":
                spheres, tris, planes = W.mesh_room(k)
                t0 = time.perf_counter()
                nodes = len(B.mesh_layout(tris)[0])
                build_s = time.perf_counter() - t0
                c.set_scene_mesh(spheres, tris, planes)
            elif name == "room_spheres_bvh":
                spheres, tris, planes = W.mesh_room(0)
                tris = tris[:0]
                c.set_scene_bvh(spheres, planes)
            else:
                spheres, planes = W.sphere_field(k, seed=k)
                tris = np.zeros(0, W.TRIANGLE_DTYPE)
                c.set_scene_bvh(spheres, planes)
            med, lo = timed(c)
            row = {"scene": name, "subdivisions": k if name == "mesh_room" else None, "triangles": int(len(tris)), "spheres": int(len(spheres)),
                   "planes": int(len(planes)), "ms_per_launch": round(med, 3), "ms_min": round(lo, 3),
                   "msamples_per_s": round(a.width * a.height * a.spp / med / 1e3, 2),
                   "mesh_build_s": round(build_s, 3) if build_s is not None else None, "mesh_nodes": nodes}
            rows.append(row)
            print("%-17s %8d triangles %8d spheres %9.3f ms/launch (min %.3f) %8.2f Msamples/s  build %s  nodes %s" % (
                name, row["triangles"], row["spheres"], med, lo, row["msamples_per_s"], row["mesh_build_s"], nodes), flush=True)
    res = {"tool": "mesh_bench", "build_id": B.load_library().build_id, "shape": [a.width, a.height], "spp": a.spp, "limit": a.limit, "rows": rows}
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
