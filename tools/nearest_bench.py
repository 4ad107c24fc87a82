#!/usr/bin/env python3
"""nearest_bench.py -- points per second of the nearest-primitive query (ptmi_nearest_device) beside the closest hit (ptmi_trace_rays_device)
on as many rays, in one session.  The scenes are tools/multi_hit_bench.py's: S16 through ptmi_set_scene, world.sphere_field(10^5) through
ptmi_set_scene_bvh, world.mesh_room(8) (1.3 M triangles) through ptmi_set_scene_mesh.  The points: a 126^3 grid (2.0 M points) through the
box of the scene's sphere centres and triangle vertices, in grid order (coherent), shuffled, and shuffled but asked through
ptmi_ray_order_device's index over the rays [p, 0 0 1] (the indexed entry: the order's cost is not in the figure).  Each without r_max and
with r_max at a hundredth of the box's largest extent.  The rays of the yardstick are [p, 0 0 1] in the same order.  No figure is fixed in
advance: nothing exists to compare against but the enumeration, which the small scene shows (S16 is enumerated by every lane).

Timing (device events on the caller's stream, which the context launches on): --warmup calls, then --reps windows of --inner calls each
between two events; the median window / inner is the time per call.  Before any timing, the three point sets' answers are compared with
each other through the permutation, bit for bit, and the answers under r_max are checked to lie below it.
Usage: tools/nearest_bench.py [--reps 5] [--inner 2] [--warmup 1] [--grid 126] [--scenes s16,field,mesh] [--out profiles/nearest_bench.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inner", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--grid", type=int, default=126)
    ap.add_argument("--scenes", default="s16,field,mesh")
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch
    torch.zeros(1, device="cuda")                      # torch brings the runtime up first, as in bench.py
    torch.cuda.synchronize()
    import __graft_entry__ as graft
    pkg = graft.load_package()
    B, W = pkg.binding, pkg.world
    g = a.grid
    n = g ** 3
    perm = np.random.default_rng(1).permutation(n)
    stream = torch.cuda.Stream()
    rows = []

    def timed(call):
        for _ in range(a.warmup):
            call()
        ms = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for _ in range(a.inner):
                call()
            e1.record(stream)
            e1.synchronize()
            ms.append(e0.elapsed_time(e1) / a.inner)
        return float(np.median(ms)), float(min(ms)), float(max(ms))

    with pkg.Context(0) as c:
        c.set_stream(stream.cuda_stream)
        for name in a.scenes.split(","):
            if name == "s16":
                spheres, planes = W.scene16()
                c.set_scene(spheres, planes)
                corners, prims = [spheres["position"]], "%d spheres, %d planes" % (len(spheres), len(planes))
            elif name == "field":
                spheres, planes = W.sphere_field(100_000, seed=100_000)
                c.set_scene_bvh(spheres, planes)
                corners, prims = [spheres["position"]], "%d spheres, %d planes" % (len(spheres), len(planes))
            else:
                spheres, triangles, planes = W.mesh_room(8)
                c.set_scene_mesh(spheres, triangles, planes)
                corners, prims = [spheres["position"], triangles["v0"], triangles["v1"], triangles["v2"]], "%d spheres, %d triangles" % (len(spheres), len(triangles))
            pts = np.concatenate([np.asarray(x, np.float64).reshape(-1, 3) for x in corners])
            lo, hi = pts.min(0), pts.max(0)
            small = float((hi - lo).max()) / 100.0
            axes = [np.linspace(lo[k], hi[k], g) for k in range(3)]
            grid = np.ascontiguousarray(np.stack(np.meshgrid(*axes, indexing="ij"), -1).reshape(-1, 3), np.float32)
            shuffled = np.ascontiguousarray(grid[perm])
            up = np.tile(np.array([0, 0, 1], np.float32), (n, 1))
            with torch.cuda.stream(stream):
                d_small = torch.full((n,), small, dtype=torch.float32, device="cuda")
                d_sets = {"grid": torch.from_numpy(grid).to("cuda"), "shuffled": torch.from_numpy(shuffled).to("cuda")}
                d_rays = {k: torch.from_numpy(np.ascontiguousarray(np.concatenate([v, up], 1))).to("cuda") for k, v in (("grid", grid), ("shuffled", shuffled))}
                order = c.ray_order(d_rays["shuffled"])
                outs = (torch.empty(n, dtype=torch.float32, device="cuda"), torch.empty(n, dtype=torch.int32, device="cuda"), torch.empty((n, 3), dtype=torch.float32, device="cuda"))
                t, idx = torch.empty(n, dtype=torch.float32, device="cuda"), torch.empty(n, dtype=torch.int32, device="cuda")
                # the answers, before any timing
                ref = tuple(x.clone() for x in c.nearest(d_sets["grid"], point=True))
                d_perm = torch.from_numpy(perm).to("cuda")
                for how, kw in (("shuffled", {}), ("ordered", {"index": order})):
                    got = c.nearest(d_sets["shuffled"], out=outs, **kw)
                    stream.synchronize()
                    assert all(torch.equal(gv.view(torch.int32), rv[d_perm].view(torch.int32)) for gv, rv in zip(got, ref)), "%s, %s: the answers differ from the grid's" % (name, how)
                within = c.nearest(d_sets["grid"], r_max=d_small, point=True)
                stream.synchronize()
                found = within[1] >= 0
                assert bool((within[0].abs()[found] < small).all()) and bool((ref[0].abs()[~found] >= small).all()) and bool(torch.equal(within[1][found], ref[1][found])), name
                for set_name, d_pts, rays, kw in (("grid", d_sets["grid"], d_rays["grid"], {}), ("shuffled", d_sets["shuffled"], d_rays["shuffled"], {}),
                                                  ("shuffled, ray_order's index", d_sets["shuffled"], d_rays["shuffled"], {"index": order})):
                    figures = {"closest": timed(lambda: c.trace_rays(rays, out=(t, idx), **kw)),
                               "nearest": timed(lambda: c.nearest(d_pts, out=outs, **kw)),
                               "nearest_no_point": timed(lambda: c.nearest(d_pts, out=outs[:2], **kw)),
                               "nearest_small_r_max": timed(lambda: c.nearest(d_pts, r_max=d_small, out=outs, **kw))}
                    row = {"scene": name, "primitives": prims, "points": set_name, "n_points": n, "small_r_max": round(small, 6),
                           "within_small_r_max_share": round(float(found.float().mean().item()), 4), "mean_abs_dist": round(float(ref[0].abs().mean().item()), 5)}
                    for key, (med, lo_, hi_) in figures.items():
                        row[key + "_ms"], row[key + "_ms_min"], row[key + "_ms_max"] = round(med, 4), round(lo_, 4), round(hi_, 4)
                        row[key + "_mpoints_per_s"] = round(n / med / 1e3, 1)
                        row[key + "_over_closest"] = round(med / figures["closest"][0], 3)
                    rows.append(row)
                    print("%-5s %-28s closest hit %9.3f ms; nearest %9.3f, without locations %9.3f, within %.4g %9.3f ms (%.1f %% of the points have an answer there)" % (
                        name, set_name, row["closest_ms"], row["nearest_ms"], row["nearest_no_point_ms"], small, row["nearest_small_r_max_ms"],
                        100 * row["within_small_r_max_share"]), flush=True)
        torch.cuda.synchronize()
        c.set_stream(None)
    res = {"tool": "nearest_bench", "build_id": B.load_library().build_id, "device": torch.cuda.get_device_name(0), "grid": g,
           "clock": time.strftime("%Y-%m-%d %H:%M:%S UTC", time.gmtime()), "reps": a.reps, "inner": a.inner, "warmup": a.warmup, "rows": rows}
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
