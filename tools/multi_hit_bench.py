#!/usr/bin/env python3
"""multi_hit_bench.py -- rays per second of the multi-hit query (ptmi_trace_rays_multi_device) beside the closest hit
(ptmi_trace_rays_device), in one session.  The scenes and ray sets are tools/ray_query_bench.py's: S16 through ptmi_set_scene,
world.sphere_field(10^5) through ptmi_set_scene_bvh, world.mesh_room(8) (1.3 M triangles) through ptmi_set_scene_mesh; 1920 x 1080 camera
rays in image order (coherent) and shuffled (incoherent).  Per scene and ray set: the closest hit; k = 1, 4 and 16 without t_max; k = 4
with t_max at twice the closest hit's t.  The closest hit's kernels (csrc/ptmi_query.hip) are untouched by the multi-hit unit -- the
object is the parent commit's -- so its time in this session is the yardstick.

Timing (device events on the caller's stream, which the context launches on): --warmup calls, then --reps windows of --inner calls each
between two events; the median window / inner is the time per call.  Before any timing, column 0 at k = 1 is compared with the closest
hit bit for bit, and the rows at k = 4 under t_max are checked to lie below it in ascending order.
Usage: tools/multi_hit_bench.py [--reps 7] [--inner 3] [--warmup 2] [--scenes s16,field,mesh] [--out profiles/multi_hit_bench.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from ray_query_bench import camera_rays  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--scenes", default="s16,field,mesh")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch
    torch.zeros(1, device="cuda")                      # torch brings the runtime up first, as in bench.py
    torch.cuda.synchronize()
    import __graft_entry__ as graft
    pkg = graft.load_package()
    B, W = pkg.binding, pkg.world
    n = a.width * a.height
    coherent = camera_rays(W.initial_camera(), a.width, a.height)
    shuffled = np.ascontiguousarray(coherent[np.random.default_rng(1).permutation(n)])
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
                prims = "%d spheres, %d planes" % (len(spheres), len(planes))
            elif name == "field":
                spheres, planes = W.sphere_field(100_000, seed=100_000)
                c.set_scene_bvh(spheres, planes)
                prims = "%d spheres, %d planes" % (len(spheres), len(planes))
            else:
                spheres, triangles, planes = W.mesh_room(8)
                c.set_scene_mesh(spheres, triangles, planes)
                prims = "%d spheres, %d triangles" % (len(spheres), len(triangles))
            for rays_name, rays in (("coherent", coherent), ("incoherent", shuffled)):
                with torch.cuda.stream(stream):
                    d_rays = torch.from_numpy(rays).to("cuda")
                    t, idx = torch.empty(n, dtype=torch.float32, device="cuda"), torch.empty(n, dtype=torch.int32, device="cuda")
                    outs = {k: (torch.empty((n, k), dtype=torch.float32, device="cuda"), torch.empty((n, k), dtype=torch.int32, device="cuda"),
                                torch.empty(n, dtype=torch.int32, device="cuda")) for k in (1, 4, 16)}
                    # the answers, before any timing
                    c.trace_rays(d_rays, out=(t, idx))
                    c.trace_rays_multi(d_rays, 1, out=outs[1])
                    stream.synchronize()
                    hit = idx >= 0
                    assert torch.equal(outs[1][0][:, 0].view(torch.int32), t.view(torch.int32)) and torch.equal(outs[1][1][:, 0], idx), "column 0 at k = 1"
                    d_twice = torch.where(hit, 2.0 * t, torch.full_like(t, float("inf")))
                    c.trace_rays_multi(d_rays, 4, t_max=d_twice, out=outs[4])
                    c.trace_rays_multi(d_rays, 16, out=outs[16])
                    stream.synchronize()
                    t4, _, c4 = outs[4]
                    listed = torch.arange(4, device="cuda")[None, :] < c4[:, None]
                    assert bool(((t4 < d_twice[:, None]) | ~listed).all()) and bool(((t4[:, 1:] >= t4[:, :-1]) | ~listed[:, 1:]).all()), "k = 4 under t_max"
                    mean_count = {"k4_twice": float(c4.float().mean().item()), "k16": float(outs[16][2].float().mean().item())}
                    figures = {"closest": timed(lambda: c.trace_rays(d_rays, out=(t, idx))),
                               "k1": timed(lambda: c.trace_rays_multi(d_rays, 1, out=outs[1])),
                               "k4": timed(lambda: c.trace_rays_multi(d_rays, 4, out=outs[4])),
                               "k16": timed(lambda: c.trace_rays_multi(d_rays, 16, out=outs[16])),
                               "k4_twice": timed(lambda: c.trace_rays_multi(d_rays, 4, t_max=d_twice, out=outs[4]))}
                row = {"scene": name, "primitives": prims, "rays": rays_name, "n_rays": n, "hit_share": round(float(hit.float().mean().item()), 4),
                       "mean_count_k16": round(mean_count["k16"], 3), "mean_count_k4_twice": round(mean_count["k4_twice"], 3)}
                for key, (med, lo, hi) in figures.items():
                    row[key + "_ms"], row[key + "_ms_min"], row[key + "_ms_max"] = round(med, 4), round(lo, 4), round(hi, 4)
                    row[key + "_mrays_per_s"] = round(n / med / 1e3, 1)
                    row[key + "_over_closest"] = round(med / figures["closest"][0], 3)
                rows.append(row)
                print("%-5s %-10s closest %8.3f ms; k = 1 %8.3f, k = 4 %8.3f, k = 16 %8.3f, k = 4 within twice the closest %8.3f ms; hits listed at k = 16: %.2f a ray" % (
                    name, rays_name, row["closest_ms"], row["k1_ms"], row["k4_ms"], row["k16_ms"], row["k4_twice_ms"], row["mean_count_k16"]), flush=True)
        torch.cuda.synchronize()
        c.set_stream(None)
    res = {"tool": "multi_hit_bench", "build_id": B.load_library().build_id, "device": torch.cuda.get_device_name(0), "shape": [a.width, a.height],
           "clock": time.strftime("%Y-%m-%d %H:%M:%S UTC", time.gmtime()), "reps": a.reps, "inner": a.inner, "warmup": a.warmup, "rows": rows}
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
