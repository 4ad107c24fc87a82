#!/usr/bin/env python3
"""ray_bounce_bench.py -- what a path tracer stepped by the caller (ptmi_bounce_rays_device, ptmi_live_rays_device) costs against the closed
loop, ptmi_trace_paths_device(limit, 1 spp) of a baseline library built from the parent commit (--baseline-lib), in one session on one
device.  Three scenes at 1920 x 1080 camera rays, bounce limit 8 -- S16, world.sphere_field(10^5) as a BVH scene and world.mesh_room(8)
(1.3 M triangles) as a mesh scene: tools/ray_paths_bench.py's -- and the rays both in image order (coherent) and in a seeded random order
(shuffled).  Per scene and order the time of one whole path per ray:
  closed          the parent library's trace_paths(limit, 1 spp): one launch
  steps_all       (a) `limit` bounce_rays over all rays
  steps_live      (b) a step over all rays, then live_rays; then limit - 1 times: a step through the list, live_rays in place
  steps_ordered   (c) as (b), but before every second step the list is made from ray_order's order of the current rays, so that the live rays
                  are stepped in a coherent order (ray_order sorts all n rays: it has no indexed form)
and each of the three against closed.  The state goes through memory once per bounce -- 16 words in and out per ray -- where the closed
loop keeps it in registers.  Separately: live_rays alone at --candidates candidates, all, half and none of them live.

Timing (device events on the caller's stream, which both contexts launch on): the state is put back before every call, outside the
events; --warmup calls of every variant, then --reps rounds, a round timing every variant once in turn; the median is reported with the
smallest and largest.  Before any timing 0 + radiance and the seeds of every stepped form are compared bit for bit with the closed loop's.
Usage: tools/ray_bounce_bench.py --baseline-lib PATH [--reps 9] [--warmup 3] [--scenes s16,field,mesh] [--out profiles/ray_bounce_bench.json]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from ray_order_bench import open_baseline  # noqa: E402
from ray_query_bench import camera_rays  # noqa: E402

LIMIT = 8
VARIANTS = ("steps_all", "steps_live", "steps_ordered")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--baseline-lib", required=True, help="libptmi.so built from the parent commit")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--scenes", default="s16,field,mesh")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--candidates", type=int, default=2_000_000)
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch
    torch.zeros(1, device="cuda")                      # torch brings the runtime up first, as in bench.py
    torch.cuda.synchronize()
    import __graft_entry__ as graft
    pkg = graft.load_package()
    B, W = pkg.binding, pkg.world
    base_lib = open_baseline(B, a.baseline_lib)
    this_lib = B.load_library()
    assert base_lib.build_id != this_lib.build_id, "the baseline library is this library"
    n = a.width * a.height
    stream = torch.cuda.Stream()
    cam = W.initial_camera()
    res = {"tool": "ray_bounce_bench", "build_id": this_lib.build_id, "baseline_build_id": base_lib.build_id, "device": torch.cuda.get_device_name(0),
           "shape": [a.width, a.height], "bounce_limit": LIMIT, "reps": a.reps, "warmup": a.warmup, "rows": [], "live_rays_alone": []}

    def write():
        if a.out:
            with open(a.out, "w") as fh:
                json.dump(res, fh, indent=1)

    def timed(calls, reset):
        """{name: call} -> {name: (median, min, max) ms}; reset() before every call, outside the events; a round times every variant in turn"""
        for call in calls.values():
            for _ in range(a.warmup):
                reset()
                call()
        ms = {name: [] for name in calls}
        for _ in range(a.reps):
            for name, call in calls.items():
                reset()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                call()
                e1.record(stream)
                e1.synchronize()
                ms[name].append(e0.elapsed_time(e1))
        return {name: (float(np.median(v)), float(min(v)), float(max(v))) for name, v in ms.items()}

    with pkg.Context(0) as c, pkg.Context(0, library=base_lib) as base:
        for ctx in (c, base):
            ctx.set_stream(stream.cuda_stream)
        with torch.cuda.stream(stream):
            # the compaction alone
            m = a.candidates
            ramp = torch.arange(m, device="cuda")
            work = torch.empty(B.live_rays_bytes(m), dtype=torch.uint8, device="cuda")
            out = torch.empty(m, dtype=torch.int32, device="cuda")
            count = torch.zeros(1, dtype=torch.int32, device="cuda")
            index = torch.randperm(m, device="cuda").to(torch.int32)
            for share, alive in (("all", ramp >= 0), ("half", (ramp * 2654435761 >> 7) % 2 == 0), ("none", ramp < 0)):
                thr = alive.to(torch.float32)[:, None].repeat(1, 3).contiguous()
                f = timed({"every_ray": lambda: c.live_rays(thr, out=out, count=count, work=work),
                           "through_a_shuffled_index": lambda: c.live_rays(thr, index=index, out=out, count=count, work=work)}, lambda: None)
                assert int(count.item()) == int(alive.sum().item())
                row = {"candidates": m, "live": share}
                for key, (med, lo, hi) in f.items():
                    row[key + "_ms"], row[key + "_ms_min"], row[key + "_ms_max"] = round(med, 4), round(lo, 4), round(hi, 4)
                res["live_rays_alone"].append(row)
                print("live_rays alone, %d candidates, %s live: %.4f ms; through a shuffled index %.4f ms" % (m, share, row["every_ray_ms"],
                                                                                                            row["through_a_shuffled_index_ms"]), flush=True)
            del thr, index, out, ramp
            write()
        for name in a.scenes.split(","):
            if name == "s16":
                spheres, planes = W.scene16()
                for ctx in (c, base):
                    ctx.set_scene(spheres, planes)
                prims = "%d spheres, %d planes" % (len(spheres), len(planes))
            elif name == "field":
                spheres, planes = W.sphere_field(100_000, seed=100_000)
                for ctx in (c, base):
                    ctx.set_scene_bvh(spheres, planes)
                prims = "%d spheres, %d planes" % (len(spheres), len(planes))
            else:
                spheres, triangles, planes = W.mesh_room(8)
                for ctx in (c, base):
                    ctx.set_scene_mesh(spheres, triangles, planes)
                prims = "%d spheres, %d triangles" % (len(spheres), len(triangles))
            with torch.cuda.stream(stream):
                coherent = torch.from_numpy(camera_rays(cam, a.width, a.height)).to("cuda")
                perm = torch.from_numpy(np.random.default_rng(1).permutation(n)).to("cuda")
                seeds0 = c.path_seeds(0x5EED1234, n)
                rays = torch.empty_like(coherent)
                thr, rad = torch.empty((n, 3), dtype=torch.float32, device="cuda"), torch.empty((n, 3), dtype=torch.float32, device="cuda")
                seeds = torch.empty_like(seeds0)
                live = torch.empty(n, dtype=torch.int32, device="cuda")
                order = torch.empty(n, dtype=torch.int32, device="cuda")
                counts = torch.zeros(LIMIT, dtype=torch.int32, device="cuda")
                work = torch.empty(B.live_rays_bytes(n), dtype=torch.uint8, device="cuda")
                owork = torch.empty(B.ray_order_bytes(n), dtype=torch.uint8, device="cuda")
                for arrangement in ("coherent", "shuffled"):
                    rays0 = coherent if arrangement == "coherent" else coherent[perm].contiguous()

                    def reset():
                        rays.copy_(rays0)
                        thr.fill_(1.0)
                        rad.zero_()
                        seeds.copy_(seeds0)

                    def closed():
                        base.trace_paths(rays, seeds, LIMIT, spp=1, color=rad)

                    def steps_all():
                        for _ in range(LIMIT):
                            c.bounce_rays(rays, seeds, thr, rad)

                    def steps_live():
                        c.bounce_rays(rays, seeds, thr, rad)
                        c.live_rays(thr, out=live, count=counts[0:1], work=work)
                        for k in range(1, LIMIT):
                            c.bounce_rays(rays, seeds, thr, rad, index=live)
                            c.live_rays(thr, index=live, out=live, count=counts[k:k + 1], work=work)

                    def steps_ordered():
                        c.bounce_rays(rays, seeds, thr, rad)
                        for k in range(1, LIMIT):
                            if k % 2 == 1:                     # before every second step: the live rays in ray_order's order of the current rays
                                c.ray_order(rays, out=order, work=owork)
                                c.live_rays(thr, index=order, out=live, count=counts[k - 1:k], work=work)
                            else:
                                c.live_rays(thr, index=live, out=live, count=counts[k - 1:k], work=work)
                            c.bounce_rays(rays, seeds, thr, rad, index=live)

                    # the answers, before any timing: every stepped form against the closed loop, bit for bit
                    reset()
                    closed()
                    want = (rad.clone(), seeds.clone())
                    live_counts = None
                    for variant, call in (("steps_all", steps_all), ("steps_live", steps_live), ("steps_ordered", steps_ordered)):
                        reset()
                        call()
                        got = 0.0 + rad
                        same = (got.view(torch.int32) == want[0].view(torch.int32)) | (got.isnan() & want[0].isnan())
                        assert bool(same.all()) and torch.equal(seeds, want[1]), (name, arrangement, variant)
                        if variant == "steps_live":
                            live_counts = [int(x) for x in counts.tolist()]
                    f = timed({"closed": closed, "steps_all": steps_all, "steps_live": steps_live, "steps_ordered": steps_ordered}, reset)
                    row = {"scene": name, "primitives": prims, "rays": arrangement, "n_rays": n, "bounce_limit": LIMIT, "live_after_step": live_counts}
                    for key, (med, lo, hi) in f.items():
                        row[key + "_ms"], row[key + "_ms_min"], row[key + "_ms_max"] = round(med, 4), round(lo, 4), round(hi, 4)
                    for key in VARIANTS:
                        row[key + "_over_closed"] = round(f[key][0] / f["closed"][0], 3)
                    res["rows"].append(row)
                    print("%-5s %-8s closed %8.3f ms | steps over all %8.3f (x %.3f) through the live list %8.3f (x %.3f) ordered every second step %8.3f (x %.3f)" % (
                        name, arrangement, row["closed_ms"], row["steps_all_ms"], row["steps_all_over_closed"], row["steps_live_ms"], row["steps_live_over_closed"],
                        row["steps_ordered_ms"], row["steps_ordered_over_closed"]), flush=True)
                    write()
        torch.cuda.synchronize()
        for ctx in (c, base):
            ctx.set_stream(None)
    print(json.dumps(res))
    write()


if __name__ == "__main__":
    main()
