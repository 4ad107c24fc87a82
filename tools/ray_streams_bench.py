#!/usr/bin/env python3
"""ray_streams_bench.py -- what render Streams along a caller's rays (ptmi_trace_streams_device, ptmi_trace_streams_indexed_device) costs
against ptmi_render(PTMI_STREAMS) in its per-pixel form (PTMI_FORM_PIXEL) of a baseline library built from the parent commit
(--baseline-lib), in one session on one device.  Four scenes at 1920 x 1080: world.glass_scene() at 64 spp (the tree walk), S16 at 64 spp
(the chain), world.sphere_field(10^5) with a glass fraction as a BVH scene and world.mesh_room(8) (1.3 M triangles) with every fourth mesh
triangle GLASS as a mesh scene, at 8 spp.  Per scene the time per call of
  render             the parent library's ptmi_render(PTMI_STREAMS) of the pinhole camera
  streams_coherent   trace_streams along one ray per pixel of that camera, in image order (ray_query_bench.camera_rays)
  streams_shuffled   the same rays in a seeded random order
  streams_ordered    the shuffled rays through ptmi_ray_order_device's order as the index (the order made once, outside the timing)
and each of the three against render.  The ray kernels' waves are 64 consecutive rays where render's are 8 x 8 tiles dispatched by recorded
cost, and render splits its samples into chunks where a launch has few rounds of waves.

Timing (device events on the caller's stream, which both contexts launch on): --warmup calls of every variant, then --reps rounds; a round
times every variant in turn, --inner calls between two events each; the median window / inner is the time per call.  Before any timing the
coherent and the ordered call are compared bit for bit (a permutation apart).
Usage: tools/ray_streams_bench.py --baseline-lib PATH [--reps 7] [--inner 3] [--warmup 3] [--scenes glass,s16,field,mesh] [--out profiles/ray_streams_bench.json]"""
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

SPP = {"glass": 64, "s16": 64, "field": 8, "mesh": 8}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--baseline-lib", required=True, help="libptmi.so built from the parent commit")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--scenes", default="glass,s16,field,mesh")
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
    base_lib = open_baseline(B, a.baseline_lib)
    this_lib = B.load_library()
    assert base_lib.build_id != this_lib.build_id, "the baseline library is this library"
    n = a.width * a.height
    stream = torch.cuda.Stream()
    cam = W.initial_camera()
    rows = []

    def timed(calls):
        """{name: call} -> {name: (median, min, max) ms per call}; every round times every variant in turn"""
        for call in calls.values():
            for _ in range(a.warmup):
                call()
        ms = {name: [] for name in calls}
        for _ in range(a.reps):
            for name, call in calls.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                for _ in range(a.inner):
                    call()
                e1.record(stream)
                e1.synchronize()
                ms[name].append(e0.elapsed_time(e1) / a.inner)
        return {name: (float(np.median(v)), float(min(v)), float(max(v))) for name, v in ms.items()}

    with pkg.Context(0) as c, pkg.Context(0, library=base_lib) as base:
        for ctx in (c, base):
            ctx.set_stream(stream.cuda_stream)
        base.set_option(B.OPT_STREAMS_FORM, B.FORM_PIXEL)
        for name in a.scenes.split(","):
            spp = SPP[name]
            if name in ("glass", "s16"):
                spheres, planes = W.glass_scene() if name == "glass" else W.scene16()
                for ctx in (c, base):
                    ctx.set_scene(spheres, planes)
                prims = "%d spheres, %d planes" % (len(spheres), len(planes))
            elif name == "field":
                spheres, planes = W.sphere_field(100_000, seed=100_000, glass_fraction=0.1)
                for ctx in (c, base):
                    ctx.set_scene_bvh(spheres, planes)
                prims = "%d spheres (a tenth GLASS), %d planes" % (len(spheres), len(planes))
            else:
                spheres, triangles, planes = W.mesh_room(8)
                triangles = triangles.copy()
                glass = np.arange(len(triangles)) % 4 == 3
                glass[:13] = False                      # (the room and its light stay what they are)
                triangles["brdf_tag"][glass], triangles["brdf_param"][glass] = W.GLASS, 1.5
                triangles["color"][glass] = (0.95, 0.95, 0.95)
                for ctx in (c, base):
                    ctx.set_scene_mesh(spheres, triangles, planes)
                prims = "%d spheres, %d triangles (a quarter of the mesh GLASS)" % (len(spheres), len(triangles))
            base.resize(a.width, a.height)
            base.init_output(0x5EED1234)
            with torch.cuda.stream(stream):
                coherent = torch.from_numpy(camera_rays(cam, a.width, a.height)).to("cuda")
                perm = torch.from_numpy(np.random.default_rng(1).permutation(n)).to("cuda")
                shuffled = coherent[perm].contiguous()
                order = c.ray_order(shuffled)
                seeds0 = c.path_seeds(0x5EED1234, n)
                seeds = [seeds0.clone() for _ in range(3)]
                colors = [torch.zeros((n, 3), dtype=torch.float32, device="cuda") for _ in range(3)]
                work = torch.empty(c.trace_streams_bytes(n), dtype=torch.uint8, device="cuda")
                lost = torch.zeros(2, dtype=torch.int64, device="cuda")
                # the answers, before any timing: the shuffled batch through the order, against the coherent batch, a permutation apart
                c.trace_streams(coherent, seeds[0], spp=1, color=colors[0], work=work, lost=lost)
                seeds[2].copy_(seeds0[perm])
                c.trace_streams(shuffled, seeds[2], spp=1, color=colors[2], index=order, work=work)
                stream.synchronize()
                assert torch.equal(colors[2].view(torch.int32), colors[0][perm].view(torch.int32)) and torch.equal(seeds[2], seeds[0][perm]), name
                lit = round(float((colors[0] != 0).any(1).float().mean().item()), 4)
                f = timed({"render": lambda: base.render(cam, 8, spp, pkg.STREAMS),
                           "streams_coherent": lambda: c.trace_streams(coherent, seeds[0], spp=spp, color=colors[0], work=work),
                           "streams_shuffled": lambda: c.trace_streams(shuffled, seeds[1], spp=spp, color=colors[1], work=work),
                           "streams_ordered": lambda: c.trace_streams(shuffled, seeds[2], spp=spp, color=colors[2], index=order, work=work)})
            row = {"scene": name, "primitives": prims, "n_rays": n, "spp": spp, "lit_share": lit, "lost_in_one_sample": lost.tolist()}
            for key, (med, lo, hi) in f.items():
                row[key + "_ms"], row[key + "_ms_min"], row[key + "_ms_max"] = round(med, 4), round(lo, 4), round(hi, 4)
            for key in ("streams_coherent", "streams_shuffled", "streams_ordered"):
                row[key + "_over_render"] = round(f[key][0] / f["render"][0], 3)
            rows.append(row)
            print("%-5s %2d spp: render %8.3f ms | streams coherent %8.3f (x %.3f) shuffled %8.3f (x %.3f) shuffled through the order %8.3f (x %.3f)" % (
                name, spp, row["render_ms"], row["streams_coherent_ms"], row["streams_coherent_over_render"], row["streams_shuffled_ms"],
                row["streams_shuffled_over_render"], row["streams_ordered_ms"], row["streams_ordered_over_render"]), flush=True)
        torch.cuda.synchronize()
        for ctx in (c, base):
            ctx.set_stream(None)
    res = {"tool": "ray_streams_bench", "build_id": this_lib.build_id, "baseline_build_id": base_lib.build_id, "device": torch.cuda.get_device_name(0),
           "shape": [a.width, a.height], "reps": a.reps, "inner": a.inner, "warmup": a.warmup, "rows": rows}
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
