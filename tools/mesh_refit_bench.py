#!/usr/bin/env python3
"""mesh_refit_bench.py -- moving a mesh scene's vertices: ptmi_update_mesh_vertices (the hierarchy refitted on the device) against
ptmi_set_scene_mesh (rebuilt on the host), on world.mesh_room at icosphere subdivisions 5, 6 and 8 (~20k, 82k and 1.3M triangles).
Per scene, each figure the median of --reps after --warmup:
  (a) wall time of set_scene_mesh on the moved triangles -- the only way to move a vertex without this entry;
  (b) wall time of update_mesh_vertices from host memory and from a device tensor (each followed by a synchronize), and the device time
      of the update from the tensor between two events on the context's stream (check kernel, the host's read-back, records, levels);
  (c) render Inline, 1920 x 1080, 8 samples per pixel, bounce limit 8, after a REFIT against after a FRESH BUILD of the same geometry,
      the icosphere's vertices displaced by 1 %, 10 % and 50 % of its radius, by a smooth wave and by per-vertex noise
      (world.displaced): the price of keeping the topology.
The gate: (b) is faster than (a) of the same run at subdivisions 6 and 8, for both entries (exit status 1 otherwise).
Usage: tools/mesh_refit_bench.py [--reps 5] [--warmup 2] [--subdivisions 5,6,8] [--out FILE]  (profiles/mesh_refit_bench.json: the
DESIGN.md 5.8 table's run)"""
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
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--subdivisions", default="5,6,8")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--spp", type=int, default=8)
    ap.add_argument("--limit", type=int, default=8)
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch                                     # (torch brings the HIP runtime up first: the library then shares it, as in bench.py)
    torch.cuda.set_device(0)
    stream = torch.cuda.Stream()
    import __graft_entry__ as graft
    pkg = graft.load_package()
    B, W = pkg.binding, pkg.world
    cam = W.initial_camera()

    def median_of(call, after=None):
        out = []
        for k in range(a.warmup + a.reps):
            t0 = time.perf_counter()
            got = call()
            dt = (time.perf_counter() - t0) * 1e3
            if k >= a.warmup:
                out.append(dt if got is None else got)
            if after:
                after()
        return float(np.median(out))

    rows, ok = [], True
    with pkg.Context(0) as c, pkg.Context(0) as fresh:
        c.set_stream(stream.cuda_stream)
        for x in (c, fresh):
            x.set_timing(True)
            x.resize(a.width, a.height)

        def render_ms(x):
            x.init_output(1)
            ms = []
            for k in range(a.warmup + a.reps):
                x.render(cam, a.limit, a.spp, B.INLINE)
                x.synchronize()
                if k >= a.warmup:
                    ms.append(x.stats()["last_render_ms"])
            return float(np.median(ms))

        for sub in [int(s) for s in a.subdivisions.split(",")]:
            spheres, tris, planes = W.mesh_room(sub)
            v0 = W.triangle_vertices(tris)
            v1 = W.displaced(v0, 0.1, "wave")
            moved = W.with_vertices(tris, v1)
            c.set_scene_mesh(spheres, tris, planes)
            c.synchronize()
            set_ms = median_of(lambda: (fresh.set_scene_mesh(spheres, moved, planes), fresh.synchronize())[0])
            flip = [v1, v0]

            def host_update():
                c.update_mesh_vertices(flip[0])
                c.synchronize()
                flip.reverse()
            host_ms = median_of(host_update)
            d = [torch.from_numpy(v1).to("cuda:0"), torch.from_numpy(v0).to("cuda:0")]
            torch.cuda.synchronize()

            def device_update():
                c.update_mesh_vertices(d[0])
                c.synchronize()
                d.reverse()
            device_ms = median_of(device_update)

            def device_events():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                c.update_mesh_vertices(d[0])
                e1.record(stream)
                e1.synchronize()
                d.reverse()
                return e0.elapsed_time(e1)
            event_ms = median_of(device_events)
            row = {"subdivisions": sub, "triangles": int(len(tris)), "set_scene_mesh_ms": round(set_ms, 3), "update_host_ms": round(host_ms, 3),
                   "update_device_ms": round(device_ms, 3), "update_device_event_ms": round(event_ms, 3),
                   "set_over_update_host": round(set_ms / host_ms, 1), "set_over_update_device": round(set_ms / device_ms, 1), "renders": []}
            if sub >= 6 and not (host_ms < set_ms and device_ms < set_ms):
                ok = False
            print("subdivisions %d, %8d triangles: set_scene_mesh %9.3f ms | update from host %8.3f ms (%.1fx), from a device tensor %8.3f ms (%.1fx; "
                  "%.3f ms between events)" % (sub, len(tris), set_ms, host_ms, set_ms / host_ms, device_ms, set_ms / device_ms, event_ms), flush=True)
            for kind in ("wave", "noise"):
                for amount in (0.01, 0.1, 0.5):
                    v = W.displaced(v0, amount, kind)
                    c.set_scene_mesh(spheres, tris, planes)
                    c.update_mesh_vertices(v)
                    refit = render_ms(c)
                    fresh.set_scene_mesh(spheres, W.with_vertices(tris, v), planes)
                    built = render_ms(fresh)
                    row["renders"].append({"kind": kind, "amount": amount, "render_ms_after_refit": round(refit, 3),
                                           "render_ms_after_build": round(built, 3), "refit_over_build": round(refit / built, 3)})
                    print("    %-5s %4.0f %% of the radius: render %8.3f ms after a refit, %8.3f ms after a fresh build (x %.3f)" % (
                        kind, 100 * amount, refit, built, refit / built), flush=True)
            rows.append(row)
    res = {"tool": "mesh_refit_bench", "build_id": B.load_library().build_id, "shape": [a.width, a.height], "spp": a.spp, "limit": a.limit,
           "reps": a.reps, "warmup": a.warmup, "gate_update_faster_than_set_scene_at_6_and_8": ok, "rows": rows}
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
