#!/usr/bin/env python3
"""mesh_build_bench.py -- giving a mesh scene new triangles: ptmi_set_mesh_triangles (the hierarchy built on the device) against
ptmi_set_scene_mesh (built on the host), on world.mesh_room at icosphere subdivisions 3, 6 and 8 (1 293, 81 933 and 1 310 733
triangles).  Per scene, each figure the median of --reps after --warmup:
  (a) wall time of set_scene_mesh;
  (b) wall time of set_mesh_triangles from host memory;
  (c) wall time of set_mesh_triangles from a device tensor (each followed by a synchronize);
  (d) render Inline, 1920 x 1080, 8 samples per pixel, bounce limit 8, over the host-built hierarchy (longest-axis median splits);
  (e) the same render over the device-built hierarchy (Morton order, equal-count splits) -- the same image, another tree.
The gate: (c) is below (a) of the same run by more than 2 % at subdivisions 6 and 8 (exit status 1 otherwise).
Usage: tools/mesh_build_bench.py [--reps 5] [--warmup 2] [--subdivisions 3,6,8] [--out FILE]  (profiles/mesh_build_bench.json: the
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
    ap.add_argument("--subdivisions", default="3,6,8")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--spp", type=int, default=8)
    ap.add_argument("--limit", type=int, default=8)
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch                                     # (torch brings the HIP runtime up first: the library then shares it, as in bench.py)
    torch.cuda.set_device(0)
    import __graft_entry__ as graft
    pkg = graft.load_package()
    B, W = pkg.binding, pkg.world
    cam = W.initial_camera()

    def median_of(call):
        out = []
        for k in range(a.warmup + a.reps):
            t0 = time.perf_counter()
            call()
            if k >= a.warmup:
                out.append((time.perf_counter() - t0) * 1e3)
        return float(np.median(out))

    rows, ok = [], True
    with pkg.Context(0) as c, pkg.Context(0) as fresh:
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
            return float(np.median(ms)), [np.asarray(p).copy() for p in x.download_color()]

        small = W.mesh_room(2)
        for sub in [int(s) for s in a.subdivisions.split(",")]:
            spheres, tris, planes = W.mesh_room(sub)
            c.set_scene_mesh(spheres, small[1], planes)
            c.synchronize()
            set_ms = median_of(lambda: (fresh.set_scene_mesh(spheres, tris, planes), fresh.synchronize()))
            host_ms = median_of(lambda: (c.set_mesh_triangles(tris), c.synchronize()))
            d = torch.from_numpy(np.ascontiguousarray(tris).view(np.float32).reshape(-1, 15).copy()).to("cuda:0").contiguous()
            torch.cuda.synchronize()
            device_ms = median_of(lambda: (c.set_mesh_triangles(d), c.synchronize()))
            host_tree_ms, want = render_ms(fresh)
            device_tree_ms, got = render_ms(c)
            same = all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(got, want))
            row = {"subdivisions": sub, "triangles": int(len(tris)), "set_scene_mesh_ms": round(set_ms, 3), "set_mesh_triangles_host_ms": round(host_ms, 3),
                   "set_mesh_triangles_device_ms": round(device_ms, 3), "set_scene_over_device_build": round(set_ms / device_ms, 2),
                   "render_ms_host_tree": round(host_tree_ms, 3), "render_ms_device_tree": round(device_tree_ms, 3),
                   "device_tree_over_host_tree": round(device_tree_ms / host_tree_ms, 3), "images_equal": bool(same)}
            if not same or (sub >= 6 and not device_ms < 0.98 * set_ms):
                ok = False
            print("subdivisions %d, %8d triangles: set_scene_mesh %9.3f ms | set_mesh_triangles from host %8.3f ms, from a device tensor %8.3f ms (%.2fx) | "
                  "render %8.3f ms over the host's tree, %8.3f ms over the device's (x %.3f), images %s" % (
                      sub, len(tris), set_ms, host_ms, device_ms, set_ms / device_ms, host_tree_ms, device_tree_ms, device_tree_ms / host_tree_ms,
                      "equal" if same else "DIFFER"), flush=True)
            rows.append(row)
    res = {"tool": "mesh_build_bench", "build_id": B.load_library().build_id, "shape": [a.width, a.height], "spp": a.spp, "limit": a.limit,
           "reps": a.reps, "warmup": a.warmup, "gate_device_build_below_set_scene_by_2_percent_at_6_and_8": ok, "rows": rows}
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
