#!/usr/bin/env python3
"""ray_query_bench.py -- rays per second of the device-resident ray queries (ptmi_trace_rays_device, ptmi_occluded_device) against
ptmi_eval_check_hit from host memory, in one session.  Three scenes: S16 (16 primitives, ptmi_set_scene), world.sphere_field(10^5)
through ptmi_set_scene_bvh, world.mesh_room at its largest subdivision (8: 1.3 M triangles) through ptmi_set_scene_mesh.  Two ray sets of
1920 x 1080 rays: COHERENT -- one ray per pixel of a pinhole camera at initial_camera()'s position and angles, in image order (not the
renderer's primary rays bit for bit: its rotation goes through a quaternion) -- and INCOHERENT, the same rays shuffled.  Per scene and
ray set: closest hit without and with the hit record; occlusion with t_max = +inf (every ray that hits anything is occluded: the early
exit at work) and with t_max = the closest hit's own t (no ray is occluded: the walk must look at everything nearer); and
ptmi_eval_check_hit (host clock around the call, which stages, synchronises and copies back).

Timing (device events on the caller's stream, which the context launches on): --warmup calls, then --reps windows of --inner calls each
between two events; the median window / inner is the time per call.  Before any timing the answers are compared with
ptmi_eval_check_hit's (t and idx bit for bit) and with the occlusion's specification.
Usage: tools/ray_query_bench.py [--reps 10] [--inner 10] [--warmup 3] [--scenes s16,field,mesh] [--out profiles/ray_query_bench.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def camera_rays(cam, width, height):
    """One ray per pixel, row-major: a pinhole at the camera's position, horizontal field of view cam.fov, turned by its (roll, pitch, yaw)"""
    half = np.tan(np.radians(float(cam["fov"])) / 2.0)
    x = ((np.arange(width) + 0.5) / width * 2.0 - 1.0) * half
    y = (1.0 - (np.arange(height) + 0.5) / height * 2.0) * half * height / width
    d = np.stack(np.broadcast_arrays(x[None, :], y[:, None], -1.0), -1).reshape(-1, 3)
    roll, pitch, yaw = (float(a) for a in cam["rotation"])
    cz, sz, cx, sx, cy, sy = np.cos(roll), np.sin(roll), np.cos(pitch), np.sin(pitch), np.cos(yaw), np.sin(yaw)
    rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    d = d @ (ry @ rx @ rz).T
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    o = np.broadcast_to(np.asarray(cam["position"], np.float64), d.shape)
    return np.ascontiguousarray(np.hstack([o, d]), np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-reps", type=int, default=3)
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
    cam = W.initial_camera()
    n = a.width * a.height
    coherent = camera_rays(cam, a.width, a.height)
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
                t0 = time.perf_counter()
                e_t, e_idx, _ = c.eval_check_hit(rays)
                host_ms = [1e3 * (time.perf_counter() - t0)]
                for _ in range(a.host_reps):
                    t0 = time.perf_counter()
                    c.eval_check_hit(rays)
                    host_ms.append(1e3 * (time.perf_counter() - t0))
                hit = e_idx >= 0
                t_own = np.where(hit, e_t, np.float32(np.inf)).astype(np.float32)
                with torch.cuda.stream(stream):
                    d_rays = torch.from_numpy(rays).to("cuda")
                    d_inf = torch.full((n,), float("inf"), dtype=torch.float32, device="cuda")
                    d_own = torch.from_numpy(t_own).to("cuda")
                    t, idx, rec = (torch.empty(n, dtype=torch.float32, device="cuda"), torch.empty(n, dtype=torch.int32, device="cuda"),
                                   torch.empty((n, 6), dtype=torch.float32, device="cuda"))
                    occ = torch.empty(n, dtype=torch.int32, device="cuda")
                    # the answers, before any timing
                    c.trace_rays(d_rays, out=(t, idx, rec))
                    stream.synchronize()
                    assert np.array_equal(t.cpu().numpy().view(np.uint32), e_t.view(np.uint32)) and np.array_equal(idx.cpu().numpy(), e_idx), "closest hit"
                    c.occluded(d_rays, d_inf, out=occ)
                    stream.synchronize()
                    assert np.array_equal(occ.cpu().numpy(), (hit & (e_t < np.inf)).astype(np.int32)), "occluded, t_max = inf"
                    occluded_share = float(occ.sum().item()) / n
                    c.occluded(d_rays, d_own, out=occ)
                    stream.synchronize()
                    assert int(occ.sum().item()) == 0, "occluded, t_max = t"
                    figures = {"closest": timed(lambda: c.trace_rays(d_rays, out=(t, idx))),
                               "closest_with_record": timed(lambda: c.trace_rays(d_rays, out=(t, idx, rec))),
                               "occluded_most": timed(lambda: c.occluded(d_rays, d_inf, out=occ)),
                               "occluded_none": timed(lambda: c.occluded(d_rays, d_own, out=occ))}
                row = {"scene": name, "primitives": prims, "rays": rays_name, "n_rays": n, "hit_share": round(float(hit.mean()), 4),
                       "occluded_share_at_inf": round(occluded_share, 4),
                       "eval_check_hit_host_ms": round(float(np.median(host_ms[1:])), 3), "eval_check_hit_host_mrays_per_s": round(n / np.median(host_ms[1:]) / 1e3, 1)}
                for key, (med, lo, hi) in figures.items():
                    row[key + "_ms"], row[key + "_ms_min"], row[key + "_ms_max"] = round(med, 4), round(lo, 4), round(hi, 4)
                    row[key + "_mrays_per_s"] = round(n / med / 1e3, 1)
                rows.append(row)
                print("%-5s %-10s closest %8.1f (with record %8.1f)  occluded: most %8.1f none %8.1f  eval_check_hit from host %7.1f  Mrays/s" % (
                    name, rays_name, row["closest_mrays_per_s"], row["closest_with_record_mrays_per_s"], row["occluded_most_mrays_per_s"],
                    row["occluded_none_mrays_per_s"], row["eval_check_hit_host_mrays_per_s"]), flush=True)
        torch.cuda.synchronize()
        c.set_stream(None)
    res = {"tool": "ray_query_bench", "build_id": B.load_library().build_id, "device": torch.cuda.get_device_name(0), "shape": [a.width, a.height],
           "reps": a.reps, "inner": a.inner, "warmup": a.warmup, "rows": rows}
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
