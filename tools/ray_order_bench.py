#!/usr/bin/env python3
"""ray_order_bench.py -- what ordering a batch of rays (ptmi_ray_order_device) and tracing it through the order
(ptmi_trace_rays_indexed_device, ptmi_occluded_indexed_device) costs and saves, against the PLAIN queries of a baseline library built from
the parent commit (--baseline-lib), in one session on one device.  ray_query_bench.py's three scenes -- S16, world.sphere_field(10^5) as a
BVH scene, world.mesh_room(8) (1.3 M triangles) as a mesh scene -- at 1920 x 1080 rays, and three batches:
  coherent  one ray per pixel of a pinhole camera, in image order (ray_query_bench.camera_rays);
  shuffled  the same rays in a seeded random order;
  bounce    one diffuse bounce of the coherent batch, made with torch on the device from a seed: a ray that hit starts at its hit position
            pushed 2^-10 along the normal (turned against the incoming ray) and leaves by a cosine-hemisphere draw; a ray that missed stays.
Per scene, batch and query (closest hit without the record; occlusion with t_max = +inf), the time per call of
  baseline_plain    the parent library's plain query           plain            this library's plain query
  order             ptmi_ray_order_device alone                 indexed_order    the indexed query through that order
  indexed_identity  the indexed query through 0 .. n - 1: the price of the indirection
and from them order + indexed_order against baseline_plain (a batch ordered once and traced once) and indexed_order against
baseline_plain (an order that is reused: fixed sensor beams over a moving scene).

Timing (device events on the caller's stream, which both contexts launch on): --warmup calls of every variant, then --reps rounds; a round
times every variant in turn, --inner calls between two events each, so the variants alternate and share whatever else the device is
doing; the median window / inner is the time per call.  Before any timing the indexed answers through the order are compared with the
plain ones bit for bit, and this library's plain answers with the baseline's.
Usage: tools/ray_order_bench.py --baseline-lib PATH [--reps 10] [--inner 10] [--warmup 3] [--scenes s16,field,mesh] [--out profiles/ray_order_bench.json]"""
import argparse
import ctypes as C
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from ray_query_bench import camera_rays  # noqa: E402


def open_baseline(B, path):
    """A library of OTHER sources (the parent commit's): every symbol of the binding that it exports, typed; the ones it lacks are not touched"""
    lib = C.CDLL(path)
    for name, (res, args) in B.SYMBOLS.items():
        if hasattr(lib, name):
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, args
    lib.build_id = (lib.ptmi_build_id() or b"").decode("ascii", "replace")
    return lib


def bounce_rays(torch, rays, t, idx, rec, seed):
    """One diffuse bounce of `rays` from their hit records (device tensors) -> (n, 6) device rays"""
    gen = torch.Generator(device="cuda")
    gen.manual_seed(seed)
    n = rays.shape[0]
    d, pos, nrm = rays[:, 3:], rec[:, :3], rec[:, 3:]
    nrm = torch.where(((nrm * d).sum(1, keepdim=True) > 0), -nrm, nrm)
    u = torch.rand((n, 2), generator=gen, device="cuda", dtype=torch.float32)
    r, phi = torch.sqrt(u[:, 0]), (2.0 * math.pi) * u[:, 1]
    local = torch.stack([r * torch.cos(phi), r * torch.sin(phi), torch.sqrt(torch.clamp(1.0 - u[:, 0], min=0.0))], 1)
    helper = torch.where((nrm[:, 0:1].abs() < 0.5), torch.tensor([1.0, 0.0, 0.0], device="cuda"), torch.tensor([0.0, 1.0, 0.0], device="cuda"))
    tangent = torch.linalg.cross(helper.expand(n, 3), nrm)
    tangent = tangent / tangent.norm(dim=1, keepdim=True)
    bitangent = torch.linalg.cross(nrm, tangent)
    out_d = local[:, 0:1] * tangent + local[:, 1:2] * bitangent + local[:, 2:3] * nrm
    out_d = out_d / out_d.norm(dim=1, keepdim=True)
    bounced = torch.cat([pos + nrm * (2.0 ** -10), out_d], 1)
    hit = (idx >= 0)[:, None] & torch.isfinite(bounced).all(1, keepdim=True)
    return torch.where(hit, bounced, rays).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--baseline-lib", required=True, help="libptmi.so built from the parent commit")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
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
    base_lib = open_baseline(B, a.baseline_lib)
    this_lib = B.load_library()
    assert base_lib.build_id != this_lib.build_id, "the baseline library is this library"
    n = a.width * a.height
    stream = torch.cuda.Stream()
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

    def same(x, y):
        return torch.equal(x.view(torch.int32), y.view(torch.int32))

    with pkg.Context(0) as c, pkg.Context(0, library=base_lib) as base:
        for ctx in (c, base):
            ctx.set_stream(stream.cuda_stream)
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
                coherent = torch.from_numpy(camera_rays(W.initial_camera(), a.width, a.height)).to("cuda")
                perm = torch.from_numpy(np.random.default_rng(1).permutation(n)).to("cuda")
                t, idx, rec = c.trace_rays(coherent, hit=True)
                batches = (("coherent", coherent), ("shuffled", coherent[perm].contiguous()), ("bounce", bounce_rays(torch, coherent, t, idx, rec, seed=2)))
                d_inf = torch.full((n,), float("inf"), dtype=torch.float32, device="cuda")
                identity = torch.arange(n, dtype=torch.int32, device="cuda")
                order = torch.empty(n, dtype=torch.int32, device="cuda")
                work = torch.empty(B.ray_order_bytes(n), dtype=torch.uint8, device="cuda")
                outs = [(torch.empty(n, dtype=torch.float32, device="cuda"), torch.empty(n, dtype=torch.int32, device="cuda")) for _ in range(3)]
                occs = [torch.empty(n, dtype=torch.int32, device="cuda") for _ in range(3)]
                for batch, rays in batches:
                    c.ray_order(rays, out=order, work=work)
                    # the answers, before any timing
                    base.trace_rays(rays, out=outs[0])
                    c.trace_rays(rays, out=outs[1])
                    outs[2][0].fill_(-1.0)
                    outs[2][1].fill_(-7)
                    c.trace_rays(rays, out=outs[2], index=order)
                    base.occluded(rays, d_inf, out=occs[0])
                    c.occluded(rays, d_inf, out=occs[1])
                    occs[2].fill_(-7)
                    c.occluded(rays, d_inf, out=occs[2], index=order)
                    stream.synchronize()
                    assert bool((torch.sort(order.long()).values == torch.arange(n, device="cuda")).all()), "the order is not a permutation"
                    for k in (1, 2):
                        assert same(outs[k][0], outs[0][0]) and same(outs[k][1], outs[0][1]) and same(occs[k], occs[0]), (name, batch, k)
                    figures = {}
                    for query, calls in (("closest", {"baseline_plain": lambda: base.trace_rays(rays, out=outs[0]),
                                                      "plain": lambda: c.trace_rays(rays, out=outs[1]),
                                                      "order": lambda: c.ray_order(rays, out=order, work=work),
                                                      "indexed_order": lambda: c.trace_rays(rays, out=outs[2], index=order),
                                                      "indexed_identity": lambda: c.trace_rays(rays, out=outs[2], index=identity)}),
                                         ("occluded", {"baseline_plain": lambda: base.occluded(rays, d_inf, out=occs[0]),
                                                       "plain": lambda: c.occluded(rays, d_inf, out=occs[1]),
                                                       "order": lambda: c.ray_order(rays, out=order, work=work),
                                                       "indexed_order": lambda: c.occluded(rays, d_inf, out=occs[2], index=order),
                                                       "indexed_identity": lambda: c.occluded(rays, d_inf, out=occs[2], index=identity)})):
                        figures[query] = timed(calls)
                    row = {"scene": name, "primitives": prims, "rays": batch, "n_rays": n, "hit_share": round(float((outs[0][1] >= 0).float().mean().item()), 4)}
                    for query, f in figures.items():
                        for key, (med, lo, hi) in f.items():
                            row["%s_%s_ms" % (query, key)], row["%s_%s_ms_min" % (query, key)], row["%s_%s_ms_max" % (query, key)] = round(med, 4), round(lo, 4), round(hi, 4)
                        ref = f["baseline_plain"][0]
                        row[query + "_order_plus_indexed_over_baseline"] = round((f["order"][0] + f["indexed_order"][0]) / ref, 3)
                        row[query + "_indexed_over_baseline"] = round(f["indexed_order"][0] / ref, 3)
                        row[query + "_identity_over_baseline"] = round(f["indexed_identity"][0] / ref, 3)
                        row[query + "_plain_over_baseline"] = round(f["plain"][0] / ref, 3)
                    rows.append(row)
                    print("%-5s %-8s closest: baseline %7.3f plain %7.3f order %7.3f indexed %7.3f identity %7.3f ms | occluded: baseline %7.3f indexed %7.3f identity %7.3f ms" % (
                        name, batch, row["closest_baseline_plain_ms"], row["closest_plain_ms"], row["closest_order_ms"], row["closest_indexed_order_ms"],
                        row["closest_indexed_identity_ms"], row["occluded_baseline_plain_ms"], row["occluded_indexed_order_ms"], row["occluded_indexed_identity_ms"]), flush=True)
        torch.cuda.synchronize()
        for ctx in (c, base):
            ctx.set_stream(None)
    res = {"tool": "ray_order_bench", "build_id": this_lib.build_id, "baseline_build_id": base_lib.build_id, "device": torch.cuda.get_device_name(0),
           "shape": [a.width, a.height], "reps": a.reps, "inner": a.inner, "warmup": a.warmup, "rows": rows}
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
