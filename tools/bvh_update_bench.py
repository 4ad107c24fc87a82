#!/usr/bin/env python3
"""bvh_update_bench.py -- moving and replacing a BVH scene's spheres on the device: ptmi_update_spheres (the hierarchy refitted) and
ptmi_set_bvh_spheres (the hierarchy built on the device) against ptmi_set_scene_bvh (built on the host), on world.sphere_field at
1 020, 10^5 and 10^6 spheres.  Per scene, each figure the median of --reps after --warmup:
  (a) wall time of set_scene_bvh;
  (b) wall time of update_spheres from host memory and (c) from a device tensor (each followed by a synchronize);
  (d) wall time of set_bvh_spheres from host memory and (e) from a device tensor;
  (f) render Inline, 1920 x 1080, 8 samples per pixel, bounce limit 8, over ptmi_bvh_layout's tree (longest-axis median splits);
  (g) the same render over that tree REFITTED after a per-sphere displacement of a tenth of the field's width, against (f') the render
      over ptmi_bvh_layout's tree of the displaced spheres -- the same image, another tree;
  (h) the same render over the device-built tree (Morton order, equal-count splits), against (f);
  (d'), (e'), (h') the same three for the SPATIAL device build (PTMI_OPT_BVH_DEVICE_BUILD = PTMI_BVH_BUILD_SPATIAL: cubic cells, splits at
      the highest differing key bit), in the same session as (d), (e), (h) -- whose builder is the one every earlier version had -- with
      the spatial tree's depth, node count and the share of its nodes that fell back to the equal-count split (counted by the numpy
      restatement of tests/bvh_spatial_scenes.py, which the tests hold equal to the device's tree).
No ratio is a gate: the figures are what they are.
Usage: tools/bvh_update_bench.py [--reps 5] [--warmup 2] [--spheres 1020,100000,1000000] [--out FILE]
(profiles/bvh_update_bench.json: the run before the spatial build existed; profiles/bvh_spatial_bench.json: with it)"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--spheres", default="1020,100000,1000000")
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

    rows, same_all = [], True
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

        def equal(got, want):
            return all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(got, want))

        for n in [int(s) for s in a.spheres.split(",")]:
            s, p = W.sphere_field(n, seed=24)
            g = W.sphere_geometry(s)
            width = float(np.ptp(s["position"][:, 0]))
            g2 = W.displaced_spheres(g, 0.1 * width, "noise", seed=1)
            s2 = W.with_sphere_geometry(s, g2)
            set_ms = median_of(lambda: (fresh.set_scene_bvh(s, p), fresh.synchronize()))
            c.set_scene_bvh(s, p)
            c.synchronize()
            upd_host_ms = median_of(lambda: (c.update_spheres(g), c.synchronize()))
            d4 = torch.from_numpy(g).to("cuda:0").contiguous()
            d10 = torch.from_numpy(np.ascontiguousarray(s).view(np.float32).reshape(-1, 10).copy()).to("cuda:0").contiguous()
            torch.cuda.synchronize()
            upd_dev_ms = median_of(lambda: (c.update_spheres(d4), c.synchronize()))
            host_tree_ms, want = render_ms(fresh)
            # the refitted tree after a large displacement, against the host's tree of the displaced spheres
            c.update_spheres(g2)
            refit_ms, got = render_ms(c)
            fresh.set_scene_bvh(s2, p)
            moved_tree_ms, want2 = render_ms(fresh)
            same = equal(got, want2)
            set_host_ms = median_of(lambda: (c.set_bvh_spheres(s), c.synchronize()))
            set_dev_ms = median_of(lambda: (c.set_bvh_spheres(d10), c.synchronize()))
            morton_ms, got = render_ms(c)
            same = same and equal(got, want)
            c.set_option(B.OPT_BVH_DEVICE_BUILD, B.BVH_BUILD_SPATIAL)
            spatial_host_ms = median_of(lambda: (c.set_bvh_spheres(s), c.synchronize()))
            spatial_dev_ms = median_of(lambda: (c.set_bvh_spheres(d10), c.synchronize()))
            spatial_ms, got = render_ms(c)
            c.set_option(B.OPT_BVH_DEVICE_BUILD, B.BVH_BUILD_EQUAL_COUNT)
            same = same and equal(got, want)
            import bvh_spatial_scenes as spatial
            _, _, level_first, fallbacks = spatial.restate(s)
            same = same and c.bvh_read_layout()[0].shape[0] == level_first[-1]
            same_all = same_all and same
            row = {"spheres": int(n), "set_scene_bvh_ms": round(set_ms, 3), "update_spheres_host_ms": round(upd_host_ms, 3),
                   "update_spheres_device_ms": round(upd_dev_ms, 3), "set_bvh_spheres_host_ms": round(set_host_ms, 3),
                   "set_bvh_spheres_device_ms": round(set_dev_ms, 3), "render_ms_host_tree": round(host_tree_ms, 3),
                   "render_ms_host_tree_of_moved": round(moved_tree_ms, 3), "render_ms_refitted_tree": round(refit_ms, 3),
                   "refitted_over_host_tree": round(refit_ms / moved_tree_ms, 3), "render_ms_morton_tree": round(morton_ms, 3),
                   "morton_over_host_tree": round(morton_ms / host_tree_ms, 3),
                   "set_bvh_spheres_spatial_host_ms": round(spatial_host_ms, 3), "set_bvh_spheres_spatial_device_ms": round(spatial_dev_ms, 3),
                   "render_ms_spatial_tree": round(spatial_ms, 3), "spatial_over_host_tree": round(spatial_ms / host_tree_ms, 3),
                   "spatial_over_equal_count_call": round(spatial_dev_ms / set_dev_ms, 3),
                   "spatial_tree_levels": len(level_first) - 1, "spatial_tree_nodes": int(level_first[-1]),
                   "spatial_fallback_share": round(fallbacks / max(1, level_first[-1]), 6), "images_equal": bool(same)}
            print("%8d spheres: set_scene_bvh %9.3f ms | update_spheres host %8.3f ms, device %8.3f ms | set_bvh_spheres host %8.3f ms, device %8.3f ms | "
                  "render %8.3f ms over the host's tree, refitted x %.3f, Morton x %.3f, images %s" % (
                      n, set_ms, upd_host_ms, upd_dev_ms, set_host_ms, set_dev_ms, host_tree_ms, refit_ms / moved_tree_ms, morton_ms / host_tree_ms,
                      "equal" if same else "DIFFER"), flush=True)
            print("%8d spheres: spatial build host %8.3f ms, device %8.3f ms (x %.3f of the equal-count build) | render x %.3f of the host's tree | %d levels, "
                  "%d nodes, %d fell back" % (n, spatial_host_ms, spatial_dev_ms, spatial_dev_ms / set_dev_ms, spatial_ms / host_tree_ms, len(level_first) - 1,
                                              level_first[-1], fallbacks), flush=True)
            rows.append(row)
            del d4, d10
    res = {"tool": "bvh_update_bench", "build_id": B.load_library().build_id, "shape": [a.width, a.height], "spp": a.spp, "limit": a.limit,
           "reps": a.reps, "warmup": a.warmup, "images_equal": same_all, "rows": rows}
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)
    return 0 if same_all else 1


if __name__ == "__main__":
    sys.exit(main())
