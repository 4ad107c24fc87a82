"""The reference for the stepped path entries (ptmi_bounce_rays_device, ptmi_live_rays_device): shared by tests/test_ray_bounce_inputs.py
(no GPU: the restatement is the oracle's traceInline, and the batches exercise the step) and tests/ray_bounce_driver.py (the device
against the reference).

The scenes, their 4 096 rays and the seeds are tests/ray_paths_inputs.py's.  The step's reference is tests/cxx/ray_bounce_reference.c: one
prepareRay over ora_near_zero_v3, ora_check_hit and ora_calc_next_ray, linked against the oracle, or against the mesh reference library
(tests/mesh_rays.py: reference_lib) for the mesh scene -- as ray_paths_reference.c is.  The live list's reference is a numpy statement of
its definition (live_list)."""
import ctypes as C
import os
import subprocess

import numpy as np

import ray_paths_inputs as paths
from ray_paths_inputs import KINDS, N_RAYS, SEED0, W, _p, batch, scene  # noqa: F401

HERE = os.path.dirname(os.path.abspath(__file__))
STEPS = 8
FROZEN, MISSED, HIT = 0, 1, 2                               # ray_bounce_reference.c: BOUNCE_*


class Reference(paths.Reference):
    """ray_paths_inputs' reference libraries and the step's, built once into out_dir"""

    def __init__(self, out_dir):
        super().__init__(out_dir)
        src = os.path.join(HERE, "cxx", "ray_bounce_reference.c")
        flags = ["gcc", "-O2", "-std=c11", "-fPIC", "-shared", "-ffp-contract=off", "-fno-fast-math", "-fno-math-errno", "-fopenmp", "-Wall", "-Werror"]
        self.step_libs = {}
        for name, against in (("spheres", self.ora.LIB), ("mesh", os.path.join(str(out_dir), "libmesh_reference.so"))):
            out = os.path.join(str(out_dir), "libray_bounce_reference_%s.so" % name)
            res = subprocess.run(flags + [src, "-o", out, against, "-Wl,-rpath," + os.path.dirname(against), "-lm"], capture_output=True, text=True)
            assert res.returncode == 0, res.stdout + res.stderr
            self.step_libs[name] = C.CDLL(out)
            self.step_libs[name].ray_bounce_reference.restype = None

    def step(self, sc, rays, throughput, radiance, seeds):
        """One prepareRay for every ray -> (rays, throughput, radiance, seeds, outcome, hit): new arrays, the inputs are left as they are"""
        spheres, triangles, planes = sc
        s = np.ascontiguousarray(spheres, self.ora.SPHERE_DTYPE)
        p = np.ascontiguousarray(planes, self.ora.PLANE_DTYPE)
        n = len(rays)
        rays = np.array(rays, np.float32, copy=True).reshape(n, 6)
        throughput = np.array(throughput, np.float32, copy=True).reshape(n, 3)
        radiance = np.array(radiance, np.float32, copy=True).reshape(n, 3)
        seeds = np.array(seeds, copy=True).view(np.uint32).reshape(n, 4)
        outcome, hit = np.zeros(n, np.int32), np.zeros((n, 6), np.float32)
        lib = self.step_libs["spheres"]
        if triangles is not None:
            lib = self.step_libs["mesh"]
            t = np.ascontiguousarray(triangles, W.TRIANGLE_DTYPE)
            self.mesh_lib.mesh_reference_set(_p(t), len(t))
        lib.ray_bounce_reference(_p(s) if len(s) else None, len(s), _p(p) if len(p) else None, len(p), _p(rays), n, _p(throughput), _p(radiance), _p(seeds),
                                 _p(outcome), _p(hit))
        return rays, throughput, radiance, seeds, outcome, hit

    def steps(self, sc, rays, k=STEPS):
        """The states after 1 .. k steps from throughput 1, radiance 0 and genSeeds(SEED0) -> [step()'s tuple per step]"""
        n = len(rays)
        state = (rays, np.ones((n, 3), np.float32), np.zeros((n, 3), np.float32), self.seeds(n))
        out = []
        for _ in range(k):
            got = self.step(sc, *state)
            out.append(got)
            state = got[:4]
        return out


def near_zero(throughput):
    """linear's nearZero of every row of an (n, 3) float32 array, in binary32 and in the oracle's association: (x x + y y) + z z <= 1e-6"""
    t = np.asarray(throughput, np.float32)
    with np.errstate(all="ignore"):
        d = (t[:, 0] * t[:, 0] + t[:, 1] * t[:, 1]).astype(np.float32) + t[:, 2] * t[:, 2]
        return np.abs(d.astype(np.float32)) <= np.float32(1e-6)


def live_list(throughput, index=None):
    """The definition of ptmi_live_rays: the candidates -- index's entries, or 0 .. n - 1 -- inside [0, n) whose throughput is not nearZero,
    in candidate order, then -1 up to the candidate count -> (live int32, count)"""
    n = len(throughput)
    cand = np.arange(n, dtype=np.int64) if index is None else np.asarray(index, np.int64)
    inside = (cand >= 0) & (cand < n)
    alive = np.zeros(len(cand), bool)
    alive[inside] = ~near_zero(np.asarray(throughput, np.float32).reshape(n, 3)[cand[inside]])
    live = np.full(len(cand), -1, np.int32)
    live[:alive.sum()] = cand[alive]
    return live, int(alive.sum())
