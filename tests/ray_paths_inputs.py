"""Scenes, batches and the reference for the path entries (ptmi_trace_paths_device): shared by tests/test_ray_paths_inputs.py (no GPU: the
batches exercise what they are meant to) and tests/ray_paths_driver.py (the device against the reference).

Five scenes, one per kernel: mainScene (linear, staged in LDS, no shared-xy run), the 16-primitive bench scene (staged, with runs), a
sphere field just past what is staged in LDS (scalar loads), bvh_rays.adversarial_scene(3000) as a BVH scene and world.mesh_room(3) with
one plane as a mesh scene.  Each has 4 096 rays: half the primary rays of world.initial_camera() over a 64 x 32 image, 640 light probes
(rays from around the camera towards points of the scene's emissive primitives, so that light is carried back in the scenes whose lamps
are small) and the scene's adversarial families for the rest (tests/bvh_rays.py, tests/mesh_rays.py: grazing, on surfaces, off-length
directions, far and non-finite origins).

The reference is tests/cxx/ray_paths_reference.c: the loop ora_render_inline_ex runs for a pixel over ora_trace_inline, linked against
the oracle, or against the mesh reference library (tests/mesh_rays.py: reference_lib) for the mesh scene."""
import ctypes as C
import os
import subprocess

import numpy as np

import __graft_entry__ as graft
import bvh_rays
import mesh_rays

pkg = graft.load_package()
W = pkg.world
HERE = os.path.dirname(os.path.abspath(__file__))
KINDS = ["main", "s16", "big", "bvh", "mesh"]
N_RAYS = 4096
CAMERA_IMAGE = (64, 32)                                    # the camera half of a batch
SEED0 = 0x5EED1234
MAX_SCENE_LDS = 3 * 1024                                   # csrc/ptmi_device.h: kMaxSceneLds


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def packed_bytes(spheres, planes):
    """bytes of a linear scene as the kernels stage it: (3 ns + 4 np) float4"""
    return 16 * (3 * len(spheres) + 4 * len(planes))


def scene(kind):
    """-> (spheres, triangles or None, planes)"""
    if kind == "main":
        s, p = W.main_scene()
        return s, None, p
    if kind == "s16":
        s, p = W.scene16()
        return s, None, p
    if kind == "big":                                       # the smallest sphere field that is not staged in LDS
        s, p = W.sphere_field(59, seed=11)
        assert packed_bytes(s[:-1], p) <= MAX_SCENE_LDS < packed_bytes(s, p)
        return s, None, p
    if kind == "bvh":
        s, p = bvh_rays.adversarial_scene(3000)
        return s, None, p
    assert kind == "mesh", kind
    s, t, _ = W.mesh_room(3, seed=7)                        # tests/test_gpu_mesh_renders.py: scene
    p = np.array([W.plane((0.0, -2.5, 0.0), (0.0, 1.0, 0.0), (0.6, 0.8, 0.6), 0.0, W.MATTE, 0.9)], dtype=W.PLANE_DTYPE)
    return s, t, p


class Reference:
    """The reference libraries, built once into out_dir"""

    def __init__(self, out_dir):
        import oracle as ora
        ora.build()
        self.ora = ora
        self.mesh_lib = mesh_rays.reference_lib(out_dir)
        src = os.path.join(HERE, "cxx", "ray_paths_reference.c")
        flags = ["gcc", "-O2", "-std=c11", "-fPIC", "-shared", "-ffp-contract=off", "-fno-fast-math", "-fno-math-errno", "-fopenmp", "-Wall", "-Werror"]
        self.libs = {}
        for name, against in (("spheres", ora.LIB), ("mesh", os.path.join(str(out_dir), "libmesh_reference.so"))):
            out = os.path.join(str(out_dir), "libray_paths_reference_%s.so" % name)
            res = subprocess.run(flags + [src, "-o", out, against, "-Wl,-rpath," + os.path.dirname(against), "-lm"], capture_output=True, text=True)
            assert res.returncode == 0, res.stdout + res.stderr
            self.libs[name] = C.CDLL(out)
            self.libs[name].ray_paths_reference.restype = None
            self.libs[name].ray_paths_primaries.restype = None

    def primaries(self, camera, width, height):
        """the oracle's primary_ray of every pixel, row by row -> (width * height, 6) float32"""
        cam = np.ascontiguousarray(camera, self.ora.CAMERA_DTYPE)
        rays = np.zeros((width * height, 6), np.float32)
        self.libs["spheres"].ray_paths_primaries(_p(cam), width, height, _p(rays))
        return rays

    def seeds(self, n, seed0=SEED0, first_index=0):
        """ora_gen_seeds -> (n, 4) uint32: a, b, c, counter per ray"""
        return np.ascontiguousarray(np.stack(self.ora.gen_seeds(seed0, first_index, n), 1))

    def trace(self, sc, rays, color, seeds, limit, spp):
        """-> (color, seeds, live_min, live_max) after spp samples of traceInline along every ray; the inputs are left as they are"""
        spheres, triangles, planes = sc
        s = np.ascontiguousarray(spheres, self.ora.SPHERE_DTYPE)
        p = np.ascontiguousarray(planes, self.ora.PLANE_DTYPE)
        rays = np.ascontiguousarray(rays, np.float32)
        n = len(rays)
        color = np.array(color, np.float32, copy=True).reshape(n, 3)
        seeds = np.array(seeds, copy=True).view(np.uint32).reshape(n, 4)
        lo, hi = np.zeros(n, np.int32), np.zeros(n, np.int32)
        lib = self.libs["spheres"]
        if triangles is not None:
            lib = self.libs["mesh"]
            t = np.ascontiguousarray(triangles, W.TRIANGLE_DTYPE)
            self.mesh_lib.mesh_reference_set(_p(t), len(t))
        lib.ray_paths_reference(int(limit), int(spp), _p(s) if len(s) else None, len(s), _p(p) if len(p) else None, len(p), _p(rays), n, _p(color), _p(seeds),
                                _p(lo), _p(hi))
        return color, seeds, lo, hi


N_PROBES = 640


def light_probes(sc, n, seed=5):
    """n rays from within a unit of the camera towards points of the emissive primitives (sphere centres, points of emissive planes a few
    units from their position, points of emissive triangles) -> (n, 6) float32, unit directions"""
    spheres, triangles, planes = sc
    rng = np.random.default_rng(seed)
    targets = [spheres["position"][spheres["illuminance"] > 0].astype(np.float64)]
    for pl in planes[planes["illuminance"] > 0]:
        targets.append(pl["position"].astype(np.float64) + np.cross(rng.normal(size=(4, 3)), pl["direction"].astype(np.float64)) * 3.0)
    if triangles is not None:
        for t in triangles[triangles["illuminance"] > 0]:
            b = rng.dirichlet((1.0, 1.0, 1.0), 4)
            targets.append(b @ np.stack([t["v0"], t["v1"], t["v2"]]).astype(np.float64))
    targets = np.concatenate(targets)
    assert len(targets) > 0
    origin = np.asarray(W.initial_camera()["position"], np.float64).reshape(3) + rng.uniform(-1.0, 1.0, (n, 3))
    d = targets[rng.integers(0, len(targets), n)] - origin
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return np.hstack([origin, d]).astype(np.float32)


def batch(kind, sc, ref):
    """The scene's 4 096 rays: camera primaries, the light probes, then the adversarial families"""
    spheres, triangles, _ = sc
    w, h = CAMERA_IMAGE
    cam = np.concatenate([ref.primaries(W.initial_camera(), w, h), light_probes(sc, N_PROBES)])
    rest = N_RAYS - len(cam)
    if triangles is not None:
        adv = np.concatenate([mesh_rays.adversarial_rays(triangles, rest - 512, seed=3), bvh_rays.adversarial_rays(spheres, 512, seed=3)])
    else:
        adv = bvh_rays.adversarial_rays(spheres, rest, seed=3)
    rays = np.ascontiguousarray(np.concatenate([cam, adv]), np.float32)
    assert rays.shape == (N_RAYS, 6)
    return rays
