"""Scenes, batches and the reference for render Streams along a caller's rays (ptmi_trace_streams_device): shared by
tests/test_ray_streams_reference.py (the reference against the oracle's render loops), tests/test_ray_streams_inputs.py (no GPU: the batches
reach what they are for) and tests/ray_streams_driver.py (the device against the reference).

One scene per kernel, each with and without GLASS: world.glass_scene() and world.main_scene() (linear, staged in LDS); a sphere field
just past what is staged in LDS (scalar loads), plain and with a glass fraction; bvh_rays.adversarial_scene(3000) as a BVH scene, plain and
with every third sphere of the field GLASS; world.mesh_room(3) with one plane as a mesh scene, plain and with every fourth triangle and
one sphere GLASS.  Each has 4 096 rays built like ray_paths_inputs.batch -- camera primaries, light probes, the adversarial families --
with a family of rays aimed at the scene's glass in place of the last adversarial rays (some of them off-length).  Below their ceilings
these scenes are closed -- every child of a glass hit meets something -- and five glass reflections in a row are rare, so each GLASS scene
also carries with_sky's glass outside the enclosure and a family of rays out there (sky_rays).

The drop scene: two facing GLASS planes of ior 0.8, emissive, and grazing rays between them.  eta = 1.25, so a ray that meets a plane at
cos i < 0.6 is totally reflected: R = 1, the reflection child goes on with the whole throughput and a dead refraction child is pushed at
every hit of the lineage -- more than 16 of them long before nearZero ends it (colour 0.95: about 140 hits).

The reference is tests/cxx/ray_streams_reference.c, linked against the oracle, or against the mesh reference library for the mesh scene."""
import ctypes as C
import os
import subprocess

import numpy as np

import ray_paths_inputs as paths

W = paths.W
HERE = os.path.dirname(os.path.abspath(__file__))
PLAIN = ["main", "big", "bvh", "mesh"]
GLASS = ["glass", "big_glass", "bvh_glass", "mesh_glass"]
KINDS = PLAIN + GLASS + ["drop"]
N_RAYS = paths.N_RAYS
N_GLASS_RAYS = 512                                         # the family aimed at the scene's glass
N_SKY_RAYS = 256                                           # ... and the one outside the enclosure (with_sky)
N_DROP_RAYS = 512
STACK_DEPTH = 16                                           # csrc/ptmi_kernels.h: kTreeStackDepth
FAST_LEVELS = 4                                            # ... kTreeFastLevels
DEFAULT_CAP = 1 << 16                                      # PTMI_OPT_STREAM_STEP_CAP's default
DIAG = ["glass_hits", "deepest", "dropped", "truncated", "hits", "first_glass", "first_children", "glass_below"]
SEED0 = paths.SEED0


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def has_glass(kind):
    return kind in GLASS or kind == "drop"


SKY_SPHERE = ((3001.0, 40.0, -10.0), 3.0)                  # centre, radius: clear of the BVH scene's sphere of radius 1000 overhead
TRAP_PLANES_Y = (-102.0, -100.0)                         # far below the floor


def with_sky(sc):
    """The scene with GLASS outside its enclosure, where a child can miss and a lineage can be long: a glass sphere above the ceiling, met
    from out there, whose reflection and refraction children go up (and hit nothing) or down into the scene; and, far below the floor, the
    drop scene's two facing planes of ior 0.8, between which a grazing ray pushes a dead refraction child at every hit -- past
    kTreeFastLevels on every kind of scene.  Nothing inside the enclosure sees either: the ceiling and the floor are met first."""
    s, t, p = sc
    sky = np.array([W.sphere(SKY_SPHERE[0], SKY_SPHERE[1], (0.95, 0.95, 0.95), 0.0, W.GLASS, 1.5)], dtype=W.SPHERE_DTYPE)
    planes = np.array([W.plane((0.0, TRAP_PLANES_Y[0], 0.0), (0.0, 1.0, 0.0), (0.95, 0.95, 0.95), 0.25, W.GLASS, 0.8),
                       W.plane((0.0, TRAP_PLANES_Y[1], 0.0), (0.0, -1.0, 0.0), (0.95, 0.95, 0.95), 0.5, W.GLASS, 0.8)], dtype=W.PLANE_DTYPE)
    return np.concatenate([s, sky]), t, np.concatenate([p, planes])


def scene(kind):
    """-> (spheres, triangles or None, planes)"""
    if kind in GLASS:
        return with_sky(plain_glass_scene(kind))
    if kind == "drop":
        s = np.array([W.sphere((40.0, 0.0, 0.0), 0.5, (1.0, 0.9, 0.8), 5.0, W.MATTE, 1.0)], dtype=W.SPHERE_DTYPE)
        p = np.array([W.plane((0.0, -1.0, 0.0), (0.0, 1.0, 0.0), (0.95, 0.95, 0.95), 0.25, W.GLASS, 0.8),
                      W.plane((0.0, 1.0, 0.0), (0.0, -1.0, 0.0), (0.95, 0.95, 0.95), 0.5, W.GLASS, 0.8)], dtype=W.PLANE_DTYPE)
        return s, None, p
    return paths.scene(kind)


def plain_glass_scene(kind):
    """The GLASS scenes as the issue names them, before with_sky: what the camera tests render"""
    if kind == "glass":
        s, p = W.glass_scene()
        return s, None, p
    if kind == "big_glass":                                 # the geometry of paths.scene("big"): the glass choice is drawn last
        s, p = W.sphere_field(59, seed=11, glass_fraction=0.5)
        assert paths.packed_bytes(s, p) > paths.MAX_SCENE_LDS
        return s, None, p
    if kind == "bvh_glass":
        s, t, p = paths.scene("bvh")
        s = s.copy()
        glass = (np.arange(len(s)) % 3 == 0) & (np.abs(s["radius"]) < 100.0)
        s["brdf_tag"][glass] = W.GLASS
        s["brdf_param"][glass] = 1.5
        s["color"][glass] = (0.95, 0.95, 0.95)
        s["illuminance"][glass] = 0.0
        return s, None, p
    if kind == "mesh_glass":
        s, t, p = paths.scene("mesh")
        s, t = s.copy(), t.copy()
        glass = np.arange(len(t)) % 4 == 3
        glass[:13] = False                                  # (the room's walls and its light stay what they are)
        t["brdf_tag"][glass] = W.GLASS
        t["brdf_param"][glass] = 1.5
        t["color"][glass] = (0.95, 0.95, 0.95)
        s["brdf_tag"][1] = W.GLASS
        s["brdf_param"][1] = 1.33
        s["color"][1] = (0.95, 0.95, 0.95)
        s["illuminance"][1] = 0.0
        return s, t, p
    raise AssertionError(kind)


def sky_rays(n, seed=17):
    """n rays outside the enclosure: half between the trap planes (the drop scene's grazing rays), half from a ring around the sky sphere
    towards points of it, so that its children leave upwards (a miss) or downwards"""
    rng = np.random.default_rng(seed)
    between = drop_rays(n // 4, seed)
    between[:, 1] += np.float32(0.5 * (TRAP_PLANES_Y[0] + TRAP_PLANES_Y[1]))
    m = n - n // 4
    c, r = np.asarray(SKY_SPHERE[0], np.float64), SKY_SPHERE[1]
    phi = rng.uniform(1.05 * np.pi, 1.45 * np.pi, m)        # heading +x and +z, away from the sphere fields' two walls
    origin = c + np.stack([10.0 * np.cos(phi), rng.uniform(-8.0, 0.0, m), 10.0 * np.sin(phi)], 1)
    level = c - origin
    level /= np.linalg.norm(level, axis=1, keepdims=True)
    up = np.array([0.0, 1.0, 0.0]) - level[:, 1:2] * level   # towards the sphere's upper silhouette as the ray sees it
    up /= np.linalg.norm(up, axis=1, keepdims=True)
    off = rng.normal(size=(m, 3))
    off /= np.linalg.norm(off, axis=1, keepdims=True)
    off[::3] *= 0.8                                         # one in three anywhere on the sphere: a child goes down into the scene
    rest = np.ones(m, bool)
    rest[::3] = False                                       # the others graze the upper silhouette: both children leave upwards
    off[rest] = up[rest] * rng.choice([0.6, 0.9, 0.99], int(rest.sum()))[:, None]
    d = c + off * r - origin
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return np.concatenate([between, np.hstack([origin, d]).astype(np.float32)])


def glass_rays(sc, n, seed=9):
    """n rays from around the camera towards points of the scene's GLASS primitives (sphere centres and points near their silhouettes,
    points of glass triangles); every fourth with a direction whose length is not 1 -> (n, 6) float32"""
    spheres, triangles, planes = sc
    rng = np.random.default_rng(seed)
    targets = []
    g = spheres[spheres["brdf_tag"] == W.GLASS]
    if len(g):
        k = rng.integers(0, len(g), 4 * n)
        off = rng.normal(size=(4 * n, 3))
        off /= np.linalg.norm(off, axis=1, keepdims=True)
        targets.append(g["position"][k].astype(np.float64) + off * (g["radius"][k].astype(np.float64) * rng.choice([0.0, 0.5, 0.9, 0.99], 4 * n))[:, None])
    if triangles is not None:
        t = triangles[triangles["brdf_tag"] == W.GLASS]
        k = rng.integers(0, len(t), 4 * n)
        b = rng.dirichlet((1.0, 1.0, 1.0), 4 * n)
        targets.append(b[:, 0:1] * t["v0"][k] + b[:, 1:2] * t["v1"][k] + b[:, 2:3] * t["v2"][k])
    targets = np.concatenate(targets)
    targets = targets[rng.integers(0, len(targets), n)]
    origin = np.asarray(W.initial_camera()["position"], np.float64).reshape(3) + rng.uniform(-1.0, 1.0, (n, 3))
    d = targets - origin
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    scale = np.where(np.arange(n) % 4 == 3, rng.choice([0.5, 1.01, 3.0, 1 + 2e-4], n), 1.0)
    return np.hstack([origin, d * scale[:, None]]).astype(np.float32)


def drop_rays(n, seed=13):
    """n rays between the drop scene's planes: three in four grazing (|dy| of 0.01 to 0.3 of a unit direction: total reflection), the rest
    steep (refracted, a few hits); every eighth off-length"""
    rng = np.random.default_rng(seed)
    o = np.stack([rng.uniform(-5.0, 5.0, n), rng.uniform(-0.9, 0.9, n), rng.uniform(-5.0, 5.0, n)], 1)
    phi = rng.uniform(0.0, 2.0 * np.pi, n)
    dy = np.where(np.arange(n) % 4 == 3, rng.uniform(0.7, 1.0, n), rng.uniform(0.01, 0.3, n)) * rng.choice([-1.0, 1.0], n)
    h = np.sqrt(1.0 - dy * dy)
    d = np.stack([h * np.cos(phi), dy, h * np.sin(phi)], 1)
    scale = np.where(np.arange(n) % 8 == 5, rng.choice([0.5, 3.0], n), 1.0)
    return np.hstack([o, d * scale[:, None]]).astype(np.float32)


def batch(kind, sc, ref):
    """The scene's rays: paths.batch's 4 096, the last N_GLASS_RAYS of them replaced by the glass family on a scene with GLASS"""
    if kind == "drop":
        return drop_rays(N_DROP_RAYS)
    base = {"glass": "main", "big_glass": "big", "bvh_glass": "bvh", "mesh_glass": "mesh"}.get(kind, kind)
    rays = paths.batch(base, sc, ref.paths)
    if kind in GLASS:
        rays = np.concatenate([rays[:N_RAYS - N_GLASS_RAYS - N_SKY_RAYS], glass_rays(plain_glass_scene(kind), N_GLASS_RAYS), sky_rays(N_SKY_RAYS)])
    assert rays.shape == (N_RAYS, 6)
    return np.ascontiguousarray(rays, np.float32)


class Reference:
    """The reference libraries, built once into out_dir"""

    def __init__(self, out_dir):
        self.paths = paths.Reference(out_dir)               # (primaries, seeds, the mesh reference library)
        self.ora = self.paths.ora
        self.mesh_lib = self.paths.mesh_lib
        src = os.path.join(HERE, "cxx", "ray_streams_reference.c")
        flags = ["gcc", "-O2", "-std=c11", "-fPIC", "-shared", "-ffp-contract=off", "-fno-fast-math", "-fno-math-errno", "-fopenmp", "-Wall", "-Werror"]
        self.libs = {}
        for name, against in (("spheres", self.ora.LIB), ("mesh", os.path.join(str(out_dir), "libmesh_reference.so"))):
            out = os.path.join(str(out_dir), "libray_streams_reference_%s.so" % name)
            res = subprocess.run(flags + [src, "-o", out, against, "-Wl,-rpath," + os.path.dirname(against), "-lm"], capture_output=True, text=True)
            assert res.returncode == 0, res.stdout + res.stderr
            self.libs[name] = C.CDLL(out)
            self.libs[name].ray_streams_reference.restype = None

    def primaries(self, camera, width, height):
        return self.paths.primaries(camera, width, height)

    def seeds(self, n, seed0=SEED0, first_index=0):
        return self.paths.seeds(n, seed0, first_index)

    def trace(self, sc, rays, color, seeds, spp, cap=DEFAULT_CAP, from_result=None, stack_depth=STACK_DEPTH):
        """-> (color, seeds, lost, diag) after spp samples of the walk along every ray; the inputs are left as they are.  from_result: the
        seed rule; None = PTMI_SEED_AUTO (FROM_RESULT without GLASS, KEEP_ACCUMULATOR with it).  lost: (truncated, dropped); diag: a dict of
        (n,) int32 arrays, DIAG's names."""
        spheres, triangles, planes = sc
        s = np.ascontiguousarray(spheres, self.ora.SPHERE_DTYPE)
        p = np.ascontiguousarray(planes, self.ora.PLANE_DTYPE)
        rays = np.ascontiguousarray(rays, np.float32)
        n = len(rays)
        color = np.array(color, np.float32, copy=True).reshape(n, 3)
        seeds = np.array(seeds, copy=True).view(np.uint32).reshape(n, 4)
        glass = bool((s["brdf_tag"] == W.GLASS).any() or (p["brdf_tag"] == W.GLASS).any() or (triangles is not None and (triangles["brdf_tag"] == W.GLASS).any()))
        if from_result is None:
            from_result = not glass
        lost = np.zeros(2, np.int64)
        diag = np.zeros((n, len(DIAG)), np.int32)
        lib = self.libs["spheres"]
        if triangles is not None:
            lib = self.libs["mesh"]
            t = np.ascontiguousarray(triangles, W.TRIANGLE_DTYPE)
            self.mesh_lib.mesh_reference_set(_p(t), len(t))
        lib.ray_streams_reference(int(cap), int(spp), int(bool(from_result)), int(stack_depth), _p(s) if len(s) else None, len(s), _p(p) if len(p) else None,
                                  len(p), _p(rays), n, _p(color), _p(seeds), _p(lost), _p(diag))
        return color, seeds, lost, {name: diag[:, k].copy() for k, name in enumerate(DIAG)}
