"""Scenes and rays for the mesh tests (tests/test_mesh_traversal.py on the CPU, tests/test_gpu_mesh.py on the device): world.mesh_room
with the cases a triangle hierarchy can get wrong added on purpose -- duplicate triangles at other indices (ties), triangles of zero
area, a plane through a triangle with its normal (a triangle / plane tie at equal keys) -- and rays aimed at vertices, at points on
edges (shared edges of the icosphere included), at centroids from the front and from behind, along a triangle's plane, from far away,
and with directions whose length is not 1."""
import ctypes as C
import os
import subprocess

import numpy as np

import __graft_entry__ as graft

pkg = graft.load_package()
world = pkg.world
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def traverse_lib(out_dir):
    """tests/cxx/mesh_traverse.c built with the oracle's flags, linked against oracle/libptoracle.so -> ctypes library"""
    import oracle as ora
    ora.build()
    out = os.path.join(str(out_dir), "libmesh_traverse.so")
    cmd = ["gcc", "-O2", "-std=c11", "-fPIC", "-shared", "-ffp-contract=off", "-fno-fast-math", "-fno-math-errno", "-fopenmp", "-Wall", "-Werror",
           os.path.join(ROOT, "tests", "cxx", "mesh_traverse.c"), "-o", out, ora.LIB, "-Wl,-rpath," + os.path.dirname(ora.LIB), "-lm"]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    lib = C.CDLL(out)
    lib.mesh_walk_check_hit.restype = C.c_int64
    lib.mesh_lin_check_hit.restype = None
    lib.mesh_records.restype = None
    return lib


def reference_lib(out_dir):
    """The oracle's render loops with the mesh checkHit (tests/cxx/mesh_reference.c): pt_oracle.c compiled with the oracle's flags into an
    object whose ora_check_hit is weakened, linked with mesh_reference.c, whose ora_check_hit replaces it -> ctypes library"""
    import oracle as ora
    ora.build()
    flags = ["-O2", "-std=c11", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-fno-math-errno", "-fopenmp"]
    d = str(out_dir)
    obj, ref, out = os.path.join(d, "pt_oracle.o"), os.path.join(d, "mesh_reference.o"), os.path.join(d, "libmesh_reference.so")
    for cmd in (["gcc"] + flags + ["-c", os.path.join(ROOT, "oracle", "pt_oracle.c"), "-o", obj],
                ["objcopy", "--weaken-symbol=ora_check_hit", obj],
                ["gcc"] + flags + ["-Wall", "-Werror", "-c", os.path.join(ROOT, "tests", "cxx", "mesh_reference.c"), "-o", ref],
                ["gcc", "-shared", "-fopenmp", obj, ref, "-o", out, "-lm"]):
        res = subprocess.run(cmd, capture_output=True, text=True)
        assert res.returncode == 0, " ".join(cmd) + "\n" + res.stdout + res.stderr
    # every call of the render loops reaches checkHit through the symbol (nothing inlined): the replacement is what they call
    dis = subprocess.run(["objdump", "-dr", obj], capture_output=True, text=True).stdout
    assert dis.count("ora_check_hit-0x4") + dis.count("R_X86_64_PLT32\tora_check_hit") >= 4, "pt_oracle.o calls checkHit directly"
    lib = C.CDLL(out)
    lib.mesh_reference_set.restype = None
    return lib


class MeshOracle:
    """The oracle module's render functions over a mesh scene: `with MeshOracle(lib, triangles) as ora:` then ora.render_inline(spheres,
    planes, ...) etc. render spheres ++ planes ++ triangles (the oracle module's wrappers, pointed at the mesh reference library)."""

    def __init__(self, lib, triangles):
        self.lib, self.t = lib, np.ascontiguousarray(triangles, world.TRIANGLE_DTYPE)

    def __enter__(self):
        import oracle as ora
        self.ora, self.saved = ora, ora.lib
        self.lib.mesh_reference_set(_p(self.t) if len(self.t) else None, len(self.t))
        base = self.saved()
        for name in ("ora_render_inline_ex", "ora_render_streams_ex", "ora_render_streams_tree", "ora_gen_seeds", "ora_max_threads"):
            fn, want = getattr(self.lib, name), getattr(base, name)
            fn.restype, fn.argtypes = want.restype, want.argtypes
        ora.lib = lambda: self.lib
        return ora

    def __exit__(self, *exc):
        self.ora.lib = self.saved
        return False


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def records(lib, triangles):
    t = np.ascontiguousarray(triangles, world.TRIANGLE_DTYPE)
    out = np.zeros((len(t), 12), np.float32)
    lib.mesh_records(_p(t), len(t), _p(out))
    return out


def adversarial_scene(subdivisions, n_spheres=8, seed=0):
    """mesh_room(subdivisions) plus 1 % duplicated triangles, 5 triangles of zero area, and a plane through the first icosphere triangle
    with its unit normal -> (spheres, triangles, planes)"""
    rng = np.random.default_rng(seed + 500)
    s, t, _ = world.mesh_room(subdivisions, n_spheres, seed)
    dup = t[rng.integers(0, len(t), max(1, len(t) // 100))].copy()
    flat = t[rng.integers(13, len(t), 5)].copy()
    flat["v2"] = flat["v1"]
    t = np.concatenate([t, dup, flat])
    k = 13                                               # the first icosphere triangle (12 room triangles and the light before it)
    v0 = t["v0"][k].astype(np.float32)
    e1, e2 = (t["v1"][k] - t["v0"][k]).astype(np.float32), (t["v2"][k] - t["v0"][k]).astype(np.float32)
    n = np.array([e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]], np.float32)
    nn = np.float32(np.float32(n[0] * n[0] + n[1] * n[1]) + np.float32(n[2] * n[2]))
    nh = (n / np.sqrt(nn)).astype(np.float32)
    planes = np.array([world.plane(tuple(v0), tuple(nh), (0.5, 0.5, 0.5), 0.0, world.MATTE, 1.0)], dtype=world.PLANE_DTYPE)
    return s, t, planes


def _unit(v):
    v = np.asarray(v, np.float64)
    return (v / np.linalg.norm(v, axis=-1, keepdims=True)).astype(np.float32)


def adversarial_rays(triangles, n_rays, seed=0):
    """n_rays rays (n x 6 float32), a mix of the families above"""
    rng = np.random.default_rng(seed)
    t = np.asarray(triangles)
    v0, v1, v2 = (t[k].astype(np.float32) for k in ("v0", "v1", "v2"))
    n = n_rays
    kinds = rng.integers(0, 8, n)
    pick = rng.integers(0, len(t), n)
    origin = np.stack([-10.0 + 22.0 * rng.random(n), -2.5 + 17.0 * rng.random(n), -28.0 + 34.0 * rng.random(n)], 1).astype(np.float32)
    target = origin + rng.normal(size=(n, 3)).astype(np.float32)                   # kind 0: anywhere
    corner = rng.integers(0, 3, n)
    verts = np.stack([v0, v1, v2], 1)
    a, b = verts[pick, corner], verts[pick, (corner + 1) % 3]
    target = np.where((kinds == 1)[:, None], a, target)                            # 1: a vertex
    s = rng.random(n).astype(np.float32)
    edge = (a + s[:, None] * (b - a)).astype(np.float32)
    target = np.where((kinds == 2)[:, None], edge, target)                         # 2: a point on an edge
    cen = ((v0[pick] + v1[pick] + v2[pick]) / np.float32(3.0)).astype(np.float32)
    target = np.where((kinds == 3)[:, None] | (kinds == 4)[:, None], cen, target)  # 3: a centroid; 4: a centroid from far away
    far = cen + _unit(rng.normal(size=(n, 3))) * (10.0 ** rng.uniform(4, 7, n))[:, None].astype(np.float32)
    origin = np.where((kinds == 4)[:, None], far.astype(np.float32), origin)
    # 5: along a triangle's plane, from a point of the triangle; 6: from just behind a triangle (back faces)
    nrm = np.cross(v1[pick] - v0[pick], v2[pick] - v0[pick]).astype(np.float64)
    nrm /= np.maximum(np.linalg.norm(nrm, axis=1, keepdims=True), 1e-30)
    inplane = np.cross(nrm, rng.normal(size=(n, 3)))
    origin = np.where((kinds == 5)[:, None], cen, origin)
    target = np.where((kinds == 5)[:, None], (cen + inplane).astype(np.float32), target)
    origin = np.where((kinds == 6)[:, None], (cen - 0.5 * nrm).astype(np.float32), origin)
    target = np.where((kinds == 6)[:, None], (cen + 0.5 * nrm).astype(np.float32), target)
    d = _unit(target.astype(np.float64) - origin.astype(np.float64))
    d = np.where(np.isfinite(d), d, np.float32(1.0))
    scale = np.where(kinds == 7, rng.choice([1.0 + 1e-6, 1.0 - 3e-5, 1.01, 0.5], n), 1.0)         # 7: |d| != 1
    d = (d * scale[:, None]).astype(np.float32)
    rays = np.concatenate([origin, d], 1).astype(np.float32)
    rays[:3] = [[np.nan, 0, 0, 0, 1, 0], [1, 0, -5, 0, np.inf, 0], [1, 0, -5, 0, 0, 0]]      # non-finite and zero directions
    return np.ascontiguousarray(rays)


def linear_fold(lib, spheres, triangles, planes, rays):
    """the literal fold over spheres ++ planes ++ triangles -> (t, idx, just); a miss is (0, -1, 0)"""
    import oracle as ora
    s = np.ascontiguousarray(spheres, ora.SPHERE_DTYPE)
    p = np.ascontiguousarray(planes, ora.PLANE_DTYPE)
    rec = records(lib, triangles)
    n = len(rays)
    t, idx, just = np.zeros(n, np.float32), np.zeros(n, np.int32), np.zeros(n, np.int32)
    lib.mesh_lin_check_hit(_p(s), len(s), _p(p), len(p), _p(rec), len(rec), _p(rays), n, _p(t), _p(idx), _p(just))
    return t, idx, just


def walk(lib, spheres, triangles, planes, rays):
    """the triangle hierarchy of ptmi_mesh_layout walked as check_hit_mesh walks it -> ((t, idx, just), triangles tested)"""
    import oracle as ora
    s = np.ascontiguousarray(spheres, ora.SPHERE_DTYPE)
    p = np.ascontiguousarray(planes, ora.PLANE_DTYPE)
    tri = np.ascontiguousarray(triangles, world.TRIANGLE_DTYPE)
    nodes, order = pkg.binding.mesh_layout(tri)
    rec = records(lib, tri)
    kept = tri[order] if len(order) else tri[:0]
    allv = np.concatenate([kept["v0"], kept["v1"], kept["v2"]]).astype(np.float32) if len(order) else np.zeros((1, 3), np.float32)
    lo, hi = np.ascontiguousarray(allv.min(0)), np.ascontiguousarray(allv.max(0))
    n = len(rays)
    t, idx, just = np.zeros(n, np.float32), np.zeros(n, np.int32), np.zeros(n, np.int32)
    tests = lib.mesh_walk_check_hit(_p(nodes), _p(order), len(order), _p(lo), _p(hi), _p(s), len(s), _p(p), len(p), _p(rec), len(rec),
                                    _p(rays), n, _p(t), _p(idx), _p(just))
    return (t, idx, just), tests
