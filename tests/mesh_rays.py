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


ROOM_BOX = ((-10.0, 22.0), (-2.5, 17.0), (-28.0, 34.0))     # (low, extent) per axis: where world.mesh_room's rays start


def scene_box(triangles, enlarge=0.25):
    """The box of the triangles' vertices, enlarged by `enlarge` of its largest extent on every side, as adversarial_rays' `box`, and
    that largest extent (its `length`) -> (box, length)"""
    t = np.asarray(triangles)
    v = np.concatenate([t[k] for k in ("v0", "v1", "v2")]).astype(np.float64)
    lo, hi = v.min(0), v.max(0)
    length = float((hi - lo).max())
    return tuple((float(lo[a] - enlarge * length), float(hi[a] - lo[a] + 2 * enlarge * length)) for a in range(3)), length


def adversarial_rays(triangles, n_rays, seed=0, box=ROOM_BOX, length=1.0):
    """n_rays rays (n x 6 float32), a mix of the families above.  Origins are drawn from `box` and offsets are in units of `length`
    (scene_box gives both for any scene); the defaults are world.mesh_room's, and with them a seed gives the rays it always gave."""
    rng = np.random.default_rng(seed)
    t = np.asarray(triangles)
    v0, v1, v2 = (t[k].astype(np.float32) for k in ("v0", "v1", "v2"))
    n = n_rays
    kinds = rng.integers(0, 8, n)
    pick = rng.integers(0, len(t), n)
    (x0, xe), (y0, ye), (z0, ze) = box
    origin = np.stack([x0 + xe * rng.random(n), y0 + ye * rng.random(n), z0 + ze * rng.random(n)], 1).astype(np.float32)
    target = origin + rng.normal(size=(n, 3)).astype(np.float32) * np.float32(length)   # kind 0: anywhere
    corner = rng.integers(0, 3, n)
    verts = np.stack([v0, v1, v2], 1)
    a, b = verts[pick, corner], verts[pick, (corner + 1) % 3]
    target = np.where((kinds == 1)[:, None], a, target)                            # 1: a vertex
    s = rng.random(n).astype(np.float32)
    edge = (a + s[:, None] * (b - a)).astype(np.float32)
    target = np.where((kinds == 2)[:, None], edge, target)                         # 2: a point on an edge
    cen = ((v0[pick] + v1[pick] + v2[pick]) / np.float32(3.0)).astype(np.float32)
    target = np.where((kinds == 3)[:, None] | (kinds == 4)[:, None], cen, target)  # 3: a centroid; 4: a centroid from far away
    far = cen + _unit(rng.normal(size=(n, 3))) * ((10.0 ** rng.uniform(4, 7, n)) * length)[:, None].astype(np.float32)
    origin = np.where((kinds == 4)[:, None], far.astype(np.float32), origin)
    # 5: along a triangle's plane, from a point of the triangle; 6: from just behind a triangle (back faces)
    nrm = np.cross(v1[pick] - v0[pick], v2[pick] - v0[pick]).astype(np.float64)
    nrm /= np.maximum(np.linalg.norm(nrm, axis=1, keepdims=True), 1e-30)
    inplane = np.cross(nrm, rng.normal(size=(n, 3)))
    origin = np.where((kinds == 5)[:, None], cen, origin)
    target = np.where((kinds == 5)[:, None], (cen + inplane * length).astype(np.float32), target)
    origin = np.where((kinds == 6)[:, None], (cen - 0.5 * length * nrm).astype(np.float32), origin)
    target = np.where((kinds == 6)[:, None], (cen + 0.5 * length * nrm).astype(np.float32), target)
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


# ---- Beyond the room: placements, shapes and rays for tests/test_mesh_exact.py and tests/test_gpu_mesh_exact.py ----------------------
SCALES = (2.0 ** -20, 2.0 ** -12, 1.0, 3.0, 2.0 ** 12, 2.0 ** 20)
OFFSETS = ((0.0, 0.0, 0.0), (1e3, -2e3, 5e2), (3e5, 1e5, -7e5), (1e7, 1e7, 1e7))
PLACEMENTS = {"room": (1.0, OFFSETS[0]), "moved": (3.0, OFFSETS[1]), "far": (2.0 ** 12, OFFSETS[2])}
MATERIAL = ((0.8, 0.7, 0.5), 0.0, world.MATTE, 1.0)


def transformed(scene, scale, offset):
    """(spheres, triangles, planes) with every position x -> x * scale + offset (in float64, rounded once) and every radius scaled"""
    s, t, p = (np.array(a, copy=True) for a in scene)
    off = np.asarray(offset, np.float64)

    def move(x):
        return (x.astype(np.float64) * scale + off).astype(np.float32)
    for k in ("v0", "v1", "v2"):
        t[k] = move(t[k])
    if len(s):
        s["position"], s["radius"] = move(s["position"]), (s["radius"].astype(np.float64) * scale).astype(np.float32)
    if len(p):
        p["position"] = move(p["position"])
    return s, t, p


def _mesh(v0, v1, v2):
    t = np.zeros(len(v0), dtype=world.TRIANGLE_DTYPE)
    t["v0"], t["v1"], t["v2"] = v0, v1, v2
    t["color"], t["illuminance"], t["brdf_tag"], t["brdf_param"] = MATERIAL
    return t


def _only(t):
    return np.zeros(0, world.SPHERE_DTYPE), t, np.zeros(0, world.PLANE_DTYPE)


def _frames(rng, n):
    u = _unit(rng.normal(size=(n, 3))).astype(np.float64)
    v = np.cross(u, rng.normal(size=(n, 3)))
    return u, v / np.linalg.norm(v, axis=1, keepdims=True)


def needles(n=3000, seed=0, aspects=(1e3, 1e5)):
    """Needles in general position: two sides of length L in 2 .. 6, the third L / aspect, the aspect ratios in turn (e1 x e2 cancels:
    its terms are L^2, their difference L^2 / aspect).  At 1e7 (needles_1e7) the f32 normal is noise: exact_mesh calls such a triangle
    unconstrained, and one of them in a scene is a possible hit of every ray, so they have a scene of their own."""
    rng = np.random.default_rng(seed + 700)
    u, v = _frames(rng, n)
    c = rng.uniform(-10, 10, (n, 3))
    L = rng.uniform(2, 6, n)[:, None]
    w = L / np.asarray(aspects)[np.arange(n) % len(aspects)][:, None]
    return _only(_mesh(c, c + L * u, c + L * u + w * v))


def needles_1e7(n=3000, seed=0):
    return needles(n, seed, aspects=(1e7,))


def slivers(n=3000, seed=0):
    """One angle near 180 degrees: the apex over the middle of a side of length L at a height of L * 10^-2.5 .. 10^-5"""
    rng = np.random.default_rng(seed + 701)
    u, v = _frames(rng, n)
    c = rng.uniform(-10, 10, (n, 3))
    L = rng.uniform(2, 6, n)[:, None]
    h = L * (10.0 ** rng.uniform(-5, -2.5, n))[:, None]
    return _only(_mesh(c, c + L * u, c + (0.3 + 0.4 * rng.random((n, 1))) * L * u + h * v))


def _grid(m, y, flip=False):
    x, z = np.meshgrid(-9.0 + 0.47 * np.arange(m + 1), -25.0 + 0.53 * np.arange(m + 1), indexing="ij")
    P = np.stack([x, np.full_like(x, y), z], -1)
    a, b, c, d = P[:-1, :-1].reshape(-1, 3), P[1:, :-1].reshape(-1, 3), P[1:, 1:].reshape(-1, 3), P[:-1, 1:].reshape(-1, 3)
    v0, v1, v2 = np.concatenate([a, a]), np.concatenate([c, d]), np.concatenate([b, c])       # normal +y
    return _mesh(v0, v2, v1) if flip else _mesh(v0, v1, v2)


def planar_grid(m=40, seed=0):
    """An axis-aligned grid in the plane y = 1.7 (2 m^2 triangles, normal +y): every box has no thickness in y, adjacent triangles are
    coplanar, every shared edge a tie candidate"""
    return _only(_grid(m, 1.7))


def coincident_grids(m=28, seed=0):
    """Two coincident grids of opposite winding: one faces +y, the other -y, at the same place"""
    return _only(np.concatenate([_grid(m, 1.7), _grid(m, 1.7, flip=True)]))


def multiscale(n=3000, seed=0):
    """Triangle sizes 2^-20 .. 2^20 in one scene, each at a distance of its size times 2^0 .. 2^10 from the origin: tiny triangles far
    (in their own measure) from the origin, next to huge ones whose pads cover them"""
    rng = np.random.default_rng(seed + 702)
    size = (2.0 ** rng.uniform(-20, 20, n))[:, None]
    c = _unit(rng.normal(size=(n, 3))) * size * (2.0 ** rng.uniform(0, 10, (n, 1)))
    u, v = _frames(rng, n)
    return _only(_mesh(c, c + size * u, c + size * (0.5 * u + v)))


def closed_icosphere(subdivisions=4, seed=0):
    """world.mesh_room's icosphere alone (radius 3 about (1, 3, -16), faces outward): closed, seen from inside and from outside"""
    v, f = world.icosphere(subdivisions)
    return _only(world.triangles_of(v * 3.0 + np.array([1.0, 3.0, -16.0]), f, MATERIAL))


def closed_room(subdivisions=3, seed=0):
    """adversarial_scene's triangles alone (the room, the icosphere, duplicates, zero areas)"""
    return _only(adversarial_scene(subdivisions, seed=seed)[1])


def mixed_room(subdivisions=3, seed=0):
    """adversarial_scene with its spheres, its plane through a triangle and a floor plane below the room (a primitive beyond the mesh)"""
    s, t, p = adversarial_scene(subdivisions, seed=seed)
    below = np.array([world.plane((0.0, -6.0, 0.0), (0.0, 1.0, 0.0), (0.5, 0.5, 0.5), 0.0, world.MATTE, 1.0)], dtype=world.PLANE_DTYPE)
    return s, t, np.concatenate([p, below])


FAMILIES = {"room": closed_room, "needles": needles, "slivers": slivers, "planar_grid": planar_grid, "coincident_grids": coincident_grids,
            "multiscale": multiscale, "icosphere": closed_icosphere, "needles_1e7": needles_1e7, "mixed": None}
SWEPT = ("room", "needles", "slivers", "planar_grid", "coincident_grids", "multiscale", "icosphere", "mixed")      # the sweeps with shares
# multiscale: sizes up to 2^20 scaled by 2^12 overflow nn (the scene is refused, rightly), 2^-20 by 2^-12 underflow it,
# and an offset would round its small triangles away: its placements are scales alone
FAMILY_PLACEMENTS = {"multiscale": {"room": PLACEMENTS["room"], "moved": (3.0, OFFSETS[0]), "far": (2.0 ** -3, OFFSETS[0])},
                     # needles: at x3 + (1e3, -2e3, 5e2) a short side of 1e-4 is one unit in the last place of its coordinates, and the
                     # needle is no longer one; the offset that keeps 60 units
                     "needles": {"room": PLACEMENTS["room"], "moved": (3.0, (10.0, -20.0, 5.0)), "far": PLACEMENTS["far"]}}


def placed(family, placement, seed=0):
    """The family's scene at a placement of PLACEMENTS -> (spheres, triangles, planes)"""
    scale, offset = FAMILY_PLACEMENTS.get(family, PLACEMENTS)[placement]
    scene = FAMILIES[family](seed=seed) if family != "mixed" else mixed_room(seed=seed)
    return scene if (scale, tuple(offset)) == (1.0, OFFSETS[0]) else transformed(scene, scale, offset)


def placed_point(family, placement, point, radius):
    scale, offset = FAMILY_PLACEMENTS.get(family, PLACEMENTS)[placement]
    return np.asarray(point, np.float64) * scale + np.asarray(offset, np.float64), radius * scale


def sweep_rays(family, triangles, n_rays, seed=0):
    return family_rays(triangles, n_rays, seed, aimed=AIMED_SHARE.get(family, 0.0))


# where a closed mesh is seen from inside: (centre, radius) of the origins at the room placement
INSIDE = {"icosphere": ((1.0, 3.0, -16.0), 2.5), "room": ((1.0, 10.0, -5.0), 2.0)}


def _next(x, steps):
    """f32 x moved by `steps` units in the last place (x > 0)"""
    return (np.asarray(x, np.float32).view(np.int32) + np.asarray(steps, np.int32)).view(np.float32)


def special_rays(triangles, n_rays, seed=0):
    """Rays at the walk's own limits, a fifth each: (a) axis-parallel directions whose other components are exact zeros or 1e-30 .. 1e-42
    (the 2^-80 clamp on 1 / d); (b) |d|^2 - 1 just below, at and just above +-2^-12 (the admission test); (c) origins that put
    bvh_reach on both sides of 2^40 (hierarchy and literal fold); (d) origins on a triangle's plane and on a face of a box of the
    hierarchy; (e) grazing: d . n within a few units in the last place of 1e-6 (exactly so where n is an axis)"""
    rng = np.random.default_rng(seed + 900)
    t = np.asarray(triangles)
    v = np.stack([t[k].astype(np.float64) for k in ("v0", "v1", "v2")], 1)
    _, length = scene_box(t)
    n = n_rays
    fam = np.arange(n) % 5
    pick = rng.integers(0, len(t), n)
    b = rng.dirichlet((1.0, 1.0, 1.0), n)
    b[rng.random(n) < 0.3] = (0.5, 0.5, 0.0)                                           # some on an edge
    inside = np.einsum("nk,nkj->nj", b, v[pick])
    nrm = np.cross(v[pick, 1] - v[pick, 0], v[pick, 2] - v[pick, 0])
    nrm /= np.maximum(np.linalg.norm(nrm, axis=1, keepdims=True), 1e-300)
    rnd = _unit(rng.normal(size=(n, 3))).astype(np.float64)
    rnd = np.where((np.sum(rnd * nrm, 1) > 0)[:, None] & (rng.random(n) < 0.85)[:, None], -rnd, rnd)      # mostly onto the front face
    dist = length * 10.0 ** rng.uniform(-2, 0.5, n)
    d = rnd.copy()
    o = inside - d * dist[:, None]
    # (a)
    a = fam == 0
    axis = rng.integers(0, 3, n)
    sign = np.where(nrm[np.arange(n), axis] > 0, -1.0, 1.0)
    da = np.zeros((n, 3))
    tiny = rng.choice([0.0, 1e-30, -1e-30, 1e-36, 1e-38, -1e-40, 1e-42, -1e-42], (n, 3))
    da[:] = tiny
    da[np.arange(n), axis] = sign
    d[a] = da[a]
    o[a] = inside[a] - da[a] * dist[a, None]
    # (b)
    k = fam == 1
    eta = 2.0 ** -12 * rng.choice([1 - 1e-3, 1 - 1e-6, 1.0, 1 + 1e-6, 1 + 1e-3], n) * rng.choice([-1.0, 1.0], n)
    d[k] = rnd[k] * np.sqrt(1.0 + eta[k])[:, None]
    # (c)
    k = fam == 2
    R = 2.0 ** 40 * rng.choice([0.25, 0.98, 1.02, 4.0], n)
    o[k] = inside[k] - rnd[k] * R[k, None]
    # (d)
    k = fam == 3
    nodes, _ = pkg.binding.mesh_layout(np.ascontiguousarray(t, world.TRIANGLE_DTYPE))
    nd = nodes[rng.integers(0, len(nodes), n)]
    ch = rng.integers(0, 2, n)
    bc, bh = nd["center"][np.arange(n), ch].astype(np.float64), np.abs(nd["half"][np.arange(n), ch].astype(np.float64))
    face = bc + (rng.random((n, 3)) * 2 - 1) * bh
    ax = rng.integers(0, 3, n)
    face[np.arange(n), ax] = (bc + rng.choice([-1.0, 1.0], n)[:, None] * bh)[np.arange(n), ax]
    on_box = (rng.random(n) < 0.4) & np.all(np.isfinite(face), 1)
    o[k] = np.where(on_box[k, None], face[k], inside[k])
    d[k] = _unit(rng.normal(size=(int(k.sum()), 3)))
    # (e)
    k = fam == 4
    tang = np.cross(nrm, rng.normal(size=(n, 3)))
    tang /= np.maximum(np.linalg.norm(tang, axis=1, keepdims=True), 1e-300)
    c = _next(np.full(n, 1e-6, np.float32), rng.integers(-4, 5, n)).astype(np.float64) * rng.choice([1.0, 1.0, -1.0], n)
    d[k] = (tang + nrm * c[:, None])[k]
    o[k] = inside[k] - d[k] * dist[k, None]
    rays = np.concatenate([o, d], 1).astype(np.float32)
    flat = k & (np.abs(nrm).max(1) == 1.0)                                             # an axis normal: d . n is that component, exactly
    axn = np.abs(nrm).argmax(1)
    rays[flat, 3 + axn[flat]] = (c * nrm[np.arange(n), axn])[flat].astype(np.float32)
    return np.ascontiguousarray(rays[np.all(np.isfinite(rays), 1)])


def aimed_rays(triangles, n_rays, seed=0):
    """Rays at interior points of triangles picked by area, from the front and within 45 degrees of the normal, from 0.01 .. 1 scene lengths away"""
    rng = np.random.default_rng(seed + 902)
    t = np.asarray(triangles)
    if n_rays == 0:
        return np.zeros((0, 6), np.float32)
    v = np.stack([t[k].astype(np.float64) for k in ("v0", "v1", "v2")], 1)
    nrm = np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0])
    area = np.linalg.norm(nrm, axis=1)
    pick = rng.choice(len(t), n_rays, p=area / area.sum())
    b = rng.dirichlet((2.0, 2.0, 2.0), n_rays)
    target = np.einsum("nk,nkj->nj", b, v[pick])
    nh = nrm[pick] / area[pick][:, None]
    d = _unit(0.7 * _unit(rng.normal(size=(n_rays, 3))).astype(np.float64) - nh).astype(np.float64)       # within 45 degrees of head-on
    _, length = scene_box(t)
    o = target - d * (length * 10.0 ** rng.uniform(-2, 0, n_rays))[:, None]
    return np.concatenate([o, d], 1).astype(np.float32)


AIMED_SHARE = {"needles": 0.5, "slivers": 0.6, "planar_grid": 0.4, "coincident_grids": 0.3}


def admitted(triangles, rays):
    """Which rays the walk serves from the hierarchy (the others take the literal fold): check_hit_mesh's admission test for a scene
    without spheres, operation for operation in f32 -> bool per ray"""
    tri = np.ascontiguousarray(triangles, world.TRIANGLE_DTYPE)
    _, order = pkg.binding.mesh_layout(tri)
    kept = tri[order]
    allv = np.concatenate([kept["v0"], kept["v1"], kept["v2"]]).astype(np.float32)
    lo, hi = allv.min(0), allv.max(0)
    r = np.asarray(rays, np.float32)
    o, d = r[:, :3], r[:, 3:]
    with np.errstate(all="ignore"):
        eta = np.abs(((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]) - np.float32(1.0))
        P2 = np.zeros(len(r), np.float32)
        for a in range(3):
            pa = np.maximum(np.abs(lo[a] - o[:, a]), np.abs(hi[a] - o[:, a]))
            P2 = P2 + pa * pa
        P = np.sqrt(P2) * (np.float32(1.0) + np.float32(2.0 ** -20))
    return np.all(np.isfinite(r), 1) & (eta <= np.float32(2.0 ** -12)) & (P <= np.float32(2.0 ** 40))


def family_rays(triangles, n_rays, seed=0, aimed=0.0):
    """adversarial_rays drawn from the scene's own box, a quarter special_rays, and a share `aimed` of aimed_rays (thin shapes are
    rarely met by chance: AIMED_SHARE[family]); finite rays with a direction only"""
    box, length = scene_box(triangles)
    n_aimed = int(n_rays * aimed)
    a = adversarial_rays(triangles, n_rays - n_rays // 4 - n_aimed, seed, box=box, length=length)[3:]
    rays = np.concatenate([a, special_rays(triangles, n_rays // 4, seed), aimed_rays(triangles, n_aimed, seed)])
    return np.ascontiguousarray(rays[np.all(np.isfinite(rays), 1) & np.any(rays[:, 3:] != 0, 1)])


def inside_edge_rays(triangles, centre, radius, n_rays, seed=0):
    """Rays from within `radius` of `centre` (inside a closed mesh) aimed at vertices and at points on edges: what a crack lets through"""
    rng = np.random.default_rng(seed + 901)
    t = np.asarray(triangles)
    v = np.stack([t[k].astype(np.float32) for k in ("v0", "v1", "v2")], 1)
    pick, corner = rng.integers(0, len(t), n_rays), rng.integers(0, 3, n_rays)
    a, b = v[pick, corner], v[pick, (corner + 1) % 3]
    s = np.where(rng.random(n_rays) < 0.3, 0.0, rng.random(n_rays)).astype(np.float32)
    target = (a + s[:, None] * (b - a)).astype(np.float32)
    o = (np.asarray(centre, np.float64) + _unit(rng.normal(size=(n_rays, 3))) * (radius * rng.random((n_rays, 1)) ** (1 / 3))).astype(np.float32)
    return np.ascontiguousarray(np.concatenate([o, _unit(target.astype(np.float64) - o)], 1).astype(np.float32))
