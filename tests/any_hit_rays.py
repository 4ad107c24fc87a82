"""Inputs and the CPU restatement for the occlusion tests (tests/test_any_hit_traversal.py on the CPU, tests/any_hit_driver.py on the
device; t_max_for also serves tests/ray_query_driver.py): the families of t_max, the scenes beyond those of ray_query_driver.py, the
loader of tests/cxx/any_hit_traverse.c, and the conditions that keep a case from passing vacuously.  Not a test module."""
import ctypes as C
import os
import subprocess
import types

import numpy as np

import bvh_rays
import mesh_rays
from t_max_families import T_MAX_OF_HITS, T_MAX_OF_MISSES, t_max_for  # noqa: F401

pkg = bvh_rays.pkg
B, W = pkg.binding, pkg.world
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PATHS = ("not served", "early occluder", "to the end", "full search by key", "no limit")      # any_hit_traverse.c: ANY_*
NOT_SERVED, EARLY, TO_THE_END, FULL_BY_KEY, NO_LIMIT = range(5)


def of_fold(fold):
    """t_max_for for a literal fold (t, idx, just), a miss (0, -1, 0)"""
    t, idx, just = fold
    return t_max_for(types.SimpleNamespace(t=np.asarray(t, np.float32), idx=np.where(np.asarray(just) != 0, idx, -1)))


def any_hit_lib(out_dir):
    """tests/cxx/any_hit_traverse.c built with the oracle's flags, linked against oracle/libptoracle.so -> ctypes library"""
    import oracle as ora
    ora.build()
    out = os.path.join(str(out_dir), "libany_hit_traverse.so")
    cmd = ["gcc", "-O2", "-std=c11", "-fPIC", "-shared", "-ffp-contract=off", "-fno-fast-math", "-fno-math-errno", "-fopenmp", "-Wall", "-Werror",
           os.path.join(ROOT, "tests", "cxx", "any_hit_traverse.c"), "-o", out, ora.LIB, "-Wl,-rpath," + os.path.dirname(ora.LIB), "-lm"]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    lib = C.CDLL(out)
    lib.any_linear.restype = None
    lib.any_hierarchy.restype = C.c_int
    lib.any_sphere_reach.restype = C.c_float
    return lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _box(points):
    """(lo, hi) of the rows of points as the scene calls take them: zeros for none"""
    pts = np.asarray(points, np.float32).reshape(-1, 3)
    if len(pts) == 0:
        return np.zeros(3, np.float32), np.zeros(3, np.float32)
    return np.ascontiguousarray(pts.min(0)), np.ascontiguousarray(pts.max(0))


class Case:
    """One scene with its rays: kind "linear", "bvh" or "mesh"; the literal fold, the families of t_max and the specification's answer are
    made once (fold_libs: (bvh_rays.traverse_lib, mesh_rays.traverse_lib))"""

    def __init__(self, name, kind, spheres, planes, rays, fold_libs, triangles=None):
        import oracle as ora
        self.name, self.kind = name, kind
        self.spheres = np.ascontiguousarray(spheres, ora.SPHERE_DTYPE)
        self.planes = np.ascontiguousarray(planes, ora.PLANE_DTYPE)
        self.triangles = None if triangles is None else np.ascontiguousarray(triangles, W.TRIANGLE_DTYPE)
        self.rays = np.ascontiguousarray(rays, np.float32)
        blib, mlib = fold_libs
        if kind == "mesh":
            self.records = mesh_rays.records(mlib, self.triangles)
            self.fold = mesh_rays.linear_fold(mlib, self.spheres, self.triangles, self.planes, self.rays)
        else:
            self.records = np.zeros((0, 12), np.float32)
            self.fold = bvh_rays.linear_fold(blib, self.spheres, self.planes, self.rays)
        self.t_max, self.want, self.family = of_fold(self.fold)
        self.hit = np.asarray(self.fold[2]) != 0

    def trees(self):
        """The hierarchies the host build gives -> (sphere (nodes, order), triangle (nodes, order))"""
        s = B.bvh_layout(self.spheres) if self.kind != "linear" else None
        t = B.mesh_layout(self.triangles) if self.kind == "mesh" else None
        return s, t

    def walk(self, lib, sphere_tree=None, triangle_tree=None, widen=1.0, strict=0):
        """The restatement's (answer, path, primitive tests) per ray, over these trees (default: the host build's)"""
        n = len(self.rays)
        answer, path, tests = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.int32)
        s, p = self.spheres, self.planes
        if self.kind == "linear":
            assert widen == 1.0 and not strict
            lib.any_linear(_p(s), len(s), _p(p), len(p), _p(self.rays), _p(self.t_max), n, _p(answer), _p(path), _p(tests))
            return answer, path, tests
        built = self.trees()
        snodes, sorder = sphere_tree if sphere_tree is not None else built[0]
        slo, shi = _box(s["position"])
        if self.kind == "mesh":
            tnodes, torder = triangle_tree if triangle_tree is not None else built[1]
            kept = self.triangles[torder]
            tlo, thi = _box(np.concatenate([kept["v0"], kept["v1"], kept["v2"]]))
        else:
            tnodes, torder, tlo, thi = snodes, sorder, slo, shi          # (never read)
        torder = np.ascontiguousarray(torder, np.int32)
        sorder = np.ascontiguousarray(sorder, np.int32)
        over = lib.any_hierarchy(_p(np.ascontiguousarray(snodes)), _p(sorder), _p(slo), _p(shi), _p(np.ascontiguousarray(tnodes)), _p(torder), len(torder),
                                 _p(tlo), _p(thi), _p(s), len(s), _p(p), len(p), _p(self.records), len(self.records), int(self.kind == "mesh"),
                                 _p(self.rays), _p(self.t_max), n, C.c_float(widen), int(strict), _p(answer), _p(path), _p(tests))
        assert over == 0, "%s: the traversal stack would overflow for %d rays" % (self.name, over)
        return answer, path, tests

    def wrong(self, answer):
        return np.flatnonzero(np.asarray(answer) != self.want)

    def describe(self, i, got):
        """A failed comparison: the case, ray, family of t_max, closest hit and the answer given"""
        return "%s: ray %d (t_max %s = %r, closest hit t %r, primitive %d): %d" % (
            self.name, i, self.family[i], self.t_max[i], self.fold[0][i], self.fold[1][i], got)


def eta_of(rays):
    d = np.asarray(rays, np.float32)[:, 3:]
    with np.errstate(all="ignore"):
        return np.abs(((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]) - np.float32(1.0))


def beyond_reach(case):
    """A hierarchy scene whose own box refuses every ray: bvh_reach is at least half the box's diagonal wherever the origin lies, and that
    alone is beyond 2^40 (bvh_rays.adversarial_scene's sphere of radius 1e9 at y = -3e9, scaled by 2^12 or 2^20).  Such a case checks the
    admission test and the full search behind it, and nothing of the walk."""
    lo, hi = (np.asarray(x, np.float64) for x in _box(case.spheres["position"]))
    return case.kind != "linear" and np.linalg.norm((hi - lo) / 2) > 2.0 ** 40


def assert_conditions(case, path, brackets=True):
    """What keeps a case from passing vacuously, from the fold and the restatement's path alone"""
    n = len(case.rays)
    if beyond_reach(case):
        assert (path == NOT_SERVED).all(), (case.name, "a ray was served from a box beyond 2^40")
        assert 100 * int(case.want.sum()) >= n and 100 * int((case.hit & (case.want == 0)).sum()) >= n, case.name
        return
    for name in T_MAX_OF_HITS:
        assert (case.family[case.hit] == name).sum() >= 20, (case.name, name, int((case.family[case.hit] == name).sum()))
    for name in T_MAX_OF_MISSES:
        assert (case.family[~case.hit] == name).sum() >= 20, (case.name, name, int((case.family[~case.hit] == name).sum()))
    ones, hit_zeros = int(case.want.sum()), int((case.hit & (case.want == 0)).sum())
    assert 100 * ones >= n and 100 * hit_zeros >= n, (case.name, ones, hit_zeros, n)
    served = path != NOT_SERVED
    assert 100 * int((~served).sum()) >= n and 2 * int(served.sum()) >= n, (case.name, int(served.sum()), n)
    if brackets:
        # the admission brackets: |d|^2 - 1 within 0.2 % of 2^-12 on either side, origins beyond 2^37 on either side of a reach of 2^40
        finite = np.isfinite(case.rays).all(1)
        with np.errstate(all="ignore"):
            eta, far = eta_of(case.rays), np.abs(case.rays[:, :3]).max(1)
        lim = np.float32(2.0 ** -12)
        near_lim = finite & (np.abs(eta / lim - 1) <= 2e-3) & (far < 2.0 ** 37)
        assert (near_lim & served & (eta <= lim)).any() and (near_lim & ~served & (eta > lim)).any(), (case.name, "the |d| bracket")
        long_way = finite & (eta <= lim) & (far >= 2.0 ** 37)
        assert (long_way & served).any() and (long_way & ~served).any(), (case.name, "the reach bracket")
    # among served rays whose answer is 1, some leave early
    assert (served & (case.want == 1) & (path == EARLY)).any(), case.name


def figures(case, path, tests, closest_tests):
    """Measured, not asserted: the shares of the served rays by path, primitive tests per served ray beside the closest walk's"""
    served = path != NOT_SERVED
    k = max(1, int(served.sum()))
    return {"rays": len(path), "served": int(served.sum()), "early": float((path == EARLY).sum()) / k, "to_the_end": float((path == TO_THE_END).sum()) / k,
            "full": float((path == FULL_BY_KEY).sum()) / k, "no_limit": float((path == NO_LIMIT).sum()) / k,
            "tests": int(tests[served].sum()), "closest_tests": int(closest_tests)}


def show(name, fig, wrong_unwidened=None):
    tail = "" if wrong_unwidened is None else ", margin 0 wrong on %d" % wrong_unwidened
    return "%s: %d rays, %d served: early %.3f, to the end %.3f, full search %.4f, no limit %.3f; tests per served ray %.2f, closest walk %.2f%s" % (
        name, fig["rays"], fig["served"], fig["early"], fig["to_the_end"], fig["full"], fig["no_limit"],
        fig["tests"] / max(1, fig["served"]), fig["closest_tests"] / max(1, fig["served"]), tail)


# ---- the rays --------------------------------------------------------------------------------------------------------------------

def with_misses(rays, lo, hi, n_extra, seed=0):
    """rays plus n_extra that start outside the box (lo, hi) and point away from it: misses of a bounded scene, for the scenes (closed
    rooms) whose own rays rarely miss"""
    rng = np.random.default_rng(seed + 3000)
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    c, half = (lo + hi) / 2, np.maximum((hi - lo) / 2, 1e-30)
    u = rng.normal(size=(n_extra, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    o = c + u * (np.linalg.norm(half) * rng.uniform(1.5, 4.0, (n_extra, 1)))
    return np.ascontiguousarray(np.concatenate([rays, np.hstack([o, u]).astype(np.float32)]))


def sphere_rays(spheres, n):
    """test_mesh_exact.bvh_case_rays: adversarial and admission-bracket rays, half each"""
    return np.ascontiguousarray(np.concatenate([bvh_rays.adversarial_rays(spheres, n // 2, seed=8), bvh_rays.admission_rays(spheres, n // 2, seed=8)]))


def admitted(spheres, triangles, rays):
    """Which rays a hierarchy scene serves: occluded_bvh's admission test (triangles None) or occluded_mesh's, operation for operation in
    f32 (mesh_rays.admitted, with the sphere box) -> bool per ray"""
    r = np.asarray(rays, np.float32)
    o = r[:, :3]
    boxes = [_box(np.asarray(spheres)["position"])]
    if triangles is not None:
        tri = np.ascontiguousarray(triangles, W.TRIANGLE_DTYPE)
        kept = tri[B.mesh_layout(tri)[1]]
        boxes.append(_box(np.concatenate([kept["v0"], kept["v1"], kept["v2"]])))
    with np.errstate(all="ignore"):
        P = np.zeros(len(r), np.float32)
        for lo, hi in boxes:
            P2 = np.zeros(len(r), np.float32)
            for a in range(3):
                pa = np.maximum(np.abs(lo[a] - o[:, a]), np.abs(hi[a] - o[:, a]))
                P2 = P2 + pa * pa
            P = np.maximum(P, np.sqrt(P2) * (np.float32(1.0) + np.float32(2.0 ** -20)))
    return np.all(np.isfinite(r), 1) & (eta_of(r) <= np.float32(2.0 ** -12)) & (P <= np.float32(2.0 ** 40))


def plain_rays(lo, hi, n, seed=0):
    """Unit directions from 0.5 .. 4 scene radii away towards points about the scene's middle; the radius is at least 2^-10 of the scene's
    distance from the origin of coordinates, so that a scene a placement has rounded to a few units in the last place still gets rays
    with a direction"""
    rng = np.random.default_rng(seed + 3001)
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    c = (lo + hi) / 2
    R = max(np.linalg.norm(hi - lo) / 2, 2.0 ** -10 * np.abs(c).max(), 1e-30)
    u = rng.normal(size=(n, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    o = (c + u * R * rng.uniform(0.5, 4.0, (n, 1))).astype(np.float32)
    target = c + rng.uniform(-0.5, 0.5, (n, 3)) * (hi - lo)
    d = target - o
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return np.hstack([o, d.astype(np.float32)]).astype(np.float32)


def head_on_rays(records, n, seed=0):
    """Rays at interior points of triangles along the STORED unit normal (mesh_rays.records: v0, v1, v2, n), from the front, from 2^-6 .. 1
    triangle sizes away: where the f32 normal of a needle is noise, a ray aimed by the true normal (mesh_rays.aimed_rays) rarely passes the
    edge functions, which are taken with the stored one"""
    rng = np.random.default_rng(seed + 3002)
    rec = np.asarray(records, np.float64)
    rec = rec[np.isfinite(rec).all(1)]
    pick = rng.integers(0, len(rec), n)
    b = rng.dirichlet((2.0, 2.0, 2.0), n)
    v = rec[pick, :9].reshape(n, 3, 3)
    target = np.einsum("nk,nkj->nj", b, v)
    nh = rec[pick, 9:12]
    size = np.linalg.norm(v[:, 1] - v[:, 0], axis=1)
    o = target + nh * (size * 2.0 ** rng.uniform(-6, 0, n))[:, None]
    rays = np.hstack([o, -nh]).astype(np.float32)
    return np.ascontiguousarray(rays[np.isfinite(rays).all(1)])


def mesh_case_rays(family, scene, n, seed, mlib, hits_wanted=300):
    """sweep_rays of the family (family_rays for None), and more of what a scene's own rays are thin in (never fewer, and the floors of
    assert_conditions stay where they are):
      * rays that miss -- a closed room's rays rarely do;
      * plain_rays where fewer than 55 % are served -- the room scaled by 2^-20 or 2^-12 at an offset of 10^5 and more is a few units in
        the last place across, and most of family_rays' directions there are 0 / 0;
      * head_on_rays that the literal fold calls hits, up to hits_wanted in all -- needles of 1e7 are met by a ray in a thousand"""
    s, t, p = scene
    t = np.asarray(t)
    rays = mesh_rays.sweep_rays(family, t, n, seed=seed) if family else mesh_rays.family_rays(t, n, seed=seed)
    v = np.concatenate([t[k] for k in ("v0", "v1", "v2")]).astype(np.float64)
    rays = with_misses(rays, v.min(0), v.max(0), n // 10, seed)
    if admitted(s, t, rays).sum() < 0.55 * len(rays):
        rays = np.concatenate([rays, plain_rays(v.min(0), v.max(0), len(rays), seed)])
    hits = int(mesh_rays.linear_fold(mlib, s, t, p, rays)[2].sum())
    if hits < hits_wanted:
        more = head_on_rays(mesh_rays.records(mlib, t), 20 * n, seed + 1)
        more = more[mesh_rays.linear_fold(mlib, s, t, p, more)[2] != 0]
        rays = np.concatenate([rays, more[:hits_wanted - hits]])
    return np.ascontiguousarray(rays, np.float32)


# ---- the scenes ------------------------------------------------------------------------------------------------------------------

def reach_scene(n_spheres=1000, seed=4):
    """bvh_rays.multiscale_field cut to what a linear scene takes (1 000 spheres, its 4 planes); its radii reach 2^20, so r^2 comes up
    to 2^40 -> the two scenes on either side of SceneState.sphere_reach's limit: one centre component at 2^40 (1 - 2^-20) and at
    2^40 (1 + 2^-20), both f32 numbers"""
    s, p = bvh_rays.multiscale_field(3000, seed=seed)
    s = s[:n_spheres].copy()
    below, above = s.copy(), s.copy()
    below["position"][5, 1] = np.float32(2.0 ** 40 * (1 - 2.0 ** -20))
    above["position"][5, 1] = np.float32(2.0 ** 40 * (1 + 2.0 ** -20))
    return (below, p), (above, p)


def linear_scenes():
    """(name, spheres, planes, brackets asserted) of the linear cases: mainScene, the bench scene, and the two reach scenes"""
    yield ("mainScene",) + tuple(W.main_scene()) + (True,)
    yield ("bench scene",) + tuple(W.scene16()) + (True,)
    (below, p), (above, _) = reach_scene()
    yield "reach below 2^40", below, p, True
    yield "reach above 2^40", above, p, False                     # nothing is served: sphere_reach refuses the scene


def sphere_scenes():
    import test_mesh_exact
    return test_mesh_exact.bvh_cases()


def moved_spheres(spheres):
    """W.displaced_spheres(..., 0.5, "wave"): what update_spheres is given, and the spheres after it"""
    g = W.displaced_spheres(W.sphere_geometry(spheres), 0.5, "wave", seed=2)
    return np.ascontiguousarray(g, np.float32), W.with_sphere_geometry(spheres, g)


MESH_FAMILIES = mesh_rays.SWEPT + ("needles_1e7",)


def squashed(t, factor=1e-3):
    import test_gpu_mesh_exact
    return test_gpu_mesh_exact.squashed(t, factor)
