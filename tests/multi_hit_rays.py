"""Inputs, the specification and the CPU restatement for the multi-hit tests (tests/test_multi_hit_traversal.py on the CPU,
tests/multi_hit_driver.py on the device): the loader of tests/cxx/multi_hit_reference.c and multi_hit_traverse.c, the STACK a scene is
extended by -- a row of spheres (and, for a mesh scene, of quads) with duplicates, so that rays down the row have more hits than any k and
ties that only the index decides --, its rays, and the families of t_max aimed at the 1st, the k-th and the (k+1)-th hit.  Not a test
module."""
import ctypes as C
import os
import subprocess
import types

import numpy as np

import bvh_rays
import mesh_rays
from t_max_families import t_max_for

pkg = bvh_rays.pkg
B, W = pkg.binding, pkg.world
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STACK_N, STACK_RADIUS, STACK_STEP = 24, 0.4, 1.0
K_MAX = 64                                           # multi_hit_traverse.c's; the reference takes any k


def multi_hit_lib(out_dir):
    """multi_hit_reference.c and multi_hit_traverse.c built with the oracle's flags, linked against the oracle -> ctypes library"""
    import oracle as ora
    ora.build()
    out = os.path.join(str(out_dir), "libmulti_hit.so")
    cmd = ["gcc", "-O2", "-std=c11", "-fPIC", "-shared", "-ffp-contract=off", "-fno-fast-math", "-fno-math-errno", "-fopenmp", "-Wall", "-Werror",
           os.path.join(ROOT, "tests", "cxx", "multi_hit_reference.c"), os.path.join(ROOT, "tests", "cxx", "multi_hit_traverse.c"), "-o", out, ora.LIB,
           "-Wl,-rpath," + os.path.dirname(ora.LIB), "-lm"]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    lib = C.CDLL(out)
    lib.multi_hit_reference.restype = None
    lib.multi_hit_hierarchy.restype = C.c_int
    return lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def _box(points):
    pts = np.asarray(points, np.float32).reshape(-1, 3)
    if len(pts) == 0:
        return np.zeros(3, np.float32), np.zeros(3, np.float32)
    return np.ascontiguousarray(pts.min(0)), np.ascontiguousarray(pts.max(0))


def reference(lib, spheres, planes, records, rays, t_max, k):
    """The specification -> namespace(t (n, k), idx (n, k), count, total = |H|, flags (bit 0 a NaN key, bit 1 a Just at +inf), tie)"""
    import oracle as ora
    s, p = np.ascontiguousarray(spheres, ora.SPHERE_DTYPE), np.ascontiguousarray(planes, ora.PLANE_DTYPE)
    rec = None if records is None or len(records) == 0 else np.ascontiguousarray(records, np.float32)
    rays = np.ascontiguousarray(rays, np.float32)
    tm = None if t_max is None else np.ascontiguousarray(t_max, np.float32)
    n = len(rays)
    t, idx = np.zeros((n, k), np.float32), np.zeros((n, k), np.int32)
    count, total, flags, tie = (np.zeros(n, np.int32) for _ in range(4))
    lib.multi_hit_reference(_p(s), len(s), _p(p), len(p), _p(rec), 0 if rec is None else len(rec), _p(rays), _p(tm), n, k, _p(t), _p(idx), _p(count),
                            _p(total), _p(flags), _p(tie))
    return types.SimpleNamespace(t=t, idx=idx, count=count, total=total, flags=flags, tie=tie)


def walk(lib, spheres, planes, triangles, records, rays, t_max, k, sphere_tree, triangle_tree=None, widen=1.0, strict=0):
    """The restated walk over these trees -> namespace(t, idx, count, served, tests)"""
    import oracle as ora
    s, p = np.ascontiguousarray(spheres, ora.SPHERE_DTYPE), np.ascontiguousarray(planes, ora.PLANE_DTYPE)
    rays = np.ascontiguousarray(rays, np.float32)
    tm = None if t_max is None else np.ascontiguousarray(t_max, np.float32)
    n = len(rays)
    snodes, sorder = sphere_tree
    sorder = np.ascontiguousarray(sorder, np.int32)
    slo, shi = _box(s["position"])
    is_mesh = triangles is not None
    if is_mesh:
        tnodes, torder = triangle_tree
        torder = np.ascontiguousarray(torder, np.int32)
        kept = np.asarray(triangles)[torder]
        tlo, thi = _box(np.concatenate([kept["v0"], kept["v1"], kept["v2"]]))
        rec = np.ascontiguousarray(records, np.float32)
    else:
        tnodes, torder, tlo, thi, rec = snodes, sorder, slo, shi, np.zeros((1, 12), np.float32)
    t, idx = np.zeros((n, k), np.float32), np.zeros((n, k), np.int32)
    count, served, tests = (np.zeros(n, np.int32) for _ in range(3))
    over = lib.multi_hit_hierarchy(_p(np.ascontiguousarray(snodes)), _p(sorder), _p(slo), _p(shi), _p(np.ascontiguousarray(tnodes)), _p(torder),
                                   len(torder) if is_mesh else 0, _p(tlo), _p(thi), _p(s), len(s), _p(p), len(p), _p(rec), len(rec) if is_mesh else 0,
                                   int(is_mesh), _p(rays), _p(tm), n, k, C.c_float(widen), int(strict), _p(t), _p(idx), _p(count), _p(served), _p(tests))
    assert over == 0, "the traversal stack would overflow for %d rays" % over
    return types.SimpleNamespace(t=t, idx=idx, count=count, served=served, tests=tests)


def rows_differ(got, want):
    """The rays whose (t, idx, count) differ: t as numbers (the oracle's min(t0, t1) gives +0 where the device's tca - thc gives -0 for a
    ray that starts on a sphere: tests/test_gpu_bvh.py, same_hits; no listed t is a NaN), idx and count exactly"""
    gt, gi, gc = got
    bad = (np.asarray(gt) != want.t).any(1) | (np.asarray(gi) != want.idx).any(1) | (np.asarray(gc) != want.count)
    return np.flatnonzero(bad)


# ---- the stack -------------------------------------------------------------------------------------------------------------------

def stack_spheres(like, base, axis=0):
    """STACK_N spheres of radius STACK_RADIUS, STACK_STEP apart from `base` along `axis`, then a copy of every eighth (identical geometry
    at a higher index), with the material of like[0]"""
    s = np.concatenate([like[:1]] * STACK_N).copy()
    c = np.tile(np.asarray(base, np.float32), (STACK_N, 1))
    c[:, axis] += np.arange(STACK_N, dtype=np.float32) * np.float32(STACK_STEP)
    s["position"], s["radius"] = c, STACK_RADIUS
    return np.concatenate([s, s[::8].copy()])


def stack_quads(like, base, half=0.6):
    """STACK_N quads (two triangles each) across the x axis, midway between the stack's spheres, facing -x (a ray down the stack meets
    their fronts), then a copy of every eighth triangle pair"""
    t = np.concatenate([like[:1]] * (2 * STACK_N)).copy()
    b = np.asarray(base, np.float32)
    for q in range(STACK_N):
        x = b[0] + np.float32(q * STACK_STEP + 0.5)
        c = [(x, b[1] - half, b[2] - half), (x, b[1] - half, b[2] + half), (x, b[1] + half, b[2] + half), (x, b[1] + half, b[2] - half)]
        t["v0"][2 * q], t["v1"][2 * q], t["v2"][2 * q] = c[0], c[1], c[2]
        t["v0"][2 * q + 1], t["v1"][2 * q + 1], t["v2"][2 * q + 1] = c[0], c[2], c[3]
    pairs = np.concatenate([np.arange(0, 2 * STACK_N, 16), np.arange(1, 2 * STACK_N, 16)])
    return np.concatenate([t, t[np.sort(pairs)].copy()])


def stack_rays(base, n_down, n_oblique, n_away, seed=0):
    """n_down rays down the stack (parallel to +x within a quarter radius of the axis: every sphere and quad is hit), n_oblique that cross
    it at an angle (one to three spheres), n_away that start beside it and point away from it, up and outwards (nothing of the stack)"""
    rng = np.random.default_rng(seed + 7000)
    b = np.asarray(base, np.float64)
    o = b + np.column_stack([-rng.uniform(1.0, 4.0, n_down), rng.uniform(-0.1, 0.1, n_down), rng.uniform(-0.1, 0.1, n_down)])
    down = np.hstack([o, np.tile([1.0, 0.0, 0.0], (n_down, 1))])
    target = b + np.column_stack([rng.uniform(0.0, (STACK_N - 1) * STACK_STEP, n_oblique), rng.uniform(-0.3, 0.3, n_oblique), rng.uniform(-0.3, 0.3, n_oblique)])
    u = rng.normal(size=(n_oblique, 3)) * [1.0, 0.6, 0.6]
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    oblique = np.hstack([target - u * rng.uniform(1.0, 3.0, (n_oblique, 1)), u])
    u = np.column_stack([rng.uniform(-0.3, 0.3, n_away), rng.uniform(0.5, 1.0, n_away), rng.uniform(-0.3, 0.3, n_away)])
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    start = b + np.column_stack([rng.uniform(0.0, (STACK_N - 1) * STACK_STEP, n_away), np.full(n_away, 1.0), rng.uniform(-0.3, 0.3, n_away)])
    away = np.hstack([start, u])
    return np.ascontiguousarray(np.concatenate([down, oblique, away]), np.float32)


# ---- t_max aimed at the 1st, the k-th and the (k+1)-th hit -----------------------------------------------------------------------

def aimed_t_max(ref, k):
    """ref: reference(..., None, k + 1) -- every family of t_max_families (below, equal, above, half, double, zero, -1, inf, nan; one, inf,
    nan where there is no such hit) dealt over the rays, aimed by turns (ray index mod 3) at the 1st, the k-th and the (k+1)-th hit"""
    n = len(ref.count)
    out = np.zeros(n, np.float32)
    turn = np.arange(n) % 3
    for which, col in enumerate((0, k - 1, k)):
        sc = types.SimpleNamespace(t=np.ascontiguousarray(ref.t[:, col]), idx=np.ascontiguousarray(ref.idx[:, col]))
        tm = t_max_for(sc)[0]
        out[turn == which] = tm[turn == which]
    return out


# ---- the device test's scenes (tests/multi_hit_driver.py), made here so that their conditions can be checked without a device -----

N_RAYS = 4096
KINDS = ["plain", "s16", "runs", "bvh", "mesh"]
STACK_BASE = {"plain": (60.0, 40.0, 60.0), "s16": (60.0, 40.0, 60.0), "runs": (60.0, 40.0, 60.0), "bvh": (300.0, 40.0, 300.0), "mesh": (60.0, 80.0, 60.0)}


def driver_scene(kind):
    """tests/ray_query_driver.py's scene of this kind and its 4 096 adversarial rays (the not-served families included), extended by the
    stack: its spheres (and quads) appended, rays 1024 .. 2047 replaced by 512 down the stack, 384 across it and 128 away from it
    -> (spheres, triangles or None, planes, rays)"""
    triangles = None
    if kind == "plain":
        spheres, planes = W.main_scene()
    elif kind == "s16":
        spheres, planes = W.scene16()
    elif kind == "runs":
        from test_gpu_shared_xy import row_scene
        spheres, planes = row_scene(pkg, 9, 2, 4)
    elif kind in ("bvh", "nonfinite linear", "nonfinite bvh"):
        spheres, planes = bvh_rays.adversarial_scene(3000 if kind == "bvh" else 300, seed=0 if kind == "bvh" else 5)
    else:
        spheres, triangles, planes = mesh_rays.adversarial_scene(0)
        assert len(spheres) == 8
    if kind == "mesh":
        rays = np.concatenate([mesh_rays.adversarial_rays(triangles, N_RAYS - 1024, seed=3), bvh_rays.adversarial_rays(spheres, 1024, seed=3)])
    else:
        rays = bvh_rays.adversarial_rays(spheres, N_RAYS, seed=3)
    rays = np.ascontiguousarray(rays, np.float32)
    base = STACK_BASE.get(kind, STACK_BASE["bvh"])
    spheres = np.concatenate([spheres, stack_spheres(spheres, base)])
    if triangles is not None:
        triangles = np.concatenate([triangles, stack_quads(triangles, base)])
    rays[1024:2048] = stack_rays(base, 512, 384, 128, seed=1)
    if kind.startswith("nonfinite"):                 # ray_query_driver.py's: three bad planes in front, and for the linear scene three bad spheres
        bad = np.concatenate([planes[:1]] * 3)
        bad["direction"][0] = (np.nan, 1.0, 0.0)
        bad["position"][1] = (0.0, np.inf, 0.0)
        bad["direction"][2] = (0.0, 0.0, 0.0)
        planes = np.concatenate([bad, planes])
        if kind == "nonfinite linear":
            spheres = spheres.copy()
            spheres["position"][7, 0] = np.nan
            spheres["radius"][11] = np.inf
            spheres["position"][13] = (3e38, -3e38, 3e38)
    rays[-4:] = [[np.nan, 0, 0, 0, 1, 0], [1, 0, -5, 0, np.inf, 0], [np.inf, 1, 2, 0, 0, -1], [1, 0, -5, 0, 0, 0]]
    return spheres, triangles, planes, rays


def served_by(kind, spheres, triangles, rays):
    """Which rays the scene's walk serves: the hierarchies' admission test (any_hit_rays.admitted); a linear scene enumerates for every ray
    and prunes nothing, so all count as served"""
    import any_hit_rays
    if kind in ("bvh", "nonfinite bvh", "mesh"):
        return any_hit_rays.admitted(spheres, triangles, rays)
    return np.ones(len(rays), bool)


def assert_not_vacuous(kind, ref4, served):
    """The cap of the device test, on the specification at k = 4 alone"""
    more, fewer, none, tie = (int((served & m).sum()) for m in (ref4.total > 4, (ref4.total > 0) & (ref4.total < 4), ref4.total == 0, ref4.tie != 0))
    fig = (kind, more, fewer, none, tie, int((~served).sum()))
    assert more >= 64 and fewer >= 64 and none >= 64 and tie >= 64, fig
    if kind in ("bvh", "mesh"):
        assert (~served).sum() >= 32, fig
    return fig
