"""Inputs and the CPU restatement for the nearest-primitive query's tests (tests/test_nearest_exact.py and test_nearest_traversal.py on the
CPU, tests/nearest_driver.py on the device): the loader of tests/cxx/nearest_traverse.cpp, the families of points a scene is asked at, and
the families of r_max aimed at the winner's key.  Not a test module."""
import ctypes as C
import os
import subprocess
import types

import numpy as np

import bvh_rays

pkg = bvh_rays.pkg
B, W = pkg.binding, pkg.world
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MARGIN = 2.0 ** -16                                  # kNearestMargin (csrc/ptmi_nearest.h)


def traverse_lib(out_dir):
    """tests/cxx/nearest_traverse.cpp built with the library's host flags (it includes csrc/ptmi_nearest.h) -> ctypes library"""
    out = os.path.join(str(out_dir), "libnearest_traverse.so")
    host_flags = [f for f in pkg._build.COMPILE_FLAGS if not f.startswith("--offload-arch")]
    cmd = [pkg._build.hipcc_path()] + host_flags + ["-Werror", "-shared", os.path.join(ROOT, "tests", "cxx", "nearest_traverse.cpp"), "-o", out]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    lib = C.CDLL(out)
    lib.nearest_hierarchy.restype = C.c_int
    lib.nearest_records.restype = None
    return lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def _box(points):
    pts = np.asarray(points, np.float32).reshape(-1, 3)
    if len(pts) == 0:
        return np.zeros(3, np.float32), np.zeros(3, np.float32)
    return np.ascontiguousarray(pts.min(0)), np.ascontiguousarray(pts.max(0))


def walk(lib, spheres, planes, triangles, points, r_max, sphere_tree, triangle_tree=None, margin=MARGIN):
    """The restated walk over these trees -> namespace(dist, idx, point, served, tests)"""
    s = np.ascontiguousarray(spheres, B.SPHERE_DTYPE).reshape(-1)
    p = np.ascontiguousarray(planes, B.PLANE_DTYPE).reshape(-1)
    pts = np.ascontiguousarray(points, np.float32)
    rm = None if r_max is None else np.ascontiguousarray(r_max, np.float32)
    n = len(pts)
    snodes, sorder = sphere_tree
    sorder = np.ascontiguousarray(sorder, np.int32)
    slo, shi = _box(s["position"])
    is_mesh = triangles is not None
    if is_mesh:
        t = np.ascontiguousarray(triangles, B.TRIANGLE_DTYPE).reshape(-1)
        tnodes, torder = triangle_tree
        torder = np.ascontiguousarray(torder, np.int32)
        kept = t[torder]
        tlo, thi = _box(np.concatenate([kept["v0"], kept["v1"], kept["v2"]]))
        rec = np.zeros((max(1, len(t)), 12), np.float32)
        lib.nearest_records(_p(t), len(t), _p(rec))
    else:
        t, tnodes, torder, tlo, thi, rec = np.zeros(0), snodes, sorder, slo, shi, np.zeros((1, 12), np.float32)
    dist, idx, at = np.zeros(n, np.float32), np.zeros(n, np.int32), np.zeros((n, 3), np.float32)
    served, tests = np.zeros(n, np.int32), np.zeros(n, np.int32)
    over = lib.nearest_hierarchy(_p(np.ascontiguousarray(snodes)), _p(sorder), _p(slo), _p(shi), _p(np.ascontiguousarray(tnodes)), _p(torder),
                                 len(torder) if is_mesh else 0, _p(tlo), _p(thi), _p(s), len(s), _p(p), len(p), _p(rec), len(t) if is_mesh else 0,
                                 int(is_mesh), _p(pts), _p(rm), n, C.c_float(margin), _p(dist), _p(idx), _p(at), _p(served), _p(tests))
    assert over == 0, "the traversal stack would overflow for %d points" % over
    return types.SimpleNamespace(dist=dist, idx=idx, point=at, served=served, tests=tests)


def same_bits(got, want):
    """The points whose (dist, idx, point) differ in any bit -> their indices"""
    gd, gi, gp = (np.asarray(a) for a in got)
    wd, wi, wp = (np.asarray(a) for a in want)
    bad = (gd.view(np.uint32) != wd.view(np.uint32)) | (gi != wi) | (gp.view(np.uint32) != wp.view(np.uint32)).any(1)
    return np.flatnonzero(bad)


# ---- the points ------------------------------------------------------------------------------------------------------------------

def _unit(rng, n):
    u = rng.normal(size=(n, 3))
    return u / np.linalg.norm(u, axis=1, keepdims=True)


def scene_box(spheres, planes, triangles):
    """Where the scene's primitives lie: the box of the sphere centres and the triangle vertices between their 2nd and 98th percentiles
    per axis (a field's one giant sphere far below it does not stretch it), of the planes' positions for a scene of planes alone"""
    pts = []
    if len(spheres):
        pts.append(spheres["position"].astype(np.float64))
    if triangles is not None and len(triangles):
        pts += [triangles[k].astype(np.float64) for k in ("v0", "v1", "v2")]
    if not pts:
        pts = [planes["position"].astype(np.float64) - 1.0, planes["position"].astype(np.float64) + 1.0]
    a = np.concatenate(pts)
    a = a[np.isfinite(a).all(1)]
    lo, hi = np.percentile(a, 2, axis=0), np.percentile(a, 98, axis=0)
    pad = np.maximum(1e-3 * np.abs(a).max(), 0.0) * (hi <= lo)
    return lo - pad, hi + pad


NON_FINITE = np.array([[np.nan, 0, 0], [0, np.inf, 0], [1, 2, -np.inf], [np.nan, np.nan, np.nan]], np.float32)


def points(spheres, planes, triangles, n, seed=0, far=True):
    """n points (float32 (n, 3)) by turns of seven families: inside the scene's box (enlarged by a quarter); on surfaces (a sphere's, a
    triangle's interior, a plane); at sphere centres; on triangle edges and at vertices; 2^14 .. 2^20 box diagonals away (`far`: where
    a box's own padding no longer covers the rounding); and the last four with non-finite words."""
    rng = np.random.default_rng(seed + 9100)
    lo, hi = scene_box(spheres, planes, triangles)
    diag = max(float(np.linalg.norm(hi - lo)), 1e-30)
    mid = 0.5 * (lo + hi)
    ns, nt, npl = len(spheres), 0 if triangles is None else len(triangles), len(planes)
    out = rng.uniform(lo - 0.25 * (hi - lo), hi + 0.25 * (hi - lo), (n, 3))
    turn = np.arange(n) % 7
    for i in np.flatnonzero(turn == 1):                  # on a surface
        kind = rng.integers(0, 3)
        if kind == 0 and ns:
            j = rng.integers(0, ns)
            out[i] = spheres["position"][j].astype(np.float64) + abs(float(spheres["radius"][j])) * _unit(rng, 1)[0]
        elif kind == 1 and nt:
            j = rng.integers(0, nt)
            w = rng.dirichlet((1, 1, 1))
            out[i] = sum(w[k] * triangles[v][j].astype(np.float64) for k, v in enumerate(("v0", "v1", "v2")))
        elif npl:
            j = rng.integers(0, npl)
            d = planes["direction"][j].astype(np.float64)
            if np.isfinite(d).all() and np.linalg.norm(d) > 0:
                e = out[i] - planes["position"][j].astype(np.float64)
                out[i] = out[i] - d * (e @ d) / (d @ d)
    for i in np.flatnonzero(turn == 2):                  # at a sphere's centre
        if ns:
            out[i] = spheres["position"][rng.integers(0, ns)]
    for i in np.flatnonzero(turn == 3):                  # on a triangle's edge, at a vertex
        if nt:
            j = rng.integers(0, nt)
            a, b = rng.choice(3, 2, replace=False)
            va, vb = (triangles[("v0", "v1", "v2")[k]][j].astype(np.float64) for k in (a, b))
            out[i] = va if rng.integers(0, 3) == 0 else va + (vb - va) * rng.random()
    if far:
        for i in np.flatnonzero(turn == 4):              # far away
            out[i] = mid + _unit(rng, 1)[0] * diag * 2.0 ** rng.uniform(14, 20)
    with np.errstate(over="ignore", invalid="ignore"):
        out = np.ascontiguousarray(out, np.float32)
    out[-len(NON_FINITE):] = NON_FINITE
    return out


def aimed_r_max(dist, idx):
    """r_max by turns (point index mod 8) from the answers without one: just above the winner's key (the same answer), the key itself
    (the winner no longer qualifies), just below it, NaN, 0, -1, twice the key, +inf; a miss gets 1, NaN or +inf"""
    key = np.abs(np.asarray(dist, np.float32))
    n = len(key)
    turn = np.arange(n) % 8
    up, down = np.nextafter(key, np.float32(np.inf)), np.nextafter(key, np.float32(-np.inf))
    out = np.select([turn == 0, turn == 1, turn == 2, turn == 3, turn == 4, turn == 5, turn == 6],
                    [up, key, down, np.float32(np.nan), np.float32(0), np.float32(-1), key * np.float32(2)], np.float32(np.inf)).astype(np.float32)
    miss = np.asarray(idx) < 0
    out[miss] = np.array([1.0, np.nan, np.inf], np.float32)[np.arange(n) % 3][miss]
    return np.ascontiguousarray(out)


# ---- the device test's scenes (tests/nearest_driver.py), made here so that their conditions can be checked without a device -----

N_POINTS = 4096
BEYOND = np.array([[3e12, 0, 0], [0, -2.5e12, 1], [1, 2, 4e12], [-3e12, 3e12, 3e12]], np.float32)      # beyond 2^40 of any of the scenes


def driver_scene(kind):
    """tests/ray_query_driver.py's scene of this kind (its KINDS and its two non-finite scenes, by its constructors) and 4 096 points of
    every family, four of them beyond 2^40 and four with non-finite words -> (spheres, triangles or None, planes, points)"""
    import mesh_rays
    triangles = None
    if kind == "plain":
        spheres, planes = W.main_scene()
    elif kind == "s16":
        spheres, planes = W.scene16()
    elif kind == "runs":
        from test_gpu_shared_xy import row_scene
        spheres, planes = row_scene(pkg, 9, 2, 4)
    elif kind in ("bvh", "nonfinite linear"):
        spheres, planes = bvh_rays.adversarial_scene(3000 if kind == "bvh" else 300, seed=0 if kind == "bvh" else 5)
    else:
        spheres, triangles, planes = mesh_rays.adversarial_scene(0)
        triangles = np.ascontiguousarray(triangles, B.TRIANGLE_DTYPE)
    pts = points(spheres, planes, triangles, N_POINTS, seed=6)
    pts[-8:-4] = BEYOND
    if kind == "nonfinite linear":                   # ray_query_driver.py's: three bad planes in front, three bad spheres
        bad = np.concatenate([planes[:1]] * 3)
        bad["direction"][0] = (np.nan, 1.0, 0.0)
        bad["position"][1] = (0.0, np.inf, 0.0)
        bad["direction"][2] = (0.0, 0.0, 0.0)
        planes = np.concatenate([bad, planes])
        spheres = spheres.copy()
        spheres["position"][7, 0] = np.nan
        spheres["radius"][11] = np.inf
        spheres["position"][13] = (3e38, -3e38, 3e38)
    return spheres, triangles, planes, pts


def served_by(kind, pts):
    """Which points the scene's walk serves, as far as the test needs it: a finite point within 2^39 surely is, one beyond 2^41 or with a
    non-finite word surely is not (the sets hold no point between); a linear scene enumerates for every point"""
    if kind not in ("bvh", "mesh"):
        return np.ones(len(pts), bool)
    with np.errstate(invalid="ignore"):
        big = np.abs(pts).max(1)
    served = np.isfinite(pts).all(1) & (big < 2.0 ** 39)
    assert (served | ~np.isfinite(pts).all(1) | (big > 2.0 ** 41)).all()
    return served
