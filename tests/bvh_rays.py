"""Scenes and rays for the BVH tests (tests/test_bvh_traversal.py on the CPU, tests/test_gpu_bvh.py on the device): a random sphere
field with the cases a hierarchy can get wrong added on purpose -- duplicate spheres at other indices (ties), zero and huge radii --
and rays aimed at what pads and prunes: sphere silhouettes (tangent and grazing by a relative 1e-7 .. 1e-3), box faces, edges and
corners, origins on sphere surfaces (as bounce rays start) and inside boxes, axis-parallel directions, directions whose length is
not 1 (inside and beyond what the hierarchy serves), far and non-finite origins."""
import numpy as np

import __graft_entry__ as graft

pkg = graft.load_package()
world = pkg.world


def adversarial_scene(n_spheres, seed=0):
    """sphere_field(n_spheres) plus 1 % duplicates of earlier spheres appended, 10 zero radii, a radius 1e3 and a radius 1e9."""
    rng = np.random.default_rng(seed + 1000)
    s, p = world.sphere_field(n_spheres, seed)
    dup = s[rng.integers(0, len(s), max(1, len(s) // 100))].copy()
    zero = s[rng.integers(0, len(s), 10)].copy()
    zero["radius"] = 0.0
    zero["position"][:, 0] += 0.25
    huge = s[[0, 0]].copy()
    huge["position"] = [(1.0, 2000.0, -6.0), (1.0, -3e9, -6.0)]
    huge["radius"] = [1e3, 1e9]
    return np.concatenate([s, dup, zero, huge]), p


def _unit(v):
    v = np.asarray(v, np.float64)
    return (v / np.linalg.norm(v, axis=-1, keepdims=True)).astype(np.float32)


def adversarial_rays(spheres, n_rays, seed=0):
    """n_rays rays (n x 6 float32), a mix of the families above."""
    rng = np.random.default_rng(seed)
    s = np.asarray(spheres)
    nodes, _ = pkg.binding.bvh_layout(s)
    c = s["position"].astype(np.float64)
    r = np.abs(s["radius"].astype(np.float64))
    field = r < 100.0
    lo, hi = c[field].min(0) - 1.0, c[field].max(0) + 1.0
    k = n_rays // 8
    out = []

    def rand_dir(m):
        return _unit(rng.normal(size=(m, 3)))

    # 1. random origins in the field, random directions
    o = lo + (hi - lo) * rng.random((k, 3))
    out.append(np.hstack([o, rand_dir(k)]))
    # 2. tangent and grazing at sphere silhouettes
    i = rng.integers(0, len(s), k)
    u = rand_dir(k).astype(np.float64)
    v = np.cross(u, rng.normal(size=(k, 3)))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    rel = rng.choice([0.0, 1e-7, -1e-7, 1e-6, -1e-6, 1e-5, -1e-5, 1e-4, -1e-4, 1e-3, -1e-3], k)
    x = c[i] + v * (r[i] * (1.0 + rel))[:, None]
    dist = rng.choice([0.01, 0.5, 3.0, 30.0, 300.0], k) * (1.0 + rng.random(k))
    out.append(np.hstack([x - u * dist[:, None], u]))
    # 3. grazing box faces, edges and corners of the hierarchy's child boxes
    nd = nodes[rng.integers(0, len(nodes), k)]
    ch = rng.integers(0, 2, k)
    bc = nd["center"][np.arange(k), ch].astype(np.float64)
    bh = np.abs(nd["half"][np.arange(k), ch].astype(np.float64))
    sign = rng.choice([-1.0, 1.0], (k, 3))
    which = rng.random((k, 3)) < 0.7                         # which coordinates sit on the boundary (a face, an edge or a corner)
    target = bc + np.where(which, sign * bh, (rng.random((k, 3)) * 2 - 1) * bh)
    u = rand_dir(k).astype(np.float64)
    out.append(np.hstack([target - u * rng.choice([0.1, 2.0, 50.0], k)[:, None], u]))
    # 4. origins on sphere surfaces, directions away from the surface (bounce rays) and into it
    i = rng.integers(0, len(s), k)
    nrm = rand_dir(k).astype(np.float64)
    o = (c[i] + nrm * r[i][:, None]).astype(np.float32)
    dv = rand_dir(k).astype(np.float64)
    dv = np.where((np.sum(dv * nrm, 1) < 0)[:, None] & (rng.random(k) < 0.8)[:, None], -dv, dv)
    out.append(np.hstack([o, dv]))
    # 5. origins inside boxes
    nd = nodes[rng.integers(0, len(nodes), k)]
    ch = rng.integers(0, 2, k)
    bc = nd["center"][np.arange(k), ch].astype(np.float64)
    bh = np.abs(nd["half"][np.arange(k), ch].astype(np.float64))
    out.append(np.hstack([bc + (rng.random((k, 3)) * 2 - 1) * bh, rand_dir(k)]))
    # 6. axis-parallel directions (one or two zero components), origins on sphere centres' planes and box planes
    m = k
    axes = rng.integers(0, 3, m)
    dv = np.zeros((m, 3))
    dv[np.arange(m), axes] = rng.choice([-1.0, 1.0], m)
    two = rng.random(m) < 0.4
    other = (axes + 1) % 3
    dv[two, axes[two]] *= 0.6
    dv[two, other[two]] = rng.choice([-0.8, 0.8], int(two.sum()))
    o = lo + (hi - lo) * rng.random((m, 3))
    i = rng.integers(0, len(s), m)
    snap = rng.random(m) < 0.5
    ax2 = (axes + 2) % 3
    o[snap, ax2[snap]] = c[i[snap], ax2[snap]] + rng.choice([0.0, 1.0, -1.0], int(snap.sum())) * r[i[snap]]
    out.append(np.hstack([o, dv]))
    # 7. directions whose length is not 1: within the renderer's few 1e-6, near the 2^-12 limit, beyond it
    o = lo + (hi - lo) * rng.random((k, 3))
    scale = rng.choice([1 + 3e-6, 1 - 3e-6, 1 + 1e-4, 1 - 1e-4, 1 + 2e-4, 1 - 2e-4, 1.01, 0.5, 3.0], k)
    out.append(np.hstack([o, rand_dir(k) * scale[:, None]]))
    # 8. the rest: silhouettes from far away, far and non-finite origins, zero-radius centres
    rest = n_rays - 7 * k
    i = rng.integers(0, len(s), rest)
    u = rand_dir(rest).astype(np.float64)
    v = np.cross(u, rng.normal(size=(rest, 3)))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    x = c[i] + v * r[i][:, None]
    o = x - u * rng.choice([1e3, 1e5, 1e13], rest)[:, None]
    bad = rng.random(rest) < 0.01
    o[bad, 0] = np.nan
    out.append(np.hstack([o, u]))
    return np.ascontiguousarray(np.vstack(out).astype(np.float32))


def traverse_lib(out_dir):
    """tests/cxx/bvh_traverse.c built with the oracle's flags, linked against oracle/libptoracle.so -> ctypes library"""
    import ctypes as C
    import os
    import subprocess
    import oracle as ora
    ora.build()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = os.path.join(str(out_dir), "libbvh_traverse.so")
    cmd = ["gcc", "-O2", "-std=c11", "-fPIC", "-shared", "-ffp-contract=off", "-fno-fast-math", "-fno-math-errno", "-fopenmp", "-Wall", "-Werror",
           os.path.join(root, "tests", "cxx", "bvh_traverse.c"), "-o", out, ora.LIB, "-Wl,-rpath," + os.path.dirname(ora.LIB), "-lm"]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    lib = C.CDLL(out)
    lib.bvh_check_hit.restype = C.c_int64
    lib.lin_check_hit.restype = None
    return lib


def linear_fold(lib, spheres, planes, rays):
    """ora_check_hit's fold with the index kept (tests/cxx/bvh_traverse.c) -> (t, idx, just); a miss is (0, -1, 0)"""
    import ctypes as C
    import oracle as ora
    s = np.ascontiguousarray(spheres, ora.SPHERE_DTYPE)
    p = np.ascontiguousarray(planes, ora.PLANE_DTYPE)
    n = len(rays)
    t, idx, just = np.zeros(n, np.float32), np.zeros(n, np.int32), np.zeros(n, np.int32)
    P = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    lib.lin_check_hit(P(s), len(s), P(p), len(p), P(np.ascontiguousarray(rays, np.float32)), n, P(t), P(idx), P(just))
    return t, idx, just


# ---- Beyond the field: placements, radii of every size and the admission test's brackets (tests/test_mesh_exact.py, test_gpu_mesh_exact.py) ----
SCALES = (2.0 ** -20, 2.0 ** -12, 1.0, 3.0, 2.0 ** 12, 2.0 ** 20)
OFFSETS = ((0.0, 0.0, 0.0), (1e3, -2e3, 5e2), (3e5, 1e5, -7e5), (1e7, 1e7, 1e7))


def transformed(scene, scale, offset):
    """(spheres, planes) with every position x -> x * scale + offset (in float64, rounded once) and every radius scaled"""
    s, p = (np.array(a, copy=True) for a in scene)
    off = np.asarray(offset, np.float64)
    s["position"] = (s["position"].astype(np.float64) * scale + off).astype(np.float32)
    s["radius"] = (s["radius"].astype(np.float64) * scale).astype(np.float32)
    if len(p):
        p["position"] = (p["position"].astype(np.float64) * scale + off).astype(np.float32)
    return s, p


def multiscale_field(n_spheres=3000, seed=0):
    """Radii 2^-20 .. 2^20 in one field, each centre 2 .. 2^7 radii from the origin; sphere_field's materials and planes"""
    rng = np.random.default_rng(seed + 2000)
    s, p = world.sphere_field(n_spheres, seed)
    r = 2.0 ** rng.uniform(-20, 20, len(s))
    s["radius"] = r
    s["position"] = _unit(rng.normal(size=(len(s), 3))) * (r * 2.0 ** rng.uniform(1, 7, len(s)))[:, None]
    return s, p


def admission_rays(spheres, n_rays, seed=0):
    """Rays at sphere centres and silhouettes that bracket what the hierarchy serves: |d|^2 - 1 just below, at and just above +-2^-12, and
    origins that put the reach on both sides of 2^40; a third each, the last third from 0.1 .. 100 radii away with |d| = 1"""
    rng = np.random.default_rng(seed + 2001)
    s = np.asarray(spheres)
    c, r = s["position"].astype(np.float64), np.abs(s["radius"].astype(np.float64))
    i = rng.integers(0, len(s), n_rays)
    u = _unit(rng.normal(size=(n_rays, 3))).astype(np.float64)
    v = np.cross(u, rng.normal(size=(n_rays, 3)))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    x = c[i] + v * (r[i] * rng.choice([0.0, 0.5, 1.0, 1.0 + 1e-6, 1.0 - 1e-6], n_rays))[:, None]
    fam = np.arange(n_rays) % 3
    dist = np.maximum(r[i], 1e-3) * 10.0 ** rng.uniform(-1, 2, n_rays)
    dist = np.where(fam == 1, 2.0 ** 40 * rng.choice([0.25, 0.98, 1.02, 4.0], n_rays), dist)
    eta = 2.0 ** -12 * rng.choice([1 - 1e-3, 1 - 1e-6, 1.0, 1 + 1e-6, 1 + 1e-3], n_rays) * rng.choice([-1.0, 1.0], n_rays)
    d = u * np.where(fam == 0, np.sqrt(1.0 + eta), 1.0)[:, None]
    return np.ascontiguousarray(np.hstack([x - u * dist[:, None], d]).astype(np.float32))
