"""The ray sets the ray order is tried with, shared by tests/test_ray_order_layout.py (against the written formula, no GPU) and
tests/ray_order_driver.py (the device against the host twin).  Not a test module; it needs numpy and the package alone."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

N_RAYS = 4096
NOT_PLACED = [[np.nan, 0, 0, 0, 1, 0], [1, 0, -5, 0, np.inf, 0], [np.inf, 1, 2, 0, 0, -1], [1, 0, -5, 0, 0, 0]]     # as tests/ray_query_driver.py ends every set


def adversarial_sets(pkg):
    """{kind: (4 096, 6) rays}: the five sets of tests/ray_query_driver.py (its Scene makes the same rays from the same seeds), each ending
    in three non-finite rays and one zero-direction ray"""
    import bvh_rays
    import mesh_rays
    from test_gpu_shared_xy import row_scene
    W = pkg.world
    sets = {}
    for kind, spheres in (("plain", W.main_scene()[0]), ("s16", W.scene16()[0]), ("runs", row_scene(pkg, 9, 2, 4)[0]),
                          ("bvh", bvh_rays.adversarial_scene(3000)[0])):
        sets[kind] = bvh_rays.adversarial_rays(spheres, N_RAYS, seed=3)
    spheres, triangles, _ = mesh_rays.adversarial_scene(0)
    sets["mesh"] = np.concatenate([mesh_rays.adversarial_rays(triangles, N_RAYS - 1024, seed=3), bvh_rays.adversarial_rays(spheres, 1024, seed=3)])
    for kind in sets:
        sets[kind] = np.ascontiguousarray(sets[kind], np.float32)
        sets[kind][-4:] = NOT_PLACED
        assert sets[kind].shape == (N_RAYS, 6)
    return sets


def camera_rays(width=64, height=48):
    """One ray per pixel of a pinhole camera: every ray shares the origin, so hi == lo on every axis"""
    x = (np.arange(width) + 0.5) / width * 2.0 - 1.0
    y = (1.0 - (np.arange(height) + 0.5) / height * 2.0) * height / width
    d = np.stack(np.broadcast_arrays(x[None, :], y[:, None], -1.0), -1).reshape(-1, 3)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    o = np.broadcast_to(np.array([0.5, 1.25, 6.0]), d.shape)
    return np.ascontiguousarray(np.hstack([o, d]), np.float32)


def _directions(rng, n):
    d = rng.normal(size=(n, 3))
    return d / np.linalg.norm(d, axis=1, keepdims=True)


def face_rays(n=512, seed=11):
    """Origins in a box, many of them ON its faces, edges and corners (o[a] == lo[a] or hi[a]: the top cell is clamped, not a 256th one)"""
    rng = np.random.default_rng(seed)
    lo, hi = np.array([-3.0, 0.25, -7.5]), np.array([5.0, 0.75, 100.0])
    o = rng.uniform(lo, hi, size=(n, 3))
    pick = rng.integers(0, 3, size=(n, 3))                  # 0 keeps the coordinate, 1 puts it on the low face, 2 on the high face
    o = np.where(pick == 1, lo, np.where(pick == 2, hi, o))
    o[:8] = [[(lo, hi)[(k >> a) & 1][a] for a in range(3)] for k in range(8)]
    return np.ascontiguousarray(np.hstack([o, _directions(rng, n)]), np.float32)


def axis_and_diagonal_rays(seed=12):
    """The six axis directions and the eight octant diagonals -- the corners, the centre and the fold of the octahedral map -- exact and
    scaled by 2^-100 and 2^100 (|d| is not the key's business), from a few origins each"""
    rng = np.random.default_rng(seed)
    dirs = [s * np.eye(3)[a] for a in range(3) for s in (1.0, -1.0)] + [np.array([sx, sy, sz]) for sx in (1.0, -1.0) for sy in (1.0, -1.0) for sz in (1.0, -1.0)]
    rows = []
    for d in dirs:
        for scale in (1.0, 2.0 ** -100, 2.0 ** 100, 1.0 / np.sqrt(3.0)):
            rows.append(np.concatenate([rng.uniform(-2, 2, 3), d * scale]))
    return np.ascontiguousarray(rows, np.float32)


def negative_zero_rays(n=256, seed=13):
    """dz = -0.0 (not < 0: the upper sheet) beside dz = +0.0 and the smallest negative dz; dx or dy of either zero too"""
    rng = np.random.default_rng(seed)
    r = np.hstack([rng.uniform(-1, 1, size=(n, 3)), _directions(rng, n)]).astype(np.float32)
    r[0::4, 5] = -0.0
    r[1::4, 5] = 0.0
    r[2::4, 5] = -np.float32(1e-45)
    r[3::8, 3] = -0.0
    r[5::8, 4] = -0.0
    r[7::16, 3:5] = -0.0
    r[7::16, 5] = -1.0                                      # the lower pole: u = v = -0 / s
    assert np.signbit(r[0, 5]) and r[0, 5] == 0
    return np.ascontiguousarray(r)


def far_rays(n=512, seed=14):
    """Origins beyond 2^40 on some or all axes, up to the largest floats (hi - lo is finite in binary64)"""
    rng = np.random.default_rng(seed)
    o = rng.uniform(-1, 1, size=(n, 3)) * 2.0 ** rng.integers(38, 128, size=(n, 3))
    o[::3, 0] = rng.uniform(-4, 4, size=len(o[::3]))
    o[0], o[1] = np.finfo(np.float32).max, -np.finfo(np.float32).max
    return np.ascontiguousarray(np.hstack([o, _directions(rng, n)]), np.float32)


def unplaced_rays(n=70):
    """No ray is placed: non-finite words and zero directions only"""
    return np.ascontiguousarray(np.resize(np.array(NOT_PLACED + [[0, 0, 0, -0.0, 0.0, -0.0], [1, 2, 3, np.nan, np.nan, np.nan], [-np.inf, 0, 0, 1, 0, 0]], np.float32),
                                          (n, 6)))


def identical_rays(n=4097):
    """One ray n times: one key, the identity -- stability across the sort's tile boundary at 4 096"""
    return np.ascontiguousarray(np.resize(np.array([[0.5, -1.0, 2.0, 0.6, 0.0, -0.8]], np.float32), (n, 6)))


def all_sets(pkg):
    """Every set with placed rays, by name"""
    sets = dict(("adversarial " + k, v) for k, v in adversarial_sets(pkg).items())
    sets.update({"camera": camera_rays(), "faces": face_rays(), "axes and diagonals": axis_and_diagonal_rays(), "negative zero": negative_zero_rays(),
                 "beyond 2^40": far_rays()})
    return sets


def tiled(rays, n):
    """The first n rays of the set repeated to length"""
    return np.ascontiguousarray(np.resize(rays, (n, 6))) if n else np.zeros((0, 6), np.float32)
