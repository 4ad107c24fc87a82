"""Exact geometry for the nearest-primitive query's tests (tests/test_nearest_exact.py), in the manner of tests/exact_mesh.py: the distances
from a point to the f32 scene data in float64 -- a sphere's radius from the stored r * r, as the device keeps it --, the bound the query's
binary32 distances are held to, and why.  Not a test module.

THE BOUNDS.  FAR is the distance from p to the farthest point of the primitive (a sphere: |p - c| + r; a triangle: its farthest vertex; a
plane has no farthest point: |p - pos|, the length every term of its distance is formed from).  csrc/ptmi_nearest.h works in coordinates
relative to p, so every rounding is 2^-24 of something no longer than FAR:
  * a sphere: three subtractions, the sum of three squares, two roots and L - r: under 8 roundings -> 2^-20 FAR;
  * a plane: the same count on e = p - pos and the stored direction, and one division -> 2^-20 FAR;
  * a triangle: its normal is formed from the relative coordinates by Kahan's difference of products, so the cancellation of a thin
    triangle's cross product does not reach it (csrc/ptmi_nearest.h has the argument): the plane's distance within 2^-20 FAR, a foot
    misjudged inside or outside only within 2^-21 FAR of an edge's line, an edge's nearest location within 2^-21 FAR -> 2^-19 FAR,
    whatever the shape.
  * a triangle's SIGN (negative behind the front) is the sign of h = dot(v0 - p, n).  The edges v1 - v0 and v2 - v0 are f32 differences,
    each off by 2^-24 of its length; on a triangle of aspect a = (longest side)^2 / (2 area) that turns the computed plane about the
    long axis by up to 2^-22 a (two edges over a height of side / a).  The plane still passes through v0, so at a foot that lies l from
    v0 in the plane the computed h is off by up to 2^-22 a l beside its own rounding: the sign is held to the exact one wherever
    |h| > bound + min(2^-22 a, 1) l, and nowhere on a needle of aspect 10^7, whose plane binary32 edges do not determine.  (The
    DISTANCE does not suffer: where the foot is inside, l across the long axis is at most the height, and 2^-22 a x side / a is 2^-22 of
    the side.)  The distance is compared unsigned.
So bound_j = 2^-20 FAR_j for spheres and planes and 2^-19 FAR_j for triangles, and the criterion tolerates ties: the reported primitive's
exact distance may exceed the least exact distance by the two bounds involved, no more."""
import numpy as np

EPS = 2.0 ** -20


def _f64(a):
    return np.asarray(a, np.float64)


def sphere_distances(spheres, p):
    """-> (D signed (n, ns), FAR (n, ns))"""
    c = _f64(spheres["position"])
    r32 = spheres["radius"].astype(np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        r = np.sqrt((r32 * r32).astype(np.float64))            # the stored r * r, an f32 product
        L = np.linalg.norm(p[:, None, :] - c[None, :, :], axis=2)
    return L - r[None, :], L + r[None, :]


def plane_distances(planes, p):
    pos, d = _f64(planes["position"]), _f64(planes["direction"])
    with np.errstate(all="ignore"):
        ln = np.linalg.norm(d, axis=1)
        e = p[:, None, :] - pos[None, :, :]
        D = (e * d[None, :, :]).sum(2) / ln[None, :]
        usable = np.isfinite(ln) & (ln > 0)
        ln32 = np.sqrt(((d.astype(np.float32) ** 2).sum(1)).astype(np.float32))      # what binary32 can hold of the length's square
        usable &= np.isfinite(ln32) & (ln32 > 0)
    D = np.where(usable[None, :], D, np.nan)
    return D, np.linalg.norm(e, axis=2)


def _segment(A, B):
    d = B - A
    dd = (d * d).sum(-1)
    with np.errstate(all="ignore"):
        t = np.where(dd > 0, -(A * d).sum(-1) / np.where(dd > 0, dd, 1.0), 0.0)
    t = np.clip(t, 0.0, 1.0)
    return A + d * t[..., None]


def triangle_closest(v0, v1, v2, p):
    """The nearest location of each triangle to each point, by numpy's broadcasting of (v0, v1, v2) against p (all triangles against
    all points as (1, m, 3) against (n, 1, 3), or pairwise as (m, 3) against (m, 3)) -> the location RELATIVE to p, and the signed
    height over the plane (positive: p behind the front)"""
    A, B, C = v0 - p, v1 - p, v2 - p
    n = np.cross(B - A, C - A)
    nn = (n * n).sum(-1)
    with np.errstate(all="ignore"):
        h = (A * n).sum(-1) / np.sqrt(nn)                        # positive: p behind the front
        q = n * ((A * n).sum(-1) / nn)[..., None]
        w0 = (np.cross(B - A, q - A) * n).sum(-1)
        w1 = (np.cross(C - B, q - B) * n).sum(-1)
        w2 = (np.cross(A - C, q - C) * n).sum(-1)
    inside = (w0 >= 0) & (w1 >= 0) & (w2 >= 0) & (nn > 0)
    best = _segment(A, B)
    key = np.linalg.norm(best, axis=-1)
    for X, Y in ((B, C), (C, A)):
        g = _segment(X, Y)
        k = np.linalg.norm(g, axis=-1)
        better = k < key
        best = np.where(better[..., None], g, best)
        key = np.where(better, k, key)
    with np.errstate(all="ignore"):
        kq = np.linalg.norm(q, axis=-1)
    take = inside & (kq <= key)
    best = np.where(take[..., None], q, best)
    return best, h


def triangle_aspects(triangles):
    """(longest side)^2 / (2 area): the longest side over the height above it; inf for no area"""
    v0, v1, v2 = (_f64(triangles[k]) for k in ("v0", "v1", "v2"))
    area2 = np.linalg.norm(np.cross(v1 - v0, v2 - v0), axis=1)
    longest = np.maximum(np.maximum(((v1 - v0) ** 2).sum(1), ((v2 - v1) ** 2).sum(1)), ((v0 - v2) ** 2).sum(1))
    with np.errstate(all="ignore"):
        return np.where(area2 > 0, longest / area2, np.inf)


def kept_triangles(triangles):
    """nn > 0 by the library's f32 operations (ptmi_mesh_box.h: triangle_normal): the triangles that are candidates"""
    f = np.float32
    v0, v1, v2 = (triangles[k].astype(f) for k in ("v0", "v1", "v2"))
    e1, e2 = v1 - v0, v2 - v0
    nx = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]
    ny = e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]
    nz = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
    return (f(nx * nx + ny * ny) + nz * nz) > 0


def triangle_distances(triangles, p, chunk=128):
    """-> (D unsigned (n, nt), FAR (n, nt), bound factor (nt,)); a triangle that is no candidate has D = nan"""
    v0, v1, v2 = (_f64(triangles[k]) for k in ("v0", "v1", "v2"))
    kept = kept_triangles(triangles)
    factor = np.full(len(v0), 2.0 * EPS)
    D = np.empty((len(p), len(v0)))
    FAR = np.empty_like(D)
    for at in range(0, len(p), chunk):
        q = p[at:at + chunk, None, :]
        best, _ = triangle_closest(v0[None], v1[None], v2[None], q)
        D[at:at + chunk] = np.linalg.norm(best, axis=-1)
        FAR[at:at + chunk] = np.maximum(np.maximum(np.linalg.norm(v0[None] - q, axis=-1), np.linalg.norm(v1[None] - q, axis=-1)), np.linalg.norm(v2[None] - q, axis=-1))
    D[:, ~kept] = np.nan
    return D, FAR, factor


def table(spheres, planes, triangles, points):
    """Every primitive's exact distance from every point -> (D signed where a sign is defined (n, N): triangles unsigned), FAR (n, N),
    bound (n, N) = factor FAR; N = ns + np + nt in the query's numbering; no candidate: nan"""
    p = _f64(points)
    cols_d, cols_f, cols_b = [], [], []
    if len(spheres):
        D, F = sphere_distances(spheres, p)
        cols_d.append(D); cols_f.append(F); cols_b.append(EPS * F)
    if len(planes):
        D, F = plane_distances(planes, p)
        cols_d.append(D); cols_f.append(F); cols_b.append(EPS * F)
    if triangles is not None and len(triangles):
        D, F, factor = triangle_distances(triangles, p)
        cols_d.append(D); cols_f.append(F); cols_b.append(factor[None, :] * F)
    return np.concatenate(cols_d, 1), np.concatenate(cols_f, 1), np.concatenate(cols_b, 1)
