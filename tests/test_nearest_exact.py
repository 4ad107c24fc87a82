"""The nearest-primitive query's host twin (binding.nearest -> ptmi_nearest, the definition the device is held to) against exact geometry:
float64 distances from the f32 scene data (tests/exact_nearest.py, which derives the bounds).  For EVERY point -- the criterion
tolerates ties, so none is left out:
  * the reported distance is the reported primitive's exact distance within that primitive's bound (signed for spheres and planes);
  * the reported primitive's exact distance exceeds the least exact distance over all primitives by at most the two bounds involved;
  * the reported location lies at the reported distance from the point and on the primitive, within the bound and the last rounding of its
    own absolute coordinates (an ulp a component: sqrt(3) 2^-23 of the largest); a triangle's distance is negative behind its front wherever binary32 edges
    determine the side (exact_nearest.py);
  * under r_max the winner's key is < r_max, a primitive that qualifies by more than its bound is not missed, and a miss is the record.
Scenes: any_hit_rays.sphere_scenes() and linear_scenes(); mesh_rays' families at every placement, needles_1e7 included; the mixed room at
scales 1e-3 and 1e3 and at an offset of 1e6; a scene with a sphere of radius 0, a duplicated sphere (the tie goes to the lower index), a
plane with a zero normal and triangles of zero area.  Points: nearest_points.points -- inside the box, on surfaces, at sphere centres, on
triangle edges and vertices, 2^14 .. 2^20 diagonals away, non-finite words.  r_max: absent, and nearest_points.aimed_r_max's families
(NaN, <= 0, just above, at and just below the winner's key)."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import any_hit_rays as A  # noqa: E402
import exact_nearest as X  # noqa: E402
import mesh_rays  # noqa: E402
import nearest_points as N  # noqa: E402

B = N.B
N_POINTS = 700
TINY = 2.0 ** -100                                   # below every scene's scale: a distance of exactly 0 against a bound of exactly 0


def check(name, spheres, planes, triangles, seed=0):
    pts = N.points(spheres, planes, triangles, N_POINTS, seed=seed)
    ns, npl = len(spheres), len(planes)
    finite = np.isfinite(pts).all(1)
    with np.errstate(all="ignore"):
        D, _, bound = X.table(spheres, planes, triangles, pts)
        key = np.abs(D)
        bound = bound + TINY
    d0, i0, _ = B.nearest(spheres, planes, triangles, pts, None, point=True)
    worst, signs = 0.0, 0
    for r_max in (None, N.aimed_r_max(d0, i0)):
        dist, idx, at = B.nearest(spheres, planes, triangles, pts, r_max, point=True)
        lim = np.full(len(pts), np.inf) if r_max is None else r_max.astype(np.float64)
        found = idx >= 0
        assert not found[~finite].any(), name
        miss = ~found
        assert (dist[miss] == 0).all() and (at[miss] == 0).all(), name
        with np.errstate(all="ignore"):
            surely = (key + bound < lim[:, None]) & finite[:, None] & (lim > 0)[:, None]      # qualifies whatever the rounding
        assert not (miss & surely.any(1)).any(), (name, np.flatnonzero(miss & surely.any(1))[:5])
        f = np.flatnonzero(found)
        j = idx[f]
        Dj, bj = D[f, j], bound[f, j]
        assert np.isfinite(Dj).all(), (name, "a primitive that is no candidate was reported")
        assert (np.abs(dist[f]) < lim[f]).all(), name
        signed = j < ns + npl
        err = np.where(signed, np.abs(dist[f].astype(np.float64) - Dj), np.abs(np.abs(dist[f].astype(np.float64)) - np.abs(Dj)))
        bad = err > bj
        assert not bad.any(), "%s: distance off its primitive's exact one beyond the bound at %d points, e.g. point %d %r: %r of primitive %d, exact %r, bound %r" % (
            name, bad.sum(), f[bad][0], pts[f[bad][0]], dist[f[bad][0]], j[bad][0], Dj[bad][0], bj[bad][0])
        worst = max(worst, float((err / bj).max()) if len(f) else 0.0)
        # the least exact distance among those that surely qualify
        with np.errstate(all="ignore"):
            cand = np.where(surely[f], key[f], np.inf)
        jm = np.argmin(cand, axis=1)
        least, bl = cand[np.arange(len(f)), jm], bound[f, jm]
        has = np.isfinite(least)
        late = has & (np.abs(Dj) > least + bj + bl)
        assert not late.any(), "%s: a nearer primitive exists beyond the two bounds at %d points, e.g. point %d %r: primitive %d at %r, primitive %d at %r" % (
            name, late.sum(), f[late][0], pts[f[late][0]], j[late][0], Dj[late][0], jm[late][0], least[late][0])
        # the location
        p64, a64 = pts[f].astype(np.float64), at[f].astype(np.float64)
        own = 3.0 ** 0.5 * 2.0 ** -23 * np.maximum(np.abs(p64).max(1), np.abs(a64).max(1))      # the location's own last rounding: an ulp a component
        tol = bj + own
        off = np.abs(np.linalg.norm(a64 - p64, axis=1) - np.abs(dist[f].astype(np.float64)))
        assert (off <= tol).all(), (name, "the location is not at the reported distance", f[off > tol][:5])
        on = np.zeros(len(f))
        s_ = j < ns
        if s_.any():
            c = spheres["position"][j[s_]].astype(np.float64)
            r32 = spheres["radius"][j[s_]].astype(np.float32)
            on[s_] = np.abs(np.linalg.norm(a64[s_] - c, axis=1) - np.sqrt((r32 * r32).astype(np.float64)))
        p_ = (j >= ns) & (j < ns + npl)
        if p_.any():
            pos, d = planes["position"][j[p_] - ns].astype(np.float64), planes["direction"][j[p_] - ns].astype(np.float64)
            on[p_] = np.abs(((a64[p_] - pos) * d).sum(1) / np.linalg.norm(d, axis=1))
        t_ = j >= ns + npl
        if t_.any():
            tt = triangles[j[t_] - ns - npl]
            best, _ = X.triangle_closest(tt["v0"].astype(np.float64), tt["v1"].astype(np.float64), tt["v2"].astype(np.float64), a64[t_])
            on[t_] = np.linalg.norm(best, axis=1)
            # the sign: negative behind the front, wherever the exact height over the plane exceeds the bound
            _, h = X.triangle_closest(tt["v0"].astype(np.float64), tt["v1"].astype(np.float64), tt["v2"].astype(np.float64), p64[t_])
            A0 = tt["v0"].astype(np.float64) - p64[t_]
            lever = np.sqrt(np.maximum((A0 * A0).sum(1) - h * h, 0.0))                  # from v0 to the foot, in the plane
            clear = np.abs(h) > bj[t_] + np.minimum(2.0 ** -22 * X.triangle_aspects(tt), 1.0) * lever      # exact_nearest.py: the sign's domain
            wrong = clear & ((dist[f][t_] < 0) != (h > 0))
            assert not wrong.any(), (name, "a triangle's distance has the wrong sign", f[t_][wrong][:5], dist[f][t_][wrong][:5], h[wrong][:5])
            signs += int(clear.sum())
        assert (on <= tol).all(), (name, "the location is not on the primitive", f[on > tol][:5], on[on > tol][:5], tol[on > tol][:5])
    if triangles is not None and len(triangles) and np.median(X.triangle_aspects(triangles)) < 2.0 ** 18:
        assert signs >= 100, (name, signs)
    print("\n%s: %d points, %d answers without r_max; the largest |dist - D| / bound %.3f; triangle signs checked %d" % (
        name, len(pts), int((i0 >= 0).sum()), worst, signs))
    return d0, i0


@pytest.mark.parametrize("name", [name for name, _ in A.sphere_scenes()])
def test_sphere_scenes(name):
    s, p = dict(A.sphere_scenes())[name]
    check(name, s, p, None, seed=1)


@pytest.mark.parametrize("name", [c[0] for c in A.linear_scenes()])
def test_linear_scenes(name):
    s, p = {c[0]: (c[1], c[2]) for c in A.linear_scenes()}[name]
    check(name, s, p, None, seed=2)


@pytest.mark.parametrize("placement", list(mesh_rays.PLACEMENTS))
@pytest.mark.parametrize("family", A.MESH_FAMILIES)
def test_mesh_families_at_every_placement(family, placement):
    s, t, p = mesh_rays.placed(family, placement, seed=1)
    check("%s, %s" % (family, placement), s, p, np.ascontiguousarray(t, B.TRIANGLE_DTYPE), seed=3)


@pytest.mark.parametrize("scale,offset", [(1e-3, (0.0, 0.0, 0.0)), (1e3, (0.0, 0.0, 0.0)), (1.0, (1e6, 1e6, 1e6))])
def test_the_mixed_room_scaled_and_offset(scale, offset):
    s, t, p = mesh_rays.transformed(mesh_rays.mixed_room(seed=1), scale, offset)
    check("mixed x %g + %r" % (scale, offset), s, p, np.ascontiguousarray(t, B.TRIANGLE_DTYPE), seed=4)


def test_radius_zero_a_duplicate_a_zero_normal_and_zero_areas():
    s, t, p = mesh_rays.mixed_room(seed=1)
    s = np.concatenate([s, s[:1], s[:2]]).copy()
    zero, dup = len(s) - 3, len(s) - 2               # s[dup] is s[0] again; s[zero] a copy of s[0] with radius 0
    s["radius"][zero] = 0.0
    s["position"][zero] += np.float32(0.37)
    p = np.concatenate([p, p[:1]]).copy()
    p["direction"][-1] = 0.0
    t = np.ascontiguousarray(t, B.TRIANGLE_DTYPE)
    assert (~X.kept_triangles(t)).sum() >= 5
    d0, i0 = check("special cases", s, p, t, seed=5)
    rng = np.random.default_rng(77)
    u = rng.normal(size=(64, 3))
    on0 = np.ascontiguousarray(s["position"][0].astype(np.float64) + float(s["radius"][0]) * u / np.linalg.norm(u, axis=1, keepdims=True), np.float32)
    i_on0 = B.nearest(s, p, t, on0)[1]
    assert (i0 != dup).all() and (i_on0 != dup).all() and (i_on0 == 0).sum() >= 16, "the tie between a sphere and its duplicate goes to the lower index"
    assert (i0 != len(s) + len(p) - 1).all(), "a plane with a zero normal is no candidate"
    flat = np.flatnonzero(~X.kept_triangles(t)) + len(s) + len(p)
    assert not np.isin(i0, flat).any(), "a triangle of zero area is no candidate"
    # at the centre of the sphere of radius 0: distance 0 to it, the location the centre
    c = np.ascontiguousarray(s["position"][zero:zero + 1], np.float32)
    d, i, at = B.nearest(s, p, t, c, None, point=True)
    assert (float(d[0]), int(i[0])) == (0.0, zero) and (at[0] == c[0]).all()
