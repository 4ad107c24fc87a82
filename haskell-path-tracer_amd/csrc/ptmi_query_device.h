// ptmi_query_device.h -- the ANY-HIT walks behind ptmi_occluded_device: "is anything in the way before t_max", over a linear scene, a BVH
// scene and a mesh scene (occluded_linear, occluded_bvh, occluded_mesh).  Included by ptmi_ray_lane_device.h, where a lane of a ray query
// calls them (occluded_ray).  DESIGN.md 5.9 summarises what follows.
#pragma once

#include "ptmi_mesh_device.h"

namespace ptmi {

namespace {

// THE SPECIFICATION is a statement about the closest hit: with h = check_hit (check_hit_bvh, check_hit_mesh) of the ray,
//     occluded = h.just && h.t < t_max            (one f32 compare)
// so a NaN or non-positive t_max answers 0 whatever the scene holds (a Just has !(t < 0)), and +inf asks for a hit with a finite t.
// The walks below answer it without finding h, and stop at the first primitive that decides it:
//   * THE LIMIT.  lim = min(t_max, FLT_MAX).  An OCCLUDER is a primitive whose own test -- PTMI_SPHERE_TEST and sqrt_rn, PTMI_PLANE_DISTANCE,
//     PTMI_TRIANGLE_TEST: the operations check_hit makes, from the same text -- is a Just with t < lim.
//   * WHY ONE OCCLUDER DECIDES.  checkHit is a left fold that keeps its accumulator iff keyA <= keyB, a Nothing keyed FLT_MAX.  While no
//     key of the scene is a NaN that fold returns the first minimum of the keys.  An occluder's key is below FLT_MAX, so the minimum is
//     too: it is a Just's t (every Nothing is keyed FLT_MAX), at most the occluder's, hence < t_max: the answer is 1.  Without an
//     occluder no Just has t < lim; the closest hit could still have t < t_max only with t = FLT_MAX under t_max = +inf, and a Just
//     whose key is not < FLT_MAX sends the lane to the full search (below) wherever it meets one.  Otherwise the answer is 0.
//   * NO KEY IS A NaN -- what the lane establishes before it trusts an early exit:
//       - planes: 0 / 0 is a NaN with finite data (a ray that lies in a plane).  There are few planes (64 at most beside a hierarchy), so
//         the lane tests ALL of them first, and any plane that is a Just with a key that is not < FLT_MAX -- the case in which check_hit
//         and check_hit_bvh fall to check_hit_exact -- sends it to the full search;
//       - spheres: a ray the walk SERVES is finite with | |d|^2 - 1 | <= 2^-12 and no sphere centre farther than 2^40 (the hierarchies'
//         own rule; a linear scene: |o| and every |centre| component and r^2 within 2^40, SceneState.sphere_reach).  Then l, tca, d2 and
//         x = r^2 - d2 are finite (the scene calls refuse a hierarchy's non-finite sphere), a candidate has x >= 0, and t = tca - sqrt x is
//         finite: never a NaN, and below 2^65;
//       - triangles: a NaN t makes the hit point, the three edge functions and their `>= 0` fail: no Just has a NaN key.  (A triangle of
//         zero area has a NaN normal and is never a Just.)  A Just at t = +inf is not excluded by this argument; it is not a NaN, and the
//         lane that meets one takes the full search.
//   * NEVER PRUNE AN OCCLUDER.  The hierarchies are walked by check_hit_bvh's walk (bvh_walk), whose rule check_hit_mesh's is, with the bound held at
//     lim: a child is entered when its widened box (bvh_sphere_slab, mesh_slab: their box tests) is hit at an entry distance
//     t_near <= lim.  Their margins guarantee that a primitive accepted at key t lies under children with t_near <= t; an occluder has
//     t < lim, so every box above it is entered.  What is pruned holds no occluder; what is skipped by leaving early holds no NaN.
//   * THE FULL SEARCH is the closest hit itself -- check_hit, check_hit_bvh behind its admission test (closest_bvh), check_hit_mesh --
//     and the compare: for rays the walk does not serve, and for lanes that met a Just key that is not < FLT_MAX.
//   * THE STACK is check_hit_bvh's column in LDS (bvh_stack_column: one array per kernel, shared with check_hit_mesh and closest_bvh).
enum : int { kAnyNone = 0, kAnyHit = 1, kAnyFull = 2 };      // no occluder met | an occluder | the lane takes the full search

// One Just key against the limit
__device__ __forceinline__ int any_hit_key(bool just, float t, float lim)
{
    if (!just) return kAnyNone;
    if (!(t < kInfinite)) return kAnyFull;
    return t < lim ? kAnyHit : kAnyNone;
}

// All planes (see above): kAnyFull outranks kAnyHit
template <typename ScenePtr>
__device__ __forceinline__ int any_hit_planes(ScenePtr S, int ns, int np, V3 o, V3 d, float lim)
{
    int found = kAnyNone;
    for (int j = 0; j < np; ++j) {
        const float4 gp = S[ns + 2 * j], gn = S[ns + 2 * j + 1];
        const float denom = PTMI_PLANE_DENOM(gn, d);
        if (!(denom > 1e-6f)) {                              // fold_planes' candidates: only they divide
            PTMI_PLANE_DISTANCE(gp, gn, o, denom);           // t, just
            const int r = any_hit_key(just, t, lim);
            found = r > found ? r : found;
        }
    }
    return found;
}

// A linear scene's spheres, in index order; the lane leaves at the first occluder
template <typename ScenePtr>
__device__ __forceinline__ int any_hit_spheres_linear(ScenePtr S, int ns, V3 o, V3 d, float lim)
{
    int found = kAnyNone;
    for (int i = 0; i < ns && found == kAnyNone; ++i) {
        const float4 g = S[i];
        PTMI_SPHERE_TEST(g, o, d);                           // tca, x, cand
        if (cand) {
            const float t = tca - sqrt_rn(x);
            found = any_hit_key(!(t < 0.0f), t, lim);
        }
    }
    return found;
}

// The hierarchies walked with the bound held at lim, leaving at the first primitive that answers
__device__ __forceinline__ int any_hit_spheres(const BvhView &B, uint32_t *col, V3 o, V3 d, float eta, float lim)
{
    return bvh_walk(B.nodes, col, [=]() { return lim; }, bvh_sphere_slab(o, d, eta), [&](int first, int count) {
        for (int k = 0; k < count; ++k) {
            float t;
            const bool just = bvh_sphere_just(B.geom[first + k], o, d, t);
            const int r = any_hit_key(just, t, lim);
            if (r != kAnyNone) return r;
        }
        return (int)kAnyNone;
    });
}

__device__ __forceinline__ int any_hit_triangles(const MeshView &M, uint32_t *col, V3 o, V3 d, float lim)
{
    return bvh_walk(M.nodes, col, [=]() { return lim; }, mesh_slab(o, d), [&](int first, int count) {
        for (int k = 0; k < count; ++k) {
            const float4 ga = M.geom[3 * (first + k)], gb = M.geom[3 * (first + k) + 1], gc = M.geom[3 * (first + k) + 2];
            PTMI_TRIANGLE_TEST(ga, gb, gc, o, d);            // t, just
            const int r = any_hit_key(just, t, lim);
            if (r != kAnyNone) return r;
        }
        return (int)kAnyNone;
    });
}

__device__ __forceinline__ bool occluded_by(HitSel h, float t_max) { return h.just && h.t < t_max; }

// ---- the three scene kinds ----
// A linear scene.  reach: SceneState.sphere_reach, the largest |centre component| or r^2 of its spheres (+inf when one is not finite)
template <SphereShare SHARE, typename ScenePtr>
__device__ __forceinline__ bool occluded_linear(ScenePtr S, int ns, int np, unsigned long long share, float reach, V3 o, V3 d, float t_max)
{
    if (!(t_max > 0.0f)) return false;
    const float lim = __builtin_fminf(t_max, kInfinite);
    const float oo = __builtin_fmaxf(__builtin_fmaxf(__builtin_fabsf(o.x), __builtin_fabsf(o.y)), __builtin_fabsf(o.z));
    int found = kAnyFull;
    if (bvh_ray_finite(o, d) && bvh_eta(d) <= 0x1p-12f && oo <= 0x1p40f && reach <= 0x1p40f) {
        found = any_hit_planes(S, ns, np, o, d, lim);
        if (found == kAnyNone) found = any_hit_spheres_linear(S, ns, o, d, lim);
    }
    if (found != kAnyFull) return found == kAnyHit;
    return occluded_by(check_hit<false, SphereFold::kStash, SHARE>(S, ns, np, o, d, nullptr, share), t_max);
}

template <typename ScenePtr>
__device__ __forceinline__ bool occluded_bvh(const BvhView &B, ScenePtr S, int ns, int np, V3 o, V3 d, float t_max)
{
    if (!(t_max > 0.0f)) return false;
    uint32_t *col = bvh_stack_column();
    const float lim = __builtin_fminf(t_max, kInfinite);
    const float eta = bvh_eta(d);
    if (!(bvh_ray_finite(o, d) && eta <= 0x1p-12f && bvh_reach(B.lo, B.hi, o) <= 0x1p40f))
        return occluded_by(check_hit<false>(S, ns, np, o, d), t_max);          // check_hit_bvh's answer for such a ray
    int found = any_hit_planes(S, ns, np, o, d, lim);
    if (found == kAnyNone && ns > 0) found = any_hit_spheres(B, col, o, d, eta, lim);
    if (found != kAnyFull) return found == kAnyHit;
    return occluded_by(closest_bvh(B, col, S, ns, np, o, d, eta), t_max);
}

template <typename ScenePtr>
__device__ __forceinline__ bool occluded_mesh(const MeshView &M, ScenePtr S, int ns, int np, V3 o, V3 d, float t_max)
{
    if (!(t_max > 0.0f)) return false;
    uint32_t *col = bvh_stack_column();
    const float lim = __builtin_fminf(t_max, kInfinite);
    const float eta = bvh_eta(d);
    const float P = __builtin_fmaxf(bvh_reach(M.spheres.lo, M.spheres.hi, o), bvh_reach(M.lo, M.hi, o));
    int found = kAnyFull;
    if (bvh_ray_finite(o, d) && eta <= 0x1p-12f && P <= 0x1p40f) {
        found = any_hit_planes(S, ns, np, o, d, lim);
        if (found == kAnyNone && ns > 0) found = any_hit_spheres(M.spheres, col, o, d, eta, lim);
        if (found == kAnyNone && M.n_kept > 0) found = any_hit_triangles(M, col, o, d, lim);
    }
    if (found != kAnyFull) return found == kAnyHit;
    return occluded_by(check_hit_mesh(M, S, ns, np, o, d), t_max);
}

}  // namespace

}  // namespace ptmi
