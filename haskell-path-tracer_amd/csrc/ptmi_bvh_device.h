// ptmi_bvh_device.h -- checkHit (src/Scene/Trace.hs:443-447) over a BVH scene (ptmi_set_scene_bvh): the spheres through the hierarchy
// ptmi_bvh.cpp builds, the planes folded linearly.  Included by the units whose kernels have BVH instantiations (render Inline, the
// Streams chain, the tree walk) and by the point query (ptmi_small.hip).  DESIGN.md 5.7 summarises what follows.
#pragma once

#include "ptmi_device.h"
#include "../../include/ptmi.h"

namespace ptmi {

namespace {

constexpr int kBvhStack = PTMI_BVH_MAX_DEPTH;   // entries of a lane's traversal stack: at a node of level k at most k are held

// check_hit_bvh (at the end of this header, from the parts before it) returns what check_hit returns, bit for bit:
//   * SAME ARITHMETIC: every sphere it tests is tested by check_hit's operations (sqrt_rn included);
//   * SAME CHOICE: among the spheres the minimum of (key, original index) -- for finite keys the left fold's first minimum -- then the
//     planes folded as check_hit folds them (a strict `<` against the accumulator, which starts as NaN when no sphere hit: an
//     accumulator check_hit never filled);
//   * NEVER PRUNE THE WINNER: a child is entered when its box is hit at an entry distance <= the best key (not <: a tie is decided by
//     the index).  The box test is a slab test on (centre, half extent) with the half extent widened by a margin m for the rounding
//     of the sphere test at distance P (P bounds |sphere centre - origin| over the child's box): m = min(sqrt(G) P, G P^2 / (2 r_min))
//     + (G + 2^-19) P + 2^-30, G = 2^-19 + 2 | |d|^2 - 1 |, widened by 2^-10 for its own rounding, and the far distance multiplied by
//     1 + 2 gamma_3 (Ize, "Robust BVH Ray Traversal", 2013).  A component of d below 2^-80 in magnitude is taken as +-2^-80: no
//     0 * inf in the slab test, and the change of the ray is far inside the margin;
//   * WHAT THE HIERARCHY DOES NOT SERVE: a ray with a non-finite component, | |d|^2 - 1 | > 2^-12 (every ray the renderer makes is
//     within a few 10^-6) or a sphere centre farther than 2^40 takes check_hit over the whole scene (the linear fold, for that lane); a final key that is
//     not < FLT_MAX (non-finite plane data) takes the literal fold (check_hit_exact), as in check_hit.
//   * THE STACK lives in LDS, one column of kBvhStack words per lane (6 KB per wave), indexed by the lane's stack pointer: a
//     runtime-indexed array in registers would go to scratch.  One array per kernel, whichever searches it runs.  The nearer child is
//     entered first, the farther one pushed.
__device__ __forceinline__ uint32_t *bvh_stack_column()
{
    __shared__ uint32_t bvh_stack[kBvhStack][kRenderBlock];
    return &bvh_stack[0][threadIdx.x % kRenderBlock];
}

// What the lane's ray may take from a hierarchy: eta = | |d|^2 - 1 |, P >= the distance from the origin to the box (lo, hi)
__device__ __forceinline__ float bvh_eta(V3 d) { return __builtin_fabsf(dot(d, d) - 1.0f); }
__device__ __forceinline__ float bvh_reach(const float lo[3], const float hi[3], V3 o)
{
    float P2 = 0.0f;
    const float oc[3] = {o.x, o.y, o.z};
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float pa = __builtin_fmaxf(__builtin_fabsf(lo[a] - oc[a]), __builtin_fabsf(hi[a] - oc[a]));
        P2 = P2 + pa * pa;
    }
    return __builtin_sqrtf(P2) * (1.0f + 0x1p-20f);
}
__device__ __forceinline__ bool bvh_ray_finite(V3 o, V3 d)
{
    return __builtin_isfinite(o.x) && __builtin_isfinite(o.y) && __builtin_isfinite(o.z) &&
           __builtin_isfinite(d.x) && __builtin_isfinite(d.y) && __builtin_isfinite(d.z);
}

// The two-child stack walk, of either hierarchy and for either question.  A child is entered when slab(c, h, inv_2r, t_near) hits its
// box at an entry distance t_near <= bound(), the nearer child first; leaf(first, count) tests the primitives at positions [first,
// first + count) of the leaf order, and a non-zero return ends the walk with that value.  bound() may move with what leaf() found:
// the farther child is held to it again after the nearer one's leaf.
template <typename Bound, typename Slab, typename Leaf>
__device__ __forceinline__ int bvh_walk(const float4 *nodes, uint32_t *col, Bound bound, Slab slab, Leaf leaf)
{
    auto at_leaf = [&](int32_t ref) {
        const uint32_t v = (uint32_t)(-1 - ref);
        return leaf((int)(v >> 8), (int)(v & 255u));
    };
    int node = 0, sp = 0;
    while (true) {
        const float4 f0 = nodes[4 * node], f1 = nodes[4 * node + 1], f2 = nodes[4 * node + 2], f3 = nodes[4 * node + 3];
        const int32_t r0 = (int32_t)f2u(f3.x), r1 = (int32_t)f2u(f3.y);
        float t0, t1;
        const bool h0 = slab(mk(f0.x, f0.y, f0.z), mk(f1.z, f1.w, f2.x), f3.z, t0) && r0 != -1 && t0 <= bound();
        const bool h1 = slab(mk(f0.w, f1.x, f1.y), mk(f2.y, f2.z, f2.w), f3.w, t1) && r1 != -1 && t1 <= bound();
        const bool swap = h1 && (!h0 || t1 < t0);           // the nearer child first
        const int32_t ra = swap ? r1 : r0, rb = swap ? r0 : r1;
        const bool ha = swap ? h1 : h0, hb = swap ? h0 : h1;
        const float tb = swap ? t0 : t1;
        int next = -1;
        if (ha) {
            if (ra < 0) { const int r = at_leaf(ra); if (r != 0) return r; }
            else next = ra;
        }
        if (hb && tb <= bound()) {
            if (rb < 0) { const int r = at_leaf(rb); if (r != 0) return r; }
            else if (next < 0) next = rb;
            else { col[sp * kRenderBlock] = (uint32_t)rb; ++sp; }
        }
        if (next < 0) {
            if (sp == 0) break;
            --sp;
            next = (int)col[sp * kRenderBlock];
        }
        node = next;
    }
    return 0;
}

// A walk's ray: 1 / d per component, |component| taken as at least 2^-80 (see above)
struct BvhRay { V3 o, inv, ainv; };
__device__ __forceinline__ BvhRay bvh_ray(V3 o, V3 d)
{
    auto inv_of = [](float v) {
        const float c = __builtin_fabsf(v) < 0x1p-80f ? __builtin_copysignf(0x1p-80f, v) : v;
        return 1.0f / c;
    };
    BvhRay R;
    R.o = o;
    R.inv = mk(inv_of(d.x), inv_of(d.y), inv_of(d.z));
    R.ainv = mk(__builtin_fabsf(R.inv.x), __builtin_fabsf(R.inv.y), __builtin_fabsf(R.inv.z));
    return R;
}

// The box test of both hierarchies: the slab test of the box (c, h) widened by m = margin(p1, p2), p1 the L1 norm and p2 the squared L2
// norm of |c - o| + h.  Assigns the entry distance (NaN-free operations ignore a NaN operand: a degenerate axis never prunes).
template <typename Margin>
__device__ __forceinline__ bool bvh_slab(const BvhRay &R, V3 c, V3 h, Margin margin, float &t_near)
{
    const float ex = c.x - R.o.x, ey = c.y - R.o.y, ez = c.z - R.o.z;
    const float ax = __builtin_fabsf(ex) + h.x, ay = __builtin_fabsf(ey) + h.y, az = __builtin_fabsf(ez) + h.z;
    const float m = margin((ax + ay) + az, (ax * ax + ay * ay) + az * az);
    constexpr float kFar = 1.0f + 2.0f * (3.0f * 0x1p-24f) / (1.0f - 3.0f * 0x1p-24f);     // 1 + 2 gamma_3
    const float tmx = ex * R.inv.x, hx = (h.x + m) * R.ainv.x;
    const float tmy = ey * R.inv.y, hy = (h.y + m) * R.ainv.y;
    const float tmz = ez * R.inv.z, hz = (h.z + m) * R.ainv.z;
    t_near = __builtin_fmaxf(__builtin_fmaxf(tmx - hx, tmy - hy), __builtin_fmaxf(tmz - hz, 0.0f));
    return t_near <= __builtin_fminf(__builtin_fminf(tmx + hx, tmy + hy), tmz + hz) * kFar;
}

// The sphere hierarchy's box test for the ray (o, d).  The margin's distance is the child's own: |centre - origin| <= |c - o| + h per
// axis for every sphere in the box, so near boxes -- where bounce rays spend their tests -- get a near-zero margin.
__device__ __forceinline__ auto bvh_sphere_slab(V3 o, V3 d, float eta)
{
    const float G = 0x1p-19f + 2.0f * eta, G_lin = G + 0x1p-19f, sqrt_G = __builtin_sqrtf(G);
    const BvhRay R = bvh_ray(o, d);
    return [=](V3 c, V3 h, float inv_2r, float &t_near) {
        auto margin = [=](float p1, float p2) {
            return ((__builtin_fminf(sqrt_G * p1, (G * p2) * inv_2r) + G_lin * p1) + 0x1p-30f) * (1.0f + 0x1p-10f);
        };
        return bvh_slab(R, c, h, margin, t_near);
    };
}

// check_hit's sphere test (ptmi_device.h) of a leaf's sphere g: its t, and whether it is a Just
__device__ __forceinline__ bool bvh_sphere_just(float4 g, V3 o, V3 d, float &t)
{
    PTMI_SPHERE_TEST(g, o, d);                               // tca, x, cand
    t = tca - sqrt_rn(x);
    return cand && !(t < 0.0f);
}

// The sphere walk: the minimum of (key, original index) over the spheres into (best_key, best_idx, best_just), which start as
// (kInfinite, 0x7fffffff, false)
__device__ __forceinline__ void bvh_walk_spheres(const BvhView &B, uint32_t *col, V3 o, V3 d, float eta, float &best_key, int &best_idx, bool &best_just)
{
    bvh_walk(B.nodes, col, [&]() { return best_key; }, bvh_sphere_slab(o, d, eta), [&](int first, int count) {
        for (int k = 0; k < count; ++k) {
            const float4 g = B.geom[first + k];
            const int i = B.index[first + k];
            float t;
            const bool just = bvh_sphere_just(g, o, d, t);
            if (just && (t < best_key || (t == best_key && i < best_idx))) { best_key = t; best_idx = i; best_just = true; }
        }
        return 0;
    });
}

// The planes folded as check_hit folds them, after the spheres
template <typename ScenePtr>
__device__ __forceinline__ void bvh_fold_planes(ScenePtr S, int ns, int np, V3 o, V3 d, float &best_key, int &best_idx, bool &best_just)
{
    if (!best_just) { best_key = __builtin_nanf(""); best_idx = 0; }    // no sphere hit: check_hit's accumulator is still unfilled
    fold_planes([&](int k) -> float4 { return S[ns + k]; }, ns, np, o, d, best_key, best_idx, best_just);   // check_hit's fold
}

// The closest hit of a ray the hierarchy serves, on the caller's stack: the minimum of (key, original index) over the spheres, then
// the planes folded as check_hit folds them
template <typename ScenePtr>
__device__ __forceinline__ HitSel closest_bvh(const BvhView &B, uint32_t *col, ScenePtr S, int ns, int np, V3 o, V3 d, float eta)
{
    float best_key = kInfinite;
    int best_idx = 0x7fffffff;
    bool best_just = false;
    if (ns > 0) bvh_walk_spheres(B, col, o, d, eta, best_key, best_idx, best_just);
    bvh_fold_planes(S, ns, np, o, d, best_key, best_idx, best_just);
    if (best_just && !(best_key < kInfinite)) return check_hit_exact(S, ns, np, o, d);
    HitSel best; best.t = best_key; best.idx = best_idx; best.just = best_just;
    return best;
}

template <typename ScenePtr>
__device__ __forceinline__ HitSel check_hit_bvh(const BvhView &B, ScenePtr S, int ns, int np, V3 o, V3 d)
{
    const float eta = bvh_eta(d);
    const float P = bvh_reach(B.lo, B.hi, o);
    const bool finite = bvh_ray_finite(o, d);
    if (!(finite && eta <= 0x1p-12f && P <= 0x1p40f)) return check_hit<false>(S, ns, np, o, d);
    return closest_bvh(B, bvh_stack_column(), S, ns, np, o, d, eta);
}

#ifndef PTMI_BVH_WAVES
#define PTMI_BVH_WAVES 4         // the BVH kernels' LDS -- 6 KB of stack per wave on top of the restart columns -- allows 4 waves per SIMD
#endif

}  // namespace

}  // namespace ptmi
