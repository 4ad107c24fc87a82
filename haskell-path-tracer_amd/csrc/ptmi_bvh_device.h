// ptmi_bvh_device.h -- checkHit (src/Scene/Trace.hs:443-447) over a BVH scene (ptmi_set_scene_bvh): the spheres through the hierarchy
// ptmi_bvh.cpp builds, the planes folded linearly.  Included by the units whose kernels have BVH instantiations (render Inline, the
// Streams chain, the tree walk) and by the point query (ptmi_small.hip).  DESIGN.md 5.7 summarises what follows.
#pragma once

#include "ptmi_device.h"
#include "../../include/ptmi.h"

namespace ptmi {

namespace {

constexpr int kBvhStack = PTMI_BVH_MAX_DEPTH;   // entries of a lane's traversal stack: at a node of level k at most k are held

// The arithmetic of the walks' box tests (the comment below says what it is for).  Macros, as PTMI_SPHERE_TEST is one, so that every walk
// -- check_hit_bvh, check_hit_mesh's two, the any-hit walks of ptmi_query_device.h -- makes the SAME operations and each keeps its code.
//   PTMI_SLAB_REACH     e = box centre - origin, and the L1 norm p1 and the squared L2 norm p2 of |e| + h: declares ex, ey, ez, p1, p2
//   PTMI_SPHERE_MARGIN  the margin m of a child of the sphere hierarchy (G, G_lin and sqrt_G are the walk's)
//   PTMI_SLAB_TEST      the slab test of the box widened by m: assigns t_near, declares t_far
#define PTMI_SLAB_REACH(c, h, o)                                                                                                    \
    const float ex = c.x - o.x, ey = c.y - o.y, ez = c.z - o.z;                                                                     \
    const float ax = __builtin_fabsf(ex) + h.x, ay = __builtin_fabsf(ey) + h.y, az = __builtin_fabsf(ez) + h.z;                     \
    const float p1 = (ax + ay) + az, p2 = (ax * ax + ay * ay) + az * az
#define PTMI_SPHERE_MARGIN(p1, p2, inv_2r) \
    (((__builtin_fminf(sqrt_G * p1, (G * p2) * inv_2r) + G_lin * p1) + 0x1p-30f) * (1.0f + 0x1p-10f))
#define PTMI_SLAB_TEST(h, m, inv, ainv, far, t_near)                                                                                \
    const float tmx = ex * inv.x, hx = (h.x + m) * ainv.x;                                                                          \
    const float tmy = ey * inv.y, hy = (h.y + m) * ainv.y;                                                                          \
    const float tmz = ez * inv.z, hz = (h.z + m) * ainv.z;                                                                          \
    t_near = __builtin_fmaxf(__builtin_fmaxf(tmx - hx, tmy - hy), __builtin_fmaxf(tmz - hz, 0.0f));                                 \
    const float t_far = __builtin_fminf(__builtin_fminf(tmx + hx, tmy + hy), tmz + hz) * far

// check_hit_bvh returns what check_hit returns, bit for bit:
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
//     runtime-indexed array in registers would go to scratch.  The nearer child is entered first, the farther one pushed.
template <typename ScenePtr>
__device__ __forceinline__ HitSel check_hit_bvh(const BvhView &B, ScenePtr S, int ns, int np, V3 o, V3 d)
{
    __shared__ uint32_t bvh_stack[kBvhStack][kRenderBlock];
    uint32_t *col = &bvh_stack[0][threadIdx.x % kRenderBlock];

    const float eta = __builtin_fabsf(dot(d, d) - 1.0f);
    float P2 = 0.0f;
    {
        const float oc[3] = {o.x, o.y, o.z};
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const float pa = __builtin_fmaxf(__builtin_fabsf(B.lo[a] - oc[a]), __builtin_fabsf(B.hi[a] - oc[a]));
            P2 = P2 + pa * pa;
        }
    }
    const float P = __builtin_sqrtf(P2) * (1.0f + 0x1p-20f);
    const bool finite = __builtin_isfinite(o.x) && __builtin_isfinite(o.y) && __builtin_isfinite(o.z) &&
                        __builtin_isfinite(d.x) && __builtin_isfinite(d.y) && __builtin_isfinite(d.z);
    if (!(finite && eta <= 0x1p-12f && P <= 0x1p40f)) return check_hit<false>(S, ns, np, o, d);

    float best_key = kInfinite;
    int best_idx = 0x7fffffff;
    bool best_just = false;
    if (ns > 0) {
        const float G = 0x1p-19f + 2.0f * eta, G_lin = G + 0x1p-19f, sqrt_G = __builtin_sqrtf(G);
        auto inv_of = [](float v) {
            const float c = __builtin_fabsf(v) < 0x1p-80f ? __builtin_copysignf(0x1p-80f, v) : v;
            return 1.0f / c;
        };
        const V3 inv = mk(inv_of(d.x), inv_of(d.y), inv_of(d.z));
        const V3 ainv = mk(__builtin_fabsf(inv.x), __builtin_fabsf(inv.y), __builtin_fabsf(inv.z));
        constexpr float kFar = 1.0f + 2.0f * (3.0f * 0x1p-24f) / (1.0f - 3.0f * 0x1p-24f);     // 1 + 2 gamma_3

        // entry distance of a child's box (NaN-free operations ignore a NaN operand: a degenerate axis never prunes).  The margin's
        // distance is the child's own: |centre - origin| <= |c - o| + h per axis for every sphere in the box (p1 its L1 norm, p2 the
        // square of its L2 norm), so near boxes -- where bounce rays spend their tests -- get a near-zero margin.
        auto slab = [&](V3 c, V3 h, float inv_2r, float &t_near) {
            PTMI_SLAB_REACH(c, h, o);                        // ex, ey, ez, p1, p2
            const float m = PTMI_SPHERE_MARGIN(p1, p2, inv_2r);
            PTMI_SLAB_TEST(h, m, inv, ainv, kFar, t_near);   // t_near, t_far
            return t_near <= t_far;
        };
        auto leaf = [&](int32_t ref) {
            const uint32_t v = (uint32_t)(-1 - ref);
            const int first = (int)(v >> 8), count = (int)(v & 255u);
            for (int k = 0; k < count; ++k) {
                const float4 g = B.geom[first + k];
                const int i = B.index[first + k];
                PTMI_SPHERE_TEST(g, o, d);                   // check_hit's sphere test (ptmi_device.h): tca, x, cand
                const float t = tca - sqrt_rn(x);
                const bool just = cand && !(t < 0.0f);
                if (just && (t < best_key || (t == best_key && i < best_idx))) { best_key = t; best_idx = i; best_just = true; }
            }
        };

        int node = 0, sp = 0;
        while (true) {
            const float4 f0 = B.nodes[4 * node], f1 = B.nodes[4 * node + 1], f2 = B.nodes[4 * node + 2], f3 = B.nodes[4 * node + 3];
            const int32_t r0 = (int32_t)f2u(f3.x), r1 = (int32_t)f2u(f3.y);
            float t0, t1;
            const bool h0 = slab(mk(f0.x, f0.y, f0.z), mk(f1.z, f1.w, f2.x), f3.z, t0) && r0 != -1 && t0 <= best_key;
            const bool h1 = slab(mk(f0.w, f1.x, f1.y), mk(f2.y, f2.z, f2.w), f3.w, t1) && r1 != -1 && t1 <= best_key;
            const bool swap = h1 && (!h0 || t1 < t0);           // the nearer child first
            const int32_t ra = swap ? r1 : r0, rb = swap ? r0 : r1;
            const bool ha = swap ? h1 : h0, hb = swap ? h0 : h1;
            const float tb = swap ? t0 : t1;
            int next = -1;
            if (ha) {
                if (ra < 0) leaf(ra);
                else next = ra;
            }
            if (hb && tb <= best_key) {
                if (rb < 0) leaf(rb);
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
    }
    if (!best_just) { best_key = __builtin_nanf(""); best_idx = 0; }    // no sphere hit: check_hit's accumulator is still unfilled
    fold_planes([&](int k) -> float4 { return S[ns + k]; }, ns, np, o, d, best_key, best_idx, best_just);   // check_hit's fold
    if (best_just && !(best_key < kInfinite)) return check_hit_exact(S, ns, np, o, d);
    HitSel best; best.t = best_key; best.idx = best_idx; best.just = best_just;
    return best;
}

#ifndef PTMI_BVH_WAVES
#define PTMI_BVH_WAVES 4         // the BVH kernels' LDS -- 6 KB of stack per wave on top of the restart columns -- allows 4 waves per SIMD
#endif

}  // namespace

}  // namespace ptmi
