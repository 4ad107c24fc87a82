// ptmi_mesh_device.h -- checkHit (src/Scene/Trace.hs:443-447) over a MESH scene (ptmi_set_scene_mesh): the fold over
// spheres ++ planes ++ triangles, the spheres through ptmi_bvh.cpp's hierarchy, the planes folded linearly, the triangles through the
// second hierarchy ptmi_mesh.cpp builds.  Included by the units whose kernels have mesh instantiations and by the point query.
// DESIGN.md 5.8 summarises what follows.
#pragma once

#include "ptmi_bvh_device.h"

namespace ptmi {

namespace {

// THE TRIANGLE TEST (an extension: the reference has no triangle).  A record is (v0, nx) (v1, ny) (v2, nz), n the unit normal the host
// derived once (ptmi_mesh.cpp).  Every operation is an f32 operation rounded on its own, in this order (tests/cxx/mesh_traverse.c
// restates it verbatim):
//   denom = dot(d, n);  cand = !(denom > 1e-6)                            distanceTo @Plane (Intersection.hs:57-62) with position v0
//   t = dot(v0 - o, n) / denom
//   p = o + d ^* t                                                        the hit position, as hit_record computes it
//   w0 = dot(cross(v1 - v0, p - v0), n),  w1 = dot(cross(v2 - v1, p - v1), n),  w2 = dot(cross(v0 - v2, p - v2), n)
//   Just t  iff  cand && !(t < 0) && w0 >= 0 && w1 >= 0 && w2 >= 0       (edges and vertices are inside)
// Declares t and just.  A macro, so that the hierarchy's leaves and the folds over all triangles make the SAME operations.
#define PTMI_TRIANGLE_TEST(ga, gb, gc, o, d)                                                                                        \
    const V3 tv0 = mk(ga.x, ga.y, ga.z), tv1 = mk(gb.x, gb.y, gb.z), tv2 = mk(gc.x, gc.y, gc.z);                                    \
    const V3 tn = mk(ga.w, gb.w, gc.w);                                                                                             \
    const float tdenom = dot(d, tn);                                                                                                \
    const float t = dot(tv0 - o, tn) / tdenom;                                                                                      \
    const V3 tp = o + scale_r(d, t);                                                                                                \
    const float tw0 = dot(cross(tv1 - tv0, tp - tv0), tn);                                                                          \
    const float tw1 = dot(cross(tv2 - tv1, tp - tv1), tn);                                                                          \
    const float tw2 = dot(cross(tv0 - tv2, tp - tv2), tn);                                                                          \
    const bool just = !(tdenom > 1e-6f) && !(t < 0.0f) && tw0 >= 0.0f && tw1 >= 0.0f && tw2 >= 0.0f

// The fold over spheres ++ planes ++ triangles written out literally (every primitive in order, a Nothing keyed FLT_MAX): what the
// hierarchy gives up on -- a ray it does not serve, a final key that is not < FLT_MAX.  A triangle of zero area (NaN normal) is a Nothing.
// (Not inlined: it calls check_hit_exact, so its frame -- 16 bytes of scratch in every mesh kernel -- holds the return address.  A unit
// whose kernels have the registers to spare defines PTMI_MESH_EXACT_INLINE as __forceinline__ before it includes this header: the fold is
// then part of the kernel, calls check_hit_exact as a leaf and needs no frame -- ptmi_query.hip, whose kernels LDS holds to four waves.)
#ifndef PTMI_MESH_EXACT_INLINE
#define PTMI_MESH_EXACT_INLINE __noinline__
#endif
template <typename ScenePtr>
__device__ PTMI_MESH_EXACT_INLINE HitSel check_hit_mesh_exact(const float4 *by_index, int n_triangles, ScenePtr S, int ns, int np, V3 o, V3 d)
{
    HitSel best = check_hit_exact(S, ns, np, o, d);
    float best_key = best.just ? best.t : kInfinite;
    for (int k = 0; k < n_triangles; ++k) {
        const float4 ga = by_index[3 * k], gb = by_index[3 * k + 1], gc = by_index[3 * k + 2];
        PTMI_TRIANGLE_TEST(ga, gb, gc, o, d);
        const bool hit = just && !__builtin_isnan(ga.w);
        const float key = hit ? t : kInfinite;
        if ((ns + np == 0 && k == 0) || !(best_key <= key)) { best_key = key; best.t = t; best.idx = ns + np + k; best.just = hit; }
    }
    return best;
}

// The triangle hierarchy's box test for the ray (o, d): the margin of check_hit_mesh's comment, o1 the L1 norm of the origin
__device__ __forceinline__ auto mesh_slab(V3 o, V3 d)
{
    const BvhRay R = bvh_ray(o, d);
    const float o1 = (__builtin_fabsf(o.x) + __builtin_fabsf(o.y)) + __builtin_fabsf(o.z);
    return [=](V3 c, V3 h, float, float &t_near) {
        return bvh_slab(R, c, h, [=](float p1, float) { return ((p1 + o1) * 0x1p-16f + 0x1p-30f) * (1.0f + 0x1p-10f); }, t_near);
    };
}

// check_hit_mesh returns what the fold over spheres ++ planes ++ triangles returns, bit for bit:
//   * the spheres and the planes as check_hit_bvh finds them (the same walk, the same plane fold, the same stack);
//   * then the triangle hierarchy, the accumulator carried in: a triangle replaces it where the fold's `<=` fails, or at an equal key
//     when the accumulator is a triangle of higher index (a sphere or plane always has the lower index, so it keeps every tie);
//   * NEVER PRUNE THE WINNER.  A triangle accepted at key t has its float hit point p = o + d t within the triangle up to the rounding
//     of the edge functions (<= 8 eps |p - v_k| in the plane), off its plane by the rounding of t (<= 3 eps t + 4 eps |v0 - o|: the
//     relative error of denom only moves p along the ray, and p stays in the triangle's prism), and p itself is o + d t up to
//     eps (|o| + |p|).  With D >= |v - o| over the child's box (p1 below, the L1 norm of |c - o| + h) and |o| <= |o|_1, every term is
//     below 24 eps (D + |o|_1) + eps (|v| + L) (L the triangle's extent): the host pads each triangle's box by 2^-16 (max |v| + L)
//     (ptmi_mesh.cpp) and the walk widens each child by m = (2^-16 (p1 + |o|_1) + 2^-30)(1 + 2^-10), 2^8 times the bound, which also
//     covers the slab test's own rounding; the far distance is multiplied by Ize's 1 + 2 gamma_3, as for the spheres;
//   * WHAT THE HIERARCHIES DO NOT SERVE -- a non-finite ray, | |d|^2 - 1 | > 2^-12, a box farther than 2^40 -- and a final key that is not
//     < FLT_MAX take the literal fold (check_hit_mesh_exact).
template <typename ScenePtr>
__device__ __forceinline__ HitSel check_hit_mesh(const MeshView &M, ScenePtr S, int ns, int np, V3 o, V3 d)
{
    uint32_t *col = bvh_stack_column();
    const float eta = bvh_eta(d);
    const float P = __builtin_fmaxf(bvh_reach(M.spheres.lo, M.spheres.hi, o), bvh_reach(M.lo, M.hi, o));
    if (!(bvh_ray_finite(o, d) && eta <= 0x1p-12f && P <= 0x1p40f)) return check_hit_mesh_exact(M.by_index, M.n_triangles, S, ns, np, o, d);

    float best_key = kInfinite;
    int best_idx = 0x7fffffff;
    bool best_just = false;
    if (ns > 0) bvh_walk_spheres(M.spheres, col, o, d, eta, best_key, best_idx, best_just);
    bvh_fold_planes(S, ns, np, o, d, best_key, best_idx, best_just);
    if (M.n_kept > 0) {
        const int first_triangle = ns + np;
        // the bound a child's entry distance is held to: the accumulator's key, or everything while it holds no key (NaN)
        auto bound = [&]() { return best_key == best_key ? best_key : kInfinite; };
        // bvh_walk's loop (ptmi_bvh_device.h), written out: through bvh_walk the compiler lays this one search out otherwise, and that
        // code is not the same speed -- renders up to 18 % faster, closest-hit queries on coherent rays 60 % slower
        // (profiles/one_walk_ab.txt).  A change to the walk is made in both places.
        const auto slab = mesh_slab(o, d);
        auto leaf = [&](int32_t ref) {
            const uint32_t v = (uint32_t)(-1 - ref);
            const int first = (int)(v >> 8), count = (int)(v & 255u);
            for (int k = 0; k < count; ++k) {
                const float4 ga = M.geom[3 * (first + k)], gb = M.geom[3 * (first + k) + 1], gc = M.geom[3 * (first + k) + 2];
                const int i = first_triangle + M.index[first + k];
                PTMI_TRIANGLE_TEST(ga, gb, gc, o, d);
                if (just && (!(best_key <= t) || (t == best_key && i < best_idx))) { best_key = t; best_idx = i; best_just = true; }
            }
        };
        int node = 0, sp = 0;
        while (true) {
            const float4 f0 = M.nodes[4 * node], f1 = M.nodes[4 * node + 1], f2 = M.nodes[4 * node + 2], f3 = M.nodes[4 * node + 3];
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
                if (ra < 0) leaf(ra);
                else next = ra;
            }
            if (hb && tb <= bound()) {
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
    if (best_just && !(best_key < kInfinite)) return check_hit_mesh_exact(M.by_index, M.n_triangles, S, ns, np, o, d);
    HitSel best; best.t = best_key; best.idx = best_idx; best.just = best_just;
    return best;
}

// hit (Intersection.hs:29-32) + normal for a mesh scene's primitive: a triangle's normal is its unit normal at every point, as for a
// plane (Intersection.hs:64); spheres and planes as hit_record
template <typename ScenePtr>
__device__ __forceinline__ void mesh_hit_record(const MeshView &M, ScenePtr S, int ns, int np, int idx, V3 o, V3 d, float t,
                                                V3 &hit_pos, V3 &normal)
{
    if (idx < ns + np) { hit_record(S, ns, idx, o, d, t, hit_pos, normal); return; }
    hit_pos = o + scale_r(d, t);
    const int k = idx - ns - np;
    normal = mk(M.by_index[3 * k].w, M.by_index[3 * k + 1].w, M.by_index[3 * k + 2].w);
}

template <typename ScenePtr>
__device__ __forceinline__ V3 mesh_normal_at(const MeshView &M, ScenePtr S, int ns, int np, int idx, V3 hit_pos)
{
    if (idx < ns + np) return normal_at(S, ns, idx, hit_pos);
    const int k = idx - ns - np;
    return mk(M.by_index[3 * k].w, M.by_index[3 * k + 1].w, M.by_index[3 * k + 2].w);
}

// The hooks of the per-pixel bodies (*_body.inc) for a mesh kernel, whose MeshView argument is named `mesh`
#define PTMI_MESH_HIT(STAGED, S, ns, np, o, d, ...) check_hit_mesh(mesh, S, ns, np, o, d)
#define PTMI_MESH_HIT_RECORD(S, ns, idx, o, d, t, p, n) mesh_hit_record(mesh, S, ns, np, idx, o, d, t, p, n)
#define PTMI_MESH_NORMAL_AT(S, ns, idx, p) mesh_normal_at(mesh, S, ns, np, idx, p)

}  // namespace

}  // namespace ptmi
