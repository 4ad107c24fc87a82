// ptmi_multi_hit_device.h -- the MULTI-HIT walks behind ptmi_trace_rays_multi_device: "the k nearest hits along the ray, in order, before
// t_max", over a linear scene, a BVH scene and a mesh scene (multi_hit_ray).  Included by ptmi_multi_hit.hip alone; it sits behind the
// any-hit walks (ptmi_query_device.h), whose primitive tests, box tests and admission rule it uses.  DESIGN.md 5.9 summarises what follows.
#pragma once

#include "ptmi_ray_lane_device.h"

namespace ptmi {

namespace {

// THE SPECIFICATION is a sorted set, no fold: with lim = t_max (+inf without one), H = { (t_j, j) : primitive j's own test is a Just and
// t_j < lim }, one f32 compare -- PTMI_SPHERE_TEST and sqrt_rn, PTMI_PLANE_DISTANCE behind fold_planes' candidate test,
// PTMI_TRIANGLE_TEST: the operations check_hit makes, from the same text, one hit per primitive.  A NaN t fails the compare and so does
// +inf: every element is finite and >= 0, and a NaN or non-positive lim leaves H empty.  The row is the min(k, |H|) smallest elements of
// H ascending by (t, j), then the miss record (0, -1).
//   * THE LIST is CAP (t, idx) pairs in vector registers, ascending.  Every access is by a compile-time slot (a runtime-indexed array in
//     registers would go to scratch): an insertion overwrites the last slot and sinks it by CAP - 1 unrolled compare-and-swaps.  A
//     runtime k <= CAP has the first CAP - k slots filled with (-inf, -1), below which nothing sinks, so the list proper is the last k
//     slots, the bound is always the last slot's t, and the row written is the last k slots.  A slot not yet taken holds (lim, -1):
//     the bound is lim until k hits are held and the k-th key from then on -- it tightens at the caller's k, not at the capacity.
//   * A LINEAR SCENE enumerates every sphere and every plane: nothing is pruned, so nothing needs proving.
//   * NEVER PRUNE A LISTED HIT.  A ray the hierarchies SERVE -- check_hit_bvh's and occluded_mesh's admission test: finite, eta <= 2^-12,
//     reach <= 2^40 -- enumerates all planes, then walks the sphere tree and, in a mesh scene, the triangle tree by bvh_walk with
//     bound() = the last slot's t.  A child is entered at t_near <= bound(), not <: a primitive that ties the k-th entry with a lower
//     index must still be reached.  The box margins (bvh_sphere_slab, mesh_slab) guarantee that a primitive accepted at key t lies under
//     children with t_near <= t.  The bound only ever falls: an insertion replaces the last slot by something no larger.  Every element
//     of the final list has t <= the final k-th key <= every earlier bound, and while fewer than k are held the bound is lim > t.  So
//     every box above a listed hit is entered whenever it is met: no listed hit is pruned.  What IS pruned has t_near > bound, so its
//     primitives have t > the k-th key and would not be inserted.  The leaves return 0: the walk never leaves early.
//   * A RAY THE HIERARCHIES DO NOT SERVE enumerates every primitive in the lane -- the spheres from the packed rows, the planes, the
//     triangles by original index (by_index; a triangle of zero area has a NaN normal, hence a NaN t, and is never listed) -- with the
//     same tests: slow and exact, the counterpart of falling to check_hit.
//   * THE STACK is check_hit_bvh's column in LDS (bvh_stack_column).
template <int CAP>
struct HitList {
    float t[CAP];
    int idx[CAP];
};

template <int CAP>
__device__ __forceinline__ void hit_list_init(HitList<CAP> &L, int k, float lim)
{
#pragma unroll
    for (int s = 0; s < CAP; ++s) {
        const bool below = s < CAP - k;                      // a slot the caller's k does not use
        L.t[s] = below ? -__builtin_inff() : lim;
        L.idx[s] = -1;
    }
}

// (t, j) of a Just into the list, if it qualifies and is below the last slot
template <int CAP>
__device__ __forceinline__ void hit_list_insert(HitList<CAP> &L, bool just, float t, int j, float lim)
{
    const float lt = L.t[CAP - 1];
    // (the lexicographic compares as mask arithmetic, not short circuits: a branch per compare keeps an exec mask per slot alive)
    if (just & (t < lim) & ((t < lt) | ((t == lt) & (j < L.idx[CAP - 1])))) {
        L.t[CAP - 1] = t;
        L.idx[CAP - 1] = j;
#pragma unroll
        for (int s = CAP - 1; s > 0; --s) {
            const float a = L.t[s - 1], b = L.t[s];
            const int ia = L.idx[s - 1], ib = L.idx[s];
            const bool sink = (b < a) | ((b == a) & (ib < ia));
            L.t[s - 1] = sink ? b : a; L.idx[s - 1] = sink ? ib : ia;
            L.t[s] = sink ? a : b;     L.idx[s] = sink ? ia : ib;
        }
    }
}

// Every plane, enumerated (any_hit_planes' loop: fold_planes' candidates only divide)
template <int CAP, typename ScenePtr>
__device__ __forceinline__ void multi_hit_planes(HitList<CAP> &L, ScenePtr S, int ns, int np, V3 o, V3 d, float lim)
{
    for (int j = 0; j < np; ++j) {
        const float4 gp = S[ns + 2 * j], gn = S[ns + 2 * j + 1];
        const float denom = PTMI_PLANE_DENOM(gn, d);
        if (!(denom > 1e-6f)) {
            PTMI_PLANE_DISTANCE(gp, gn, o, denom);           // t, just
            hit_list_insert(L, just, t, ns + j, lim);
        }
    }
}

// Every sphere of the packed rows, in index order
template <int CAP, typename ScenePtr>
__device__ __forceinline__ void multi_hit_spheres_all(HitList<CAP> &L, ScenePtr S, int ns, V3 o, V3 d, float lim)
{
    for (int i = 0; i < ns; ++i) {
        float t;
        const bool just = bvh_sphere_just(S[i], o, d, t);    // PTMI_SPHERE_TEST, sqrt_rn, !(t < 0)
        hit_list_insert(L, just, t, i, lim);
    }
}

// Every triangle by original index
template <int CAP>
__device__ __forceinline__ void multi_hit_triangles_all(HitList<CAP> &L, const float4 *by_index, int n_triangles, int first_triangle, V3 o, V3 d, float lim)
{
    for (int k = 0; k < n_triangles; ++k) {
        const float4 ga = by_index[3 * k], gb = by_index[3 * k + 1], gc = by_index[3 * k + 2];
        PTMI_TRIANGLE_TEST(ga, gb, gc, o, d);                // t, just
        hit_list_insert(L, just, t, first_triangle + k, lim);
    }
}

// The hierarchies walked with the bound at the list's last slot; a leaf inserts and never ends the walk
template <int CAP>
__device__ __forceinline__ void multi_hit_spheres(HitList<CAP> &L, const BvhView &B, uint32_t *col, V3 o, V3 d, float eta, float lim)
{
    bvh_walk(B.nodes, col, [&]() { return L.t[CAP - 1]; }, bvh_sphere_slab(o, d, eta), [&](int first, int count) {
        for (int k = 0; k < count; ++k) {
            float t;
            const bool just = bvh_sphere_just(B.geom[first + k], o, d, t);
            hit_list_insert(L, just, t, B.index[first + k], lim);
        }
        return 0;
    });
}

template <int CAP>
__device__ __forceinline__ void multi_hit_triangles(HitList<CAP> &L, const MeshView &M, uint32_t *col, int first_triangle, V3 o, V3 d, float lim)
{
    bvh_walk(M.nodes, col, [&]() { return L.t[CAP - 1]; }, mesh_slab(o, d), [&](int first, int count) {
        for (int k = 0; k < count; ++k) {
            const float4 ga = M.geom[3 * (first + k)], gb = M.geom[3 * (first + k) + 1], gc = M.geom[3 * (first + k) + 2];
            PTMI_TRIANGLE_TEST(ga, gb, gc, o, d);            // t, just
            hit_list_insert(L, just, t, first_triangle + M.index[first + k], lim);
        }
        return 0;
    });
}

// ---- the three scene kinds: the list of ray (o, d) under lim > 0 ----
template <RayScene KIND, int CAP>
__device__ __forceinline__ void multi_hit_search(HitList<CAP> &L, const SceneView &scene, const MeshView &mesh, V3 o, V3 d, float lim)
{
    const int ns = scene.n_spheres, np = scene.n_planes;
    const float4 *S = scene.packed;
    if constexpr (!is_hierarchy(KIND)) {
        multi_hit_spheres_all(L, S, ns, o, d, lim);
        multi_hit_planes(L, S, ns, np, o, d, lim);
    } else {
        uint32_t *col = bvh_stack_column();
        const float eta = bvh_eta(d);
        float P = bvh_reach(mesh.spheres.lo, mesh.spheres.hi, o);
        if constexpr (is_mesh(KIND)) P = __builtin_fmaxf(P, bvh_reach(mesh.lo, mesh.hi, o));
        if (bvh_ray_finite(o, d) && eta <= 0x1p-12f && P <= 0x1p40f) {
            multi_hit_planes(L, S, ns, np, o, d, lim);
            if (ns > 0) multi_hit_spheres(L, mesh.spheres, col, o, d, eta, lim);
            if constexpr (is_mesh(KIND)) {
                if (mesh.n_kept > 0) multi_hit_triangles(L, mesh, col, ns + np, o, d, lim);
            }
        } else {
            multi_hit_spheres_all(L, S, ns, o, d, lim);
            multi_hit_planes(L, S, ns, np, o, d, lim);
            if constexpr (is_mesh(KIND)) multi_hit_triangles_all(L, mesh.by_index, mesh.n_triangles, ns + np, o, d, lim);
        }
    }
}

// flags beside kWideRays: the rows of t and idx are 16-byte pieces (k % 4 == 0 and both arrays 16-byte aligned: the launcher found them so)
constexpr int kWideRows = 4;

// Ray i's list into row i of t_out and idx_out and its length into count_out[i]
template <RayScene KIND, int CAP>
__device__ __forceinline__ void multi_hit_ray(const SceneView &scene, const MeshView &mesh, const float *rays, const float *t_max, int i, int k, int flags,
                                              float *t_out, int32_t *idx_out, int32_t *count_out)
{
    V3 o, d;
    load_ray(rays, i, flags & kWideRays, o, d);
    const float lim = t_max ? t_max[i] : __builtin_inff();
    HitList<CAP> L;
    hit_list_init(L, k, lim);
    if (lim > 0.0f) multi_hit_search<KIND>(L, scene, mesh, o, d, lim);

    // the row: the last k slots; a slot never taken is the miss record
    int count = 0;
#pragma unroll
    for (int s = 0; s < CAP; ++s) {
        const bool taken = L.idx[s] >= 0;
        count += taken ? 1 : 0;
        L.t[s] = taken ? L.t[s] : 0.0f;
    }
    float *tr = t_out + (size_t)i * (size_t)k;
    int32_t *ir = idx_out + (size_t)i * (size_t)k;
    const int skip = CAP - k;                                // the row's column 0 is slot `skip`
    if (flags & kWideRows) {
#pragma unroll
        for (int g = 0; g < CAP / 4; ++g) {
            if (4 * g >= skip) {
                reinterpret_cast<float4 *>(tr + (4 * g - skip))[0] = float4{L.t[4 * g], L.t[4 * g + 1], L.t[4 * g + 2], L.t[4 * g + 3]};
                reinterpret_cast<int4 *>(ir + (4 * g - skip))[0] = int4{L.idx[4 * g], L.idx[4 * g + 1], L.idx[4 * g + 2], L.idx[4 * g + 3]};
            }
        }
    } else {
#pragma unroll
        for (int s = 0; s < CAP; ++s) {
            if (s >= skip) { tr[s - skip] = L.t[s]; ir[s - skip] = L.idx[s]; }
        }
    }
    count_out[i] = count;
}

}  // namespace

}  // namespace ptmi
