// ptmi_nearest_device.h -- the walks of the NEAREST-PRIMITIVE QUERY behind ptmi_nearest_device: "which primitive is nearest to this point,
// how far is it, and where on it", over a linear scene, a BVH scene and a mesh scene (nearest_point).  Included by ptmi_nearest.hip alone;
// the primitives' distances and the box bound are ptmi_nearest.h's, the traversal loop ptmi_bvh_device.h's bvh_walk, the frame
// ptmi_ray_lane_device.h's.  DESIGN.md 5.9 names the unit; HISTORY.md has the narrative and the measurements.
#pragma once

#include "ptmi_nearest.h"
#include "ptmi_ray_lane_device.h"

namespace ptmi {

namespace {

// THE SPECIFICATION is a minimum, no fold: with lim = r_max (+inf without one), every primitive j -- spheres, then planes, then
// triangles of non-zero area -- has the signed distance s_j of ptmi_nearest.h and the key |s_j|; the answer is the minimum of (key, j),
// lexicographically, over the primitives with key < lim, one f32 compare.  A NaN or +inf key fails the compare, a NaN or non-positive
// lim leaves nothing: the miss record.  ptmi_nearest (ptmi_nearest.cpp) states it by enumeration.
//   * A LINEAR SCENE enumerates every sphere and every plane: nothing is pruned, so nothing needs proving.
//   * NEVER PRUNE THE WINNER.  A point the hierarchies SERVE -- every word finite and bvh_reach of each hierarchy's box <= 2^40 --
//     enumerates all planes first (they seed the bound), then walks the sphere tree and, in a mesh scene, the triangle tree by bvh_walk
//     with bound() = the best key so far, which starts at lim and only ever falls.  A child is entered at lb <= bound(), not <: a
//     primitive that ties the best key with a lower index must still be reached.  lb is nearest_box_bound: the distance from p to the
//     child's box lowered by the margin m = 2^-16 p1 + 2^-60, and ptmi_nearest.h shows that no key under the box is below it.  The
//     winner's key is <= every bound the walk ever held, so every box above the winner is entered whenever it is met.  What IS pruned
//     has lb > bound, so its keys are > the best key and would not replace it.  The leaves return 0: the walk never leaves early; the
//     nearer child (the smaller lb) goes first.
//   * A POINT THE HIERARCHIES DO NOT SERVE enumerates every primitive in the lane -- the spheres from the packed rows, the planes, the
//     triangles by original index (by_index) -- with the same functions: slow and exact.
//   * A TRIANGLE OF ZERO AREA is a record with a NaN stored normal, and every loop over records skips it by that test: the enumeration
//     by original index, and the leaves too -- a triangle that had area when the scene was set and lost it in ptmi_update_mesh_vertices
//     stays in its leaf with a NaN normal (include/ptmi.h), and nearest_triangle, which never reads the stored normal, would answer
//     with its edges.  A point with a NaN word has NaN keys throughout and misses.
//   * THE STACK is check_hit_bvh's column in LDS (bvh_stack_column).
struct NearestBest {
    float key;
    int idx;
};

__device__ __forceinline__ V3 xyz(float4 g) { return mk(g.x, g.y, g.z); }

__device__ __forceinline__ void nearest_take(NearestBest &b, float s, int j, float lim)
{
    const float key = __builtin_fabsf(s);
    if (nearest_better(key, j, lim, b.key, b.idx)) { b.key = key; b.idx = j; }
}

template <typename ScenePtr>
__device__ __forceinline__ void nearest_planes(NearestBest &b, ScenePtr S, int ns, int np, V3 p, float lim)
{
    for (int j = 0; j < np; ++j) nearest_take(b, nearest_plane(xyz(S[ns + 2 * j]), xyz(S[ns + 2 * j + 1]), p).s, ns + j, lim);
}

template <typename ScenePtr>
__device__ __forceinline__ void nearest_spheres_all(NearestBest &b, ScenePtr S, int ns, V3 p, float lim)
{
    for (int i = 0; i < ns; ++i) {
        const float4 g = S[i];
        nearest_take(b, nearest_sphere(xyz(g), g.w, p).s, i, lim);
    }
}

__device__ __forceinline__ void nearest_triangles_all(NearestBest &b, const float4 *by_index, int n_triangles, int first_triangle, V3 p, float lim)
{
    for (int k = 0; k < n_triangles; ++k) {
        const float4 ga = by_index[3 * k], gb = by_index[3 * k + 1], gc = by_index[3 * k + 2];
        if (__builtin_isnan(ga.w)) continue;                 // zero area: no candidate
        nearest_take(b, nearest_triangle(xyz(ga), xyz(gb), xyz(gc), p).s, first_triangle + k, lim);
    }
}

// bvh_walk's box test: always "hit", the entry distance the lowered distance to the box
__device__ __forceinline__ auto nearest_slab(V3 p)
{
    return [=](V3 c, V3 h, float, float &lb) {
        lb = nearest_box_bound(c, h, p, kNearestMargin);
        return true;
    };
}

__device__ __forceinline__ void nearest_spheres(NearestBest &b, const BvhView &B, uint32_t *col, V3 p, float lim)
{
    bvh_walk(B.nodes, col, [&]() { return b.key; }, nearest_slab(p), [&](int first, int count) {
        for (int k = 0; k < count; ++k) {
            const float4 g = B.geom[first + k];
            nearest_take(b, nearest_sphere(xyz(g), g.w, p).s, B.index[first + k], lim);
        }
        return 0;
    });
}

__device__ __forceinline__ void nearest_triangles(NearestBest &b, const MeshView &M, uint32_t *col, int first_triangle, V3 p, float lim)
{
    bvh_walk(M.nodes, col, [&]() { return b.key; }, nearest_slab(p), [&](int first, int count) {
        for (int k = 0; k < count; ++k) {
            const float4 ga = M.geom[3 * (first + k)], gb = M.geom[3 * (first + k) + 1], gc = M.geom[3 * (first + k) + 2];
            if (__builtin_isnan(ga.w)) continue;             // collapsed to zero area by a refit: still in its leaf, no candidate
            nearest_take(b, nearest_triangle(xyz(ga), xyz(gb), xyz(gc), p).s, first_triangle + M.index[first + k], lim);
        }
        return 0;
    });
}

__device__ __forceinline__ bool nearest_point_finite(V3 p) { return __builtin_isfinite(p.x) && __builtin_isfinite(p.y) && __builtin_isfinite(p.z); }

// ---- the three scene kinds: the best (key, idx) of point p under lim > 0 ----
template <RayScene KIND>
__device__ __forceinline__ void nearest_search(NearestBest &b, const SceneView &scene, const MeshView &mesh, V3 p, float lim)
{
    const int ns = scene.n_spheres, np = scene.n_planes;
    const float4 *S = scene.packed;
    if constexpr (!is_hierarchy(KIND)) {
        nearest_spheres_all(b, S, ns, p, lim);
        nearest_planes(b, S, ns, np, p, lim);
    } else {
        uint32_t *col = bvh_stack_column();
        float P = bvh_reach(mesh.spheres.lo, mesh.spheres.hi, p);
        if constexpr (is_mesh(KIND)) P = __builtin_fmaxf(P, bvh_reach(mesh.lo, mesh.hi, p));
        if (nearest_point_finite(p) && P <= 0x1p40f) {
            nearest_planes(b, S, ns, np, p, lim);
            if (ns > 0) nearest_spheres(b, mesh.spheres, col, p, lim);
            if constexpr (is_mesh(KIND)) {
                if (mesh.n_kept > 0) nearest_triangles(b, mesh, col, ns + np, p, lim);
            }
        } else {
            nearest_spheres_all(b, S, ns, p, lim);
            nearest_planes(b, S, ns, np, p, lim);
            if constexpr (is_mesh(KIND)) nearest_triangles_all(b, mesh.by_index, mesh.n_triangles, ns + np, p, lim);
        }
    }
}

// The winner's record: its primitive asked once more, by its original index
template <RayScene KIND>
__device__ __forceinline__ Nearest nearest_record(const SceneView &scene, const MeshView &mesh, int idx, V3 p)
{
    const int ns = scene.n_spheres, np = scene.n_planes;
    const float4 *S = scene.packed;
    if (idx < ns) { const float4 g = S[idx]; return nearest_sphere(xyz(g), g.w, p); }
    if (!is_mesh(KIND) || idx < ns + np) return nearest_plane(xyz(S[ns + 2 * (idx - ns)]), xyz(S[ns + 2 * (idx - ns) + 1]), p);
    const int k = idx - ns - np;
    const float4 ga = mesh.by_index[3 * k], gb = mesh.by_index[3 * k + 1], gc = mesh.by_index[3 * k + 2];
    return nearest_triangle(xyz(ga), xyz(gb), xyz(gc), p);
}

// Point i's answer into position i of the outputs
template <RayScene KIND>
__device__ __forceinline__ void nearest_point(const SceneView &scene, const MeshView &mesh, const float *points, const float *r_max, int i, float *dist_out,
                                              int32_t *idx_out, float *point_out)
{
    const float *pp = points + 3 * (size_t)i;
    const V3 p = mk(pp[0], pp[1], pp[2]);
    const float lim = r_max ? r_max[i] : __builtin_inff();
    NearestBest b;
    b.key = lim; b.idx = 0x7fffffff;
    if (lim > 0.0f) nearest_search<KIND>(b, scene, mesh, p, lim);
    const bool found = b.idx != 0x7fffffff;
    Nearest a;
    a.s = 0.0f; a.at = mk(0.0f, 0.0f, 0.0f);
    if (found) a = nearest_record<KIND>(scene, mesh, b.idx, p);
    dist_out[i] = a.s;
    idx_out[i] = found ? b.idx : -1;
    if (point_out) {
        float *q = point_out + 3 * (size_t)i;
        q[0] = a.at.x; q[1] = a.at.y; q[2] = a.at.z;
    }
}

}  // namespace

}  // namespace ptmi
