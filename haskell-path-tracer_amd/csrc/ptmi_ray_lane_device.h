// ptmi_ray_lane_device.h -- what a lane of a caller-ray kernel does before and after its own loop, once for every such kernel: the ray
// queries (ptmi_query.hip, ptmi_query_indexed.hip), the paths (ptmi_paths.hip), the stepped paths (ptmi_bounce.hip) and the ray streams
// (ptmi_trace_streams.hip).  The scene kinds a family has a kernel for, the scene's staging in LDS, the wave-uniform words a hierarchy's
// kernel holds per lane, the closest hit and its record by scene kind, which ray a lane takes, a ray's, a hit record's and a seed's words
// in memory, and the launcher's choice of kernel.  A unit keeps its args struct, its lane body and its kernels' names; the any-hit walks
// and their specification are ptmi_query_device.h's.  DESIGN.md 5.9 has the rule for adding a caller-ray kernel.
#pragma once

#include <type_traits>

#include "ptmi_query_device.h"

#ifndef PTMI_INLINE_WAVES
#define PTMI_INLINE_WAVES 7      // render Inline's occupancy budget (ptmi_inline.hip)
#endif

namespace ptmi {

namespace {

// ---- the scene kinds: one kernel of a family per kind it serves ----
// A linear scene staged in LDS, without and with shared-xy runs (as launch_linear chooses), a linear scene read through scalar loads (the
// queries' only linear form; the other families' for a scene too big for LDS), a BVH scene and a mesh scene on check_hit_bvh's LDS stack.
enum class RayScene { kLinearLds, kSharedXyLds, kLinearScalar, kBvh, kMesh };
constexpr bool staged_in_lds(RayScene k) { return k == RayScene::kLinearLds || k == RayScene::kSharedXyLds; }
constexpr bool is_hierarchy(RayScene k) { return k == RayScene::kBvh || k == RayScene::kMesh; }
constexpr bool is_mesh(RayScene k) { return k == RayScene::kMesh; }

// The scene as the lane reads it: the workgroup's copy in LDS (the kernel's dynamic LDS; copied here, behind a barrier) or the packed rows
template <RayScene KIND>
__device__ __forceinline__ const float4 *stage_scene(const SceneView &scene)
{
    extern __shared__ float4 lds_scene[];
    if (staged_in_lds(KIND)) {
        const int total = scene.total_f4();
        for (int i = threadIdx.x; i < total; i += kRenderBlock) lds_scene[i] = scene.packed[i];
        __syncthreads();
    }
    return staged_in_lds(KIND) ? lds_scene : scene.packed;
}

// ---- wave-uniform words held per lane ----
// The hierarchies' kernels are short of scalar registers, not of vector ones: the boxes of the admission tests, twelve wave-uniform words
// that only ever meet a lane's own origin, are held per lane there, so that no scalar register spills into lanes -- and so are whichever
// of its counts and limits a kernel names.
__device__ __forceinline__ float per_lane(float uniform) { float v; asm volatile("v_mov_b32 %0, %1" : "=v"(v) : "s"(uniform)); return v; }
__device__ __forceinline__ int per_lane(int uniform) { int v; asm volatile("v_mov_b32 %0, %1" : "=v"(v) : "s"(uniform)); return v; }
__device__ __forceinline__ const int *per_lane_ptr(const int *uniform)
{
    const uintptr_t u = reinterpret_cast<uintptr_t>(uniform);
    uint32_t lo, hi;
    asm volatile("v_mov_b32 %0, %1" : "=v"(lo) : "s"((uint32_t)u));
    asm volatile("v_mov_b32 %0, %1" : "=v"(hi) : "s"((uint32_t)(u >> 32)));
    return reinterpret_cast<const int *>((uintptr_t)lo | ((uintptr_t)hi << 32));
}

// The view a lane walks with: the kernel's own for a linear scene; a hierarchy's with its boxes per lane and, `with_index`, the leaves'
// index arrays too, which only ever meet a lane's own leaf
template <RayScene KIND, bool WITH_INDEX>
__device__ __forceinline__ MeshView per_lane_view(const MeshView &uniform_mesh, std::bool_constant<WITH_INDEX>)
{
    MeshView mesh = uniform_mesh;
    if constexpr (is_hierarchy(KIND)) {
        for (int w = 0; w < 3; ++w) {
            mesh.spheres.lo[w] = per_lane(uniform_mesh.spheres.lo[w]); mesh.spheres.hi[w] = per_lane(uniform_mesh.spheres.hi[w]);
            if constexpr (is_mesh(KIND)) { mesh.lo[w] = per_lane(uniform_mesh.lo[w]); mesh.hi[w] = per_lane(uniform_mesh.hi[w]); }
        }
        if constexpr (WITH_INDEX) {
            mesh.spheres.index = per_lane_ptr(uniform_mesh.spheres.index);
            if constexpr (is_mesh(KIND)) mesh.index = per_lane_ptr(uniform_mesh.index);
        }
    }
    return mesh;
}

// ---- the closest hit and its record, by scene kind ----
// The render kernels' own search.  A linear scene's walk is the family's to name: STAGED_WALK (of a scene staged in LDS), FOLD and SHARE
// are check_hit's parameters; kLinearLds is the kernel of a scene without shared-xy runs and walks without them whatever SHARE says.
// A BVH scene's view travels in the mesh view's sphere part.
// How a lane calls it decides the code of the hierarchies' walks (a level of inlining more or less moves a register copy in bvh_walk's
// push): the paths' and the streams' lanes call it where they trace, the queries' and the stepped paths' behind a local lambda -- as each
// had its search before it came here.  tools/kernel_resources.py's assembly() shows what a change of either does.
template <RayScene KIND, bool STAGED_WALK, SphereFold FOLD, SphereShare SHARE>
__device__ __forceinline__ HitSel closest_hit(const MeshView &mesh, const float4 *S, int ns, int np, unsigned long long share_xy, V3 o, V3 d)
{
    if constexpr (KIND == RayScene::kLinearLds) return check_hit<STAGED_WALK, FOLD>(S, ns, np, o, d);
    else if constexpr (KIND == RayScene::kSharedXyLds) return check_hit<STAGED_WALK, FOLD, SHARE>(S, ns, np, o, d, nullptr, share_xy);
    else if constexpr (KIND == RayScene::kLinearScalar) return check_hit<false, FOLD, SHARE>(S, ns, np, o, d, nullptr, share_xy);
    else if constexpr (KIND == RayScene::kBvh) return check_hit_bvh(mesh.spheres, S, ns, np, o, d);
    else return check_hit_mesh(mesh, S, ns, np, o, d);
}

template <RayScene KIND>
__device__ __forceinline__ void record_hit(const MeshView &mesh, const float4 *S, int ns, int np, int idx, V3 o, V3 d, float t, V3 &p, V3 &n)
{
    if constexpr (is_mesh(KIND)) mesh_hit_record(mesh, S, ns, np, idx, o, d, t, p, n);
    else hit_record(S, ns, idx, o, d, t, p, n);
}

// ---- which ray a lane takes ----
// Lane k takes ray k of n, or -- the index is a wave-uniform null test -- entry k of m: i = index[k], skipped when it lies outside [0, n).
// False: the lane has no ray.  The callers take `i` into a variable of their own and copy it (int ray; ...; const int i = ray;): a ray
// number whose address was taken compiles its uses' address arithmetic to other code.  (The indexed queries, whose index is never null,
// keep their own indexed_ray.)
__device__ __forceinline__ bool lane_ray(const int32_t *index, int n, int m, int &i)
{
    const int k = blockIdx.x * kRenderBlock + threadIdx.x;
    int j = k;
    bool valid = k < n;
    if (index) {
        valid = k < m;
        if (valid) { j = index[k]; valid = (unsigned int)j < (unsigned int)n; }
    }
    i = j;
    return valid;
}

// ---- a ray's, a hit record's and a seed's words in memory ----
// flags: bit 0 the rays are 8-byte aligned, bit 1 the hit records are (the launcher found them so: wave-uniform)
constexpr int kWideRays = 1, kWideHit = 2;
inline bool aligned8(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 7u) == 0; }
inline bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

__device__ __forceinline__ void load_ray(const float *rays, int i, bool wide, V3 &o, V3 &d)
{
    const float *p = rays + 6 * (size_t)i;
    if (wide) {
        const float2 a = reinterpret_cast<const float2 *>(p)[0], b = reinterpret_cast<const float2 *>(p)[1], c = reinterpret_cast<const float2 *>(p)[2];
        o = mk(a.x, a.y, b.x);
        d = mk(b.y, c.x, c.y);
    } else {
        o = mk(p[0], p[1], p[2]);
        d = mk(p[3], p[4], p[5]);
    }
}

__device__ __forceinline__ void store_hit(float *hit, int i, bool wide, V3 pos, V3 nrm)
{
    float *q = hit + 6 * (size_t)i;
    if (wide) {
        reinterpret_cast<float2 *>(q)[0] = float2{pos.x, pos.y};
        reinterpret_cast<float2 *>(q)[1] = float2{pos.z, nrm.x};
        reinterpret_cast<float2 *>(q)[2] = float2{nrm.y, nrm.z};
    } else {
        q[0] = pos.x; q[1] = pos.y; q[2] = pos.z; q[3] = nrm.x; q[4] = nrm.y; q[5] = nrm.z;
    }
}

// A seed -- a, b, c, counter -- in one 16-byte piece when `wide`, four dwords otherwise.  `wide` is a launcher's flag (aligned16 of the
// array) or the lane's own test of its seed's address, seed_is_wide: every lane answers alike, and no flag lives in a scalar register
// from the load to the store.
__device__ __forceinline__ bool seed_is_wide(const uint32_t *sp) { return (reinterpret_cast<uintptr_t>(sp) & 15u) == 0; }

__device__ __forceinline__ void load_seed(const uint32_t *sp, bool wide, Sfc32 &seed)
{
    if (wide) {
        const uint4 w = *reinterpret_cast<const uint4 *>(sp);
        seed.a = w.x; seed.b = w.y; seed.c = w.z; seed.counter = w.w;
    } else {
        seed.a = sp[0]; seed.b = sp[1]; seed.c = sp[2]; seed.counter = sp[3];
    }
}

__device__ __forceinline__ void store_seed(uint32_t *sp, bool wide, const Sfc32 &seed)
{
    if (wide) {
        *reinterpret_cast<uint4 *>(sp) = uint4{seed.a, seed.b, seed.c, seed.counter};
    } else {
        sp[0] = seed.a; sp[1] = seed.b; sp[2] = seed.c; sp[3] = seed.counter;
    }
}

// ---- one ray of a query: what a lane of ptmi_query.hip and of ptmi_query_indexed.hip does once it knows its ray ----
// (KIND: kLinearScalar, kBvh or kMesh; SHARE: whether a linear scene's walk follows its shared-xy runs, as launch_eval_check_hit chooses)
// Ray i's closest hit into position i of the outputs
template <RayScene KIND, SphereShare SHARE>
__device__ __forceinline__ void trace_ray(const SceneView &scene, const MeshView &mesh, const float *rays, int i, int flags, float *t_out, int32_t *idx_out,
                                          float *hit_out)
{
    V3 o, d;
    load_ray(rays, i, flags & kWideRays, o, d);
    const int ns = scene.n_spheres, np = scene.n_planes;
    // (the search behind a local name: called where it is made, the hierarchies' walks compile to other code)
    auto hit = [&](V3 o, V3 d) { return closest_hit<KIND, false, SphereFold::kStash, SHARE>(mesh, scene.packed, ns, np, scene.share_xy, o, d); };
    const HitSel h = hit(o, d);
    t_out[i] = h.just ? h.t : 0.0f;
    idx_out[i] = h.just ? h.idx : -1;
    if (hit_out) {
        V3 pos = mk(0.0f, 0.0f, 0.0f), nrm = mk(0.0f, 0.0f, 0.0f);
        if (h.just) record_hit<KIND>(mesh, scene.packed, ns, np, h.idx, o, d, h.t, pos, nrm);
        store_hit(hit_out, i, flags & kWideHit, pos, nrm);
    }
}

// Ray i's occlusion before t_max[i] into position i.  reach: a linear scene's SceneState.sphere_reach (occluded_linear)
template <RayScene KIND, SphereShare SHARE>
__device__ __forceinline__ void occluded_ray(const SceneView &scene, const MeshView &mesh, float reach, const float *rays, const float *t_max, int i, int flags,
                                             int32_t *occluded_out)
{
    V3 o, d;
    load_ray(rays, i, flags & kWideRays, o, d);
    const float limit = t_max[i];
    const int ns = scene.n_spheres, np = scene.n_planes;
    bool occ;
    if constexpr (is_mesh(KIND)) occ = occluded_mesh(mesh, scene.packed, ns, np, o, d, limit);
    else if constexpr (is_hierarchy(KIND)) occ = occluded_bvh(mesh.spheres, scene.packed, ns, np, o, d, limit);
    else occ = occluded_linear<SHARE>(scene.packed, ns, np, scene.share_xy, reach, o, d, limit);
    occluded_out[i] = occ ? 1 : 0;
}

// ---- the launch: one lane per ray or index entry, one wave per workgroup, the kernel of the scene's kind ----
// The kernels take (first, the view they walk, rest...).  Mesh, else BVH through a view that holds it, else a linear scene: a family with
// a scalar kernel stages the scene in LDS (the kernel's dynamic LDS) unless it is so big that staging it per wave would cost more
// occupancy than scalar loads cost speed (scene_fits_lds); a family without one (of_scalar null: the queries) stages nothing.
template <typename Kernel, typename ScalarKernel, typename First, typename... Rest>
hipError_t launch_by_scene(const SceneView &scene, const BvhView *bvh, const MeshView *mesh, Kernel of_mesh, Kernel of_bvh, ScalarKernel of_scalar, Kernel of_shared,
                           Kernel of_linear, int lanes, hipStream_t stream, const First &first, const Rest &...rest)
{
    const dim3 grid(blocks_for(lanes, kRenderBlock)), block(kRenderBlock);
    if (mesh) return launch(of_mesh, grid, block, 0, stream, first, *mesh, rest...);
    MeshView view{};
    if (bvh) { view.spheres = *bvh; return launch(of_bvh, grid, block, 0, stream, first, view, rest...); }
    size_t lds = 0;
    if constexpr (!std::is_null_pointer_v<ScalarKernel>) {
        lds = (size_t)scene.total_f4() * sizeof(float4);
        if (lds > kMaxSceneLds) return launch(of_scalar, grid, block, 0, stream, first, view, rest...);
    }
    return launch(scene.share_xy ? of_shared : of_linear, grid, block, lds, stream, first, view, rest...);
}

}  // namespace

}  // namespace ptmi
