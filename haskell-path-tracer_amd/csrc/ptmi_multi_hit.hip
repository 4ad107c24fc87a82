// ptmi_multi_hit.hip -- the k nearest hits along a caller's device-resident rays (ptmi_trace_rays_multi_device,
// ptmi_trace_rays_multi_indexed_device): for ray i the min(k, |H|) smallest (t, primitive) pairs before t_max[i], ascending, into row i of
// the n x k outputs, the rest of the row the miss record, and the length into count[i].  The specification, the list and the argument
// that the hierarchies' walks prune no listed hit are ptmi_multi_hit_device.h's; the frame -- the scene kinds, the lane's ray, a ray's
// words, the launcher's choice -- is ptmi_ray_lane_device.h's.  One lane per ray or index entry, one wave per workgroup; nothing here
// synchronises, allocates or stages.
//   * one kernel per scene kind and list capacity: a linear scene through scalar loads (the queries' linear form; shared-xy runs are not
//     followed: PTMI_SPHERE_TEST whole gives the same bits), a BVH scene and a mesh scene on check_hit_bvh's LDS stack; capacities 4
//     (k <= 4) and 16.  The list lives in vector registers (ptmi_multi_hit_device.h);
//   * the index is a wave-uniform null test: lane p < m takes i = index[p] and skips an entry outside [0, n).
// Memory: a ray as load_ray loads it; t_max and count one dword each; a row of t and of idx is k consecutive words, stored in 16-byte
// pieces when k % 4 == 0 and both arrays are 16-byte aligned (every row then is), in dwords otherwise.
// The mesh scene's literal fold is not called here; no kernel of this unit has any scratch.
#define PTMI_MESH_EXACT_INLINE __forceinline__
#include "ptmi_multi_hit_device.h"

namespace ptmi {

namespace {

struct MultiHitArgs {
    SceneView scene;
    const float *rays;           // [n][6]
    const float *t_max;          // [n], or null: +inf
    const int32_t *index;        // [m], or null: lane p takes ray p
    int n, m, k;
    int flags;                   // kWideRays | kWideRows
    float *t;                    // [n][k]
    int32_t *idx;                // [n][k]
    int32_t *count;              // [n]
};

template <RayScene KIND, int CAP>
__device__ __forceinline__ void multi_hit_lane(const MultiHitArgs &a, const MeshView &uniform_mesh)
{
    const MeshView mesh = per_lane_view<KIND>(uniform_mesh, std::true_type{});
    int ray;
    if (!lane_ray(a.index, a.n, a.m, ray)) return;
    const int i = ray;
    const int k = is_hierarchy(KIND) ? per_lane(a.k) : a.k;
    multi_hit_ray<KIND, CAP>(a.scene, mesh, a.rays, a.t_max, i, k, a.flags, a.t, a.idx, a.count);
}

#define PTMI_MULTI_HIT_KERNELS(NAME, KIND, WAVES)                                                                                              \
    __global__ void __launch_bounds__(kRenderBlock, WAVES) multi_hit_##NAME##_4_kernel(const MultiHitArgs a, const MeshView mesh)              \
    {                                                                                                                                          \
        multi_hit_lane<KIND, 4>(a, mesh);                                                                                                      \
    }                                                                                                                                          \
    __global__ void __launch_bounds__(kRenderBlock, WAVES) multi_hit_##NAME##_16_kernel(const MultiHitArgs a, const MeshView mesh)             \
    {                                                                                                                                          \
        multi_hit_lane<KIND, 16>(a, mesh);                                                                                                     \
    }
PTMI_MULTI_HIT_KERNELS(linear, RayScene::kLinearScalar, PTMI_BVH_WAVES)
PTMI_MULTI_HIT_KERNELS(bvh, RayScene::kBvh, PTMI_BVH_WAVES)
PTMI_MULTI_HIT_KERNELS(mesh, RayScene::kMesh, PTMI_BVH_WAVES)
#undef PTMI_MULTI_HIT_KERNELS

}  // namespace

hipError_t launch_trace_rays_multi(SceneView scene, const BvhView *bvh, const MeshView *mesh, const float *rays, const float *t_max, int n,
                                   const int32_t *index, int m, int k, float *t, int32_t *idx, int32_t *count, hipStream_t stream)
{
    const int lanes = index ? m : n;
    if (n <= 0 || lanes <= 0 || k < 1 || k > PTMI_MULTI_HIT_MAX) return hipSuccess;
    MultiHitArgs a;
    a.scene = scene; a.rays = rays; a.t_max = t_max; a.index = index; a.n = n; a.m = m; a.k = k;
    a.flags = (aligned8(rays) ? kWideRays : 0) | (k % 4 == 0 && aligned16(t) && aligned16(idx) ? kWideRows : 0);
    a.t = t; a.idx = idx; a.count = count;
    if (k <= 4)
        return launch_by_scene(scene, bvh, mesh, multi_hit_mesh_4_kernel, multi_hit_bvh_4_kernel, nullptr, multi_hit_linear_4_kernel,
                               multi_hit_linear_4_kernel, lanes, stream, a);
    return launch_by_scene(scene, bvh, mesh, multi_hit_mesh_16_kernel, multi_hit_bvh_16_kernel, nullptr, multi_hit_linear_16_kernel,
                           multi_hit_linear_16_kernel, lanes, stream, a);
}

}  // namespace ptmi
