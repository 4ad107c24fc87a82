// ptmi_query_indexed.hip -- the ray queries through an index (ptmi_trace_rays_indexed_device, ptmi_occluded_indexed_device): lane k of m
// takes i = index[k] and, when 0 <= i < n, answers ray i into position i of the n-sized outputs -- by trace_ray / occluded_ray of
// ptmi_ray_lane_device.h, the very functions a lane of ptmi_query.hip runs, so the words are the plain queries' whatever the index holds.  An
// entry outside [0, n) reads and writes nothing; a position no entry names is left as it was.  One lane per entry, one wave per
// workgroup; nothing here synchronises, allocates or stages.
// With the order of ptmi_ray_order_device as the index, the 64 rays of a wave are neighbours in origin and direction and walk a hierarchy
// together; with a caller's list of live rays (m < n) only those are traced, and their answers land where the rays live.
// Memory: the index is a coalesced dword load.  A ray is a 24-byte gather: three 8-byte loads when the array is 8-byte aligned, six dword
// loads otherwise -- a ray lies in one or two 64-byte lines, and under a coherent order the lanes' neighbours in space are seldom
// neighbours in memory, so a wave's gather touches up to a line or two per lane.  t, idx and occluded are scattered dword stores, the hit
// record three 8-byte or six dword stores.  Measured: through the identity the hierarchies' kernels take the plain
// kernels' time; the scatter shows on a linear scene, whose search is short.
// The mesh scene's literal fold is inlined as in ptmi_query.hip: no kernel of this unit has any scratch.
#define PTMI_MESH_EXACT_INLINE __forceinline__
#include "ptmi_ray_lane_device.h"

namespace ptmi {

namespace {

// The ray of entry k, or -1 for an entry that is skipped: lane_ray (ptmi_ray_lane_device.h) for an index that is never null, in the shape
// these kernels were compiled from -- behind lane_ray's null test, or its bool, all eight compile to other code
__device__ __forceinline__ int indexed_ray(const int32_t *index, int m, int n)
{
    const int k = blockIdx.x * kRenderBlock + threadIdx.x;
    if (k >= m) return -1;
    const int i = index[k];
    return (unsigned int)i < (unsigned int)n ? i : -1;
}

#define PTMI_INDEXED_KERNELS(NAME, KIND, SHARE)                                                                                                         \
    __global__ void __launch_bounds__(kRenderBlock) trace_rays_indexed_##NAME##_kernel(const SceneView scene, const MeshView mesh, const float *rays, \
                                                                                       int n, const int32_t *index, int m, int flags, float *t_out, \
                                                                                       int32_t *idx_out, float *hit_out)                            \
    {                                                                                                                                               \
        const int i = indexed_ray(index, m, n);                                                                                                     \
        if (i >= 0) trace_ray<KIND, SHARE>(scene, mesh, rays, i, flags, t_out, idx_out, hit_out);                                                   \
    }                                                                                                                                               \
    __global__ void __launch_bounds__(kRenderBlock) occluded_indexed_##NAME##_kernel(const SceneView scene, const MeshView mesh, float reach,       \
                                                                                     const float *rays, const float *t_max, int n,                  \
                                                                                     const int32_t *index, int m, int flags, int32_t *occluded_out) \
    {                                                                                                                                               \
        const int i = indexed_ray(index, m, n);                                                                                                     \
        if (i >= 0) occluded_ray<KIND, SHARE>(scene, mesh, reach, rays, t_max, i, flags, occluded_out);                                             \
    }
PTMI_INDEXED_KERNELS(linear, RayScene::kLinearScalar, SphereShare::kNone)
PTMI_INDEXED_KERNELS(shared_xy, RayScene::kLinearScalar, SphereShare::kXY)
PTMI_INDEXED_KERNELS(bvh, RayScene::kBvh, SphereShare::kNone)
PTMI_INDEXED_KERNELS(mesh, RayScene::kMesh, SphereShare::kNone)
#undef PTMI_INDEXED_KERNELS

}  // namespace

hipError_t launch_trace_rays_indexed(SceneView scene, const BvhView *bvh, const MeshView *mesh, const float *rays, int n, const int32_t *index, int m,
                                     float *t, int32_t *idx, float *hit, hipStream_t stream)
{
    if (n <= 0 || m <= 0) return hipSuccess;
    const int flags = (aligned8(rays) ? kWideRays : 0) | (hit && aligned8(hit) ? kWideHit : 0);
    return launch_by_scene(scene, bvh, mesh, trace_rays_indexed_mesh_kernel, trace_rays_indexed_bvh_kernel, nullptr, trace_rays_indexed_shared_xy_kernel,
                           trace_rays_indexed_linear_kernel, m, stream, scene, rays, n, index, m, flags, t, idx, hit);
}

hipError_t launch_occluded_indexed(SceneView scene, const BvhView *bvh, const MeshView *mesh, float reach, const float *rays, const float *t_max, int n,
                                   const int32_t *index, int m, int32_t *occluded, hipStream_t stream)
{
    if (n <= 0 || m <= 0) return hipSuccess;
    const int flags = aligned8(rays) ? kWideRays : 0;
    return launch_by_scene(scene, bvh, mesh, occluded_indexed_mesh_kernel, occluded_indexed_bvh_kernel, nullptr, occluded_indexed_shared_xy_kernel,
                           occluded_indexed_linear_kernel, m, stream, scene, reach, rays, t_max, n, index, m, flags, occluded);
}

}  // namespace ptmi
