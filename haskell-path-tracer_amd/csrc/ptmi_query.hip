// ptmi_query.hip -- the ray queries of the C ABI on device-resident rays (ptmi_trace_rays_device, ptmi_occluded_device): closest hit with
// its hit record, and occlusion before t_max, against the context's scene of any kind.  One lane per ray, one wave per workgroup, as the
// point queries of ptmi_small.hip; nothing here synchronises, allocates or stages.
//   * closest hit: the render kernels' own search, unchanged -- check_hit (a linear scene; its shared-xy walk for a scene with runs, as
//     launch_eval_check_hit chooses), check_hit_bvh, check_hit_mesh -- then hit_record / mesh_hit_record for the lanes that hit;
//   * occlusion: the any-hit walks of ptmi_query_device.h.
// What a lane does with its ray is trace_ray / occluded_ray of ptmi_ray_lane_device.h, shared with the indexed queries (ptmi_query_indexed.hip).
// Memory: a ray is six words, 24 bytes apart: three 8-byte loads when the array is 8-byte aligned (every ray then is), six dword loads
// otherwise; the hit record likewise as three 8-byte stores or six dword stores; t, idx and occluded are coalesced dword stores.
// The mesh scene's literal fold is inlined here (ptmi_mesh_device.h): these kernels are held to four waves per SIMD by the LDS stack and have
// the registers for it, and without its frame no kernel of this unit has any scratch.
#define PTMI_MESH_EXACT_INLINE __forceinline__
#include "ptmi_ray_lane_device.h"

namespace ptmi {

namespace {

// One kernel of each query per scene kind, under a name that says which (a BVH scene's view travels in the mesh view's sphere part)
#define PTMI_QUERY_KERNELS(NAME, KIND, SHARE)                                                                                                          \
    __global__ void __launch_bounds__(kRenderBlock) trace_rays_##NAME##_kernel(const SceneView scene, const MeshView mesh, const float *rays, int n, \
                                                                               int flags, float *t_out, int32_t *idx_out, float *hit_out)          \
    {                                                                                                                                              \
        const int i = blockIdx.x * kRenderBlock + threadIdx.x;                                                                                     \
        if (i < n) trace_ray<KIND, SHARE>(scene, mesh, rays, i, flags, t_out, idx_out, hit_out);                                                   \
    }                                                                                                                                              \
    __global__ void __launch_bounds__(kRenderBlock) occluded_##NAME##_kernel(const SceneView scene, const MeshView mesh, float reach,              \
                                                                             const float *rays, const float *t_max, int n, int flags,              \
                                                                             int32_t *occluded_out)                                                \
    {                                                                                                                                              \
        const int i = blockIdx.x * kRenderBlock + threadIdx.x;                                                                                     \
        if (i < n) occluded_ray<KIND, SHARE>(scene, mesh, reach, rays, t_max, i, flags, occluded_out);                                             \
    }
PTMI_QUERY_KERNELS(linear, RayScene::kLinearScalar, SphereShare::kNone)
PTMI_QUERY_KERNELS(shared_xy, RayScene::kLinearScalar, SphereShare::kXY)
PTMI_QUERY_KERNELS(bvh, RayScene::kBvh, SphereShare::kNone)
PTMI_QUERY_KERNELS(mesh, RayScene::kMesh, SphereShare::kNone)
#undef PTMI_QUERY_KERNELS

}  // namespace

hipError_t launch_trace_rays(SceneView scene, const BvhView *bvh, const MeshView *mesh, const float *rays, int n, float *t, int32_t *idx, float *hit,
                             hipStream_t stream)
{
    if (n <= 0) return hipSuccess;
    const int flags = (aligned8(rays) ? kWideRays : 0) | (hit && aligned8(hit) ? kWideHit : 0);
    return launch_by_scene(scene, bvh, mesh, trace_rays_mesh_kernel, trace_rays_bvh_kernel, nullptr, trace_rays_shared_xy_kernel, trace_rays_linear_kernel, n,
                           stream, scene, rays, n, flags, t, idx, hit);
}

hipError_t launch_occluded(SceneView scene, const BvhView *bvh, const MeshView *mesh, float reach, const float *rays, const float *t_max, int n,
                           int32_t *occluded, hipStream_t stream)
{
    if (n <= 0) return hipSuccess;
    const int flags = aligned8(rays) ? kWideRays : 0;
    return launch_by_scene(scene, bvh, mesh, occluded_mesh_kernel, occluded_bvh_kernel, nullptr, occluded_shared_xy_kernel, occluded_linear_kernel, n, stream,
                           scene, reach, rays, t_max, n, flags, occluded);
}

}  // namespace ptmi
