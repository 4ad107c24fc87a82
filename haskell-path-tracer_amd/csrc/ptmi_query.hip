// ptmi_query.hip -- the ray queries of the C ABI on device-resident rays (ptmi_trace_rays_device, ptmi_occluded_device): closest hit with
// its hit record, and occlusion before t_max, against the context's scene of any kind.  One lane per ray, one wave per workgroup, as the
// point queries of ptmi_small.hip; nothing here synchronises, allocates or stages.
//   * closest hit: the render kernels' own search, unchanged -- check_hit (a linear scene; its shared-xy walk for a scene with runs, as
//     launch_eval_check_hit chooses), check_hit_bvh, check_hit_mesh -- then hit_record / mesh_hit_record for the lanes that hit;
//   * occlusion: the any-hit walks of ptmi_query_device.h.
// Memory: a ray is six words, 24 bytes apart: three 8-byte loads when the array is 8-byte aligned (every ray then is), six dword loads
// otherwise; the hit record likewise as three 8-byte stores or six dword stores; t, idx and occluded are coalesced dword stores.
// The mesh scene's literal fold is inlined here (ptmi_mesh_device.h): these kernels are held to four waves per SIMD by the LDS stack and have
// the registers for it, and without its frame no kernel of this unit has any scratch.
#define PTMI_MESH_EXACT_INLINE __forceinline__
#include "ptmi_query_device.h"

namespace ptmi {

namespace {

enum class QueryScene { kLinear, kLinearShared, kBvh, kMesh };

// `wide`: the launcher found the array 8-byte aligned (wave-uniform)
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

// flags: bit 0 the rays are 8-byte aligned, bit 1 the hit records are
constexpr int kWideRays = 1, kWideHit = 2;

template <QueryScene KIND>
__device__ __forceinline__ void trace_rays(const SceneView &scene, const MeshView &mesh, const float *rays, int n, int flags, float *t_out, int32_t *idx_out,
                                           float *hit_out)
{
    const int i = blockIdx.x * kRenderBlock + threadIdx.x;
    if (i >= n) return;
    V3 o, d;
    load_ray(rays, i, flags & kWideRays, o, d);
    const int ns = scene.n_spheres, np = scene.n_planes;
    HitSel h;
    if constexpr (KIND == QueryScene::kLinear) h = check_hit(scene.packed, ns, np, o, d);
    else if constexpr (KIND == QueryScene::kLinearShared) h = check_hit<false, SphereFold::kStash, SphereShare::kXY>(scene.packed, ns, np, o, d, nullptr, scene.share_xy);
    else if constexpr (KIND == QueryScene::kBvh) h = check_hit_bvh(mesh.spheres, scene.packed, ns, np, o, d);
    else h = check_hit_mesh(mesh, scene.packed, ns, np, o, d);
    t_out[i] = h.just ? h.t : 0.0f;
    idx_out[i] = h.just ? h.idx : -1;
    if (hit_out) {
        V3 pos = mk(0.0f, 0.0f, 0.0f), nrm = mk(0.0f, 0.0f, 0.0f);
        if (h.just) {
            if constexpr (KIND == QueryScene::kMesh) mesh_hit_record(mesh, scene.packed, ns, np, h.idx, o, d, h.t, pos, nrm);
            else hit_record(scene.packed, ns, h.idx, o, d, h.t, pos, nrm);
        }
        store_hit(hit_out, i, flags & kWideHit, pos, nrm);
    }
}

// reach: a linear scene's SceneState.sphere_reach (ptmi_query_device.h: occluded_linear)
template <QueryScene KIND>
__device__ __forceinline__ void occluded(const SceneView &scene, const MeshView &mesh, float reach, const float *rays, const float *t_max, int n, int flags,
                                         int32_t *occluded_out)
{
    const int i = blockIdx.x * kRenderBlock + threadIdx.x;
    if (i >= n) return;
    V3 o, d;
    load_ray(rays, i, flags & kWideRays, o, d);
    const float limit = t_max[i];
    const int ns = scene.n_spheres, np = scene.n_planes;
    bool occ;
    if constexpr (KIND == QueryScene::kLinear) occ = occluded_linear<SphereShare::kNone>(scene.packed, ns, np, 0ull, reach, o, d, limit);
    else if constexpr (KIND == QueryScene::kLinearShared) occ = occluded_linear<SphereShare::kXY>(scene.packed, ns, np, scene.share_xy, reach, o, d, limit);
    else if constexpr (KIND == QueryScene::kBvh) occ = occluded_bvh(mesh.spheres, scene.packed, ns, np, o, d, limit);
    else occ = occluded_mesh(mesh, scene.packed, ns, np, o, d, limit);
    occluded_out[i] = occ ? 1 : 0;
}

// One kernel of each query per scene kind, under a name that says which (a BVH scene's view travels in the mesh view's sphere part)
#define PTMI_QUERY_KERNELS(NAME, KIND)                                                                                                             \
    __global__ void __launch_bounds__(kRenderBlock) trace_rays_##NAME##_kernel(const SceneView scene, const MeshView mesh, const float *rays, int n, \
                                                                               int flags, float *t_out, int32_t *idx_out, float *hit_out)          \
    {                                                                                                                                              \
        trace_rays<KIND>(scene, mesh, rays, n, flags, t_out, idx_out, hit_out);                                                                    \
    }                                                                                                                                              \
    __global__ void __launch_bounds__(kRenderBlock) occluded_##NAME##_kernel(const SceneView scene, const MeshView mesh, float reach,              \
                                                                             const float *rays, const float *t_max, int n, int flags,              \
                                                                             int32_t *occluded_out)                                                \
    {                                                                                                                                              \
        occluded<KIND>(scene, mesh, reach, rays, t_max, n, flags, occluded_out);                                                                   \
    }
PTMI_QUERY_KERNELS(linear, QueryScene::kLinear)
PTMI_QUERY_KERNELS(shared_xy, QueryScene::kLinearShared)
PTMI_QUERY_KERNELS(bvh, QueryScene::kBvh)
PTMI_QUERY_KERNELS(mesh, QueryScene::kMesh)
#undef PTMI_QUERY_KERNELS

inline bool aligned8(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 7u) == 0; }

// The scene kind as launch_eval_check_hit chooses it: go(the mesh kernel, the BVH one, the shared-xy one, the linear one)
template <typename Kernel, typename F>
hipError_t dispatch(const SceneView &scene, const BvhView *bvh, const MeshView *mesh, Kernel of_mesh, Kernel of_bvh, Kernel of_shared, Kernel of_linear, F &&go)
{
    if (mesh) return go(of_mesh, *mesh);
    MeshView view{};
    if (bvh) { view.spheres = *bvh; return go(of_bvh, view); }
    return go(scene.share_xy ? of_shared : of_linear, view);
}

}  // namespace

hipError_t launch_trace_rays(SceneView scene, const BvhView *bvh, const MeshView *mesh, const float *rays, int n, float *t, int32_t *idx, float *hit,
                             hipStream_t stream)
{
    if (n <= 0) return hipSuccess;
    const int flags = (aligned8(rays) ? kWideRays : 0) | (hit && aligned8(hit) ? kWideHit : 0);
    return dispatch(scene, bvh, mesh, trace_rays_mesh_kernel, trace_rays_bvh_kernel, trace_rays_shared_xy_kernel, trace_rays_linear_kernel,
                    [&](auto kernel, const MeshView &view) {
        return launch(kernel, dim3(blocks_for(n, kRenderBlock)), dim3(kRenderBlock), 0, stream, scene, view, rays, n, flags, t, idx, hit);
    });
}

hipError_t launch_occluded(SceneView scene, const BvhView *bvh, const MeshView *mesh, float reach, const float *rays, const float *t_max, int n,
                           int32_t *occluded, hipStream_t stream)
{
    if (n <= 0) return hipSuccess;
    const int flags = aligned8(rays) ? kWideRays : 0;
    return dispatch(scene, bvh, mesh, occluded_mesh_kernel, occluded_bvh_kernel, occluded_shared_xy_kernel, occluded_linear_kernel,
                    [&](auto kernel, const MeshView &view) {
        return launch(kernel, dim3(blocks_for(n, kRenderBlock)), dim3(kRenderBlock), 0, stream, scene, view, reach, rays, t_max, n, flags, occluded);
    });
}

}  // namespace ptmi
