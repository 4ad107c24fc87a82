// ptmi_nearest.hip -- the nearest-primitive query over a caller's device-resident points (ptmi_nearest_device,
// ptmi_nearest_indexed_device): for point i the primitive with the least (|signed distance|, index) within r_max[i], its signed distance
// into dist[i], its index into idx[i] and the nearest location on it into point[i].  The specification and the argument that the
// hierarchies' walks never prune the winner are ptmi_nearest_device.h's, the arithmetic ptmi_nearest.h's; the frame -- the scene kinds,
// which point a lane takes, the launcher's choice -- is ptmi_ray_lane_device.h's.  One lane per point or index entry, one wave per
// workgroup; nothing here synchronises, allocates or stages.
//   * one kernel per scene kind: a linear scene through scalar loads (the queries' linear form), a BVH scene and a mesh scene on
//     check_hit_bvh's LDS stack;
//   * the index is a wave-uniform null test: lane k < m takes i = index[k] and skips an entry outside [0, n).
// Memory: a point is three dwords, r_max, dist and idx one each, the location three: 4-byte alignment suffices for every array.
// No kernel of this unit has any scratch.
#include "ptmi_nearest_device.h"

namespace ptmi {

namespace {

struct NearestArgs {
    SceneView scene;
    const float *points;         // [n][3]
    const float *r_max;          // [n], or null: +inf
    const int32_t *index;        // [m], or null: lane k takes point k
    int n, m;
    float *dist;                 // [n]
    int32_t *idx;                // [n]
    float *point;                // [n][3], or null
};

template <RayScene KIND>
__device__ __forceinline__ void nearest_lane(const NearestArgs &a, const MeshView &uniform_mesh)
{
    const MeshView mesh = per_lane_view<KIND>(uniform_mesh, std::true_type{});
    int point;
    if (!lane_ray(a.index, a.n, a.m, point)) return;
    const int i = point;
    nearest_point<KIND>(a.scene, mesh, a.points, a.r_max, i, a.dist, a.idx, a.point);
}

#define PTMI_NEAREST_KERNEL(NAME, KIND)                                                                                                        \
    __global__ void __launch_bounds__(kRenderBlock, PTMI_BVH_WAVES) nearest_##NAME##_kernel(const NearestArgs a, const MeshView mesh)          \
    {                                                                                                                                          \
        nearest_lane<KIND>(a, mesh);                                                                                                           \
    }
PTMI_NEAREST_KERNEL(linear, RayScene::kLinearScalar)
PTMI_NEAREST_KERNEL(bvh, RayScene::kBvh)
PTMI_NEAREST_KERNEL(mesh, RayScene::kMesh)
#undef PTMI_NEAREST_KERNEL

}  // namespace

hipError_t launch_nearest(SceneView scene, const BvhView *bvh, const MeshView *mesh, const float *points, const float *r_max, int n, const int32_t *index, int m,
                          float *dist, int32_t *idx, float *point, hipStream_t stream)
{
    const int lanes = index ? m : n;
    if (n <= 0 || lanes <= 0) return hipSuccess;
    NearestArgs a;
    a.scene = scene; a.points = points; a.r_max = r_max; a.index = index; a.n = n; a.m = m;
    a.dist = dist; a.idx = idx; a.point = point;
    return launch_by_scene(scene, bvh, mesh, nearest_mesh_kernel, nearest_bvh_kernel, nullptr, nearest_linear_kernel, nearest_linear_kernel, lanes, stream, a);
}

}  // namespace ptmi
