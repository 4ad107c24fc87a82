// ptmi_bvh_build.hip -- the leaf order of NEW spheres for a BVH or mesh scene (ptmi_set_bvh_spheres), from ptmi_sphere records in device
// memory.  The kernels, in the order of their launches (validation before, records and boxes behind: ptmi_bvh_refit.hip):
//   bvh_build_keys_kernel    (after the host has read the box of the centres) the Morton key of every centre -- ptmi_mesh_morton.h's
//                            morton_key(c, c, c, lo, hi), the one definition -- and its index;
//   (the radix sort of ptmi_mesh_build.hip, through launch_sort_pairs: no atomics, equal keys keep their index order)
//   bvh_build_order_kernel   order[position] = original index, from the sorted indices.
// Every dependency is a launch boundary in stream order: no workgroup waits for another.
#include "ptmi_device.h"
#include "ptmi_mesh_box.h"
#include "ptmi_mesh_morton.h"

namespace ptmi {

namespace {

constexpr int kSphereWords = 10;                          // a ptmi_sphere

struct CentreBox { float lo[3], hi[3]; };

__global__ void __launch_bounds__(kBlock) bvh_build_keys_kernel(const float *spheres, int n, CentreBox box, uint64_t *keys, uint32_t *indices)
{
    const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const float *s = spheres + (size_t)kSphereWords * i;
    const float c[3] = {s[0], s[1], s[2]};
    keys[i] = morton_key(c, c, c, box.lo, box.hi);
    indices[i] = (uint32_t)i;
}

__global__ void __launch_bounds__(kBlock) bvh_build_order_kernel(const uint32_t *sorted, int n, int32_t *order)
{
    const long long pos = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (pos >= n) return;
    order[pos] = (int32_t)sorted[pos];
}

}  // namespace

hipError_t launch_bvh_build_order(const float *spheres, int n, const float lo[3], const float hi[3], void *scratch, int32_t *order, hipStream_t stream)
{
    if (n <= 0) return hipSuccess;
    CentreBox box;
    for (int a = 0; a < 3; ++a) { box.lo[a] = lo[a]; box.hi[a] = hi[a]; }
    hipError_t e = launch(bvh_build_keys_kernel, dim3(blocks_for(n)), dim3(kBlock), 0, stream, spheres, n, box, sort_keys(scratch, n), sort_indices(scratch, n));
    const uint32_t *sorted = nullptr;
    if (e == hipSuccess) e = launch_sort_pairs(scratch, n, &sorted, stream);
    if (e == hipSuccess) e = launch(bvh_build_order_kernel, dim3(blocks_for(n)), dim3(kBlock), 0, stream, sorted, n, order);
    return e;
}

}  // namespace ptmi
