// ptmi_ray_order.hip -- a coherent order for a caller's batch of rays (ptmi_ray_order_device): order[position] = ray, ascending by
// (key, index), the key ptmi_ray_order.h's -- a function of the rays alone.  The kernels, in the order of their launches:
//   ray_order_box_kernel     the box of the placed rays' origins: per wave six extrema, then integer atomicMin / atomicMax of their
//                            ordered images (ptmi_mesh_box.h) into six words of the workspace -- no float atomics; the words are set to
//                            all ones (lo) and zero (hi) by two memsets in front of it;
//   ray_order_keys_kernel    reads the box back from those words (no host in between) and writes every ray's key and index;
//   (the radix sort of ptmi_mesh_build.hip, through launch_sort_pairs: no atomics, equal keys keep their index order)
//   ray_order_write_kernel   order[position] = original index, from the sorted indices.
// Every dependency is a launch boundary in stream order: no workgroup waits for another, and the host waits for nothing.
// The workspace: the sort's scratch (mesh_build_sort_bytes(n) bytes), then the box words.
#include "ptmi_device.h"
#include "ptmi_ray_order.h"

namespace ptmi {

namespace {

constexpr unsigned int kBoxBlocks = 512;                  // the box kernel's grid: two workgroups per compute unit walk the rays

// `wide`: the launcher found the array 8-byte aligned (wave-uniform)
__device__ __forceinline__ void load_ray_words(const float *rays, long long i, int wide, float r[6])
{
    const float *p = rays + 6 * (size_t)i;
    if (wide) {
        const float2 a = reinterpret_cast<const float2 *>(p)[0], b = reinterpret_cast<const float2 *>(p)[1], c = reinterpret_cast<const float2 *>(p)[2];
        r[0] = a.x; r[1] = a.y; r[2] = b.x; r[3] = b.y; r[4] = c.x; r[5] = c.y;
    } else {
#pragma unroll
        for (int k = 0; k < 6; ++k) r[k] = p[k];
    }
}

__global__ void __launch_bounds__(kBlock) ray_order_box_kernel(const float *rays, int n, int wide, unsigned int *box)
{
    float lo[3], hi[3];
    for (int a = 0; a < 3; ++a) { lo[a] = __builtin_inff(); hi[a] = -__builtin_inff(); }
    for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < n; i += (long long)gridDim.x * kBlock) {
        float r[6];
        load_ray_words(rays, i, wide, r);
        if (ray_placed(r)) {
#pragma unroll
            for (int a = 0; a < 3; ++a) { lo[a] = __builtin_fminf(lo[a], r[a]); hi[a] = __builtin_fmaxf(hi[a], r[a]); }
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            lo[a] = __builtin_fminf(lo[a], __shfl_xor(lo[a], off));
            hi[a] = __builtin_fmaxf(hi[a], __shfl_xor(hi[a], off));
        }
    }
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            if (lo[a] <= hi[a]) {                          // (a wave without a placed ray adds nothing)
                atomicMin(&box[kRayLo + a], ordered_image(lo[a]));
                atomicMax(&box[kRayHi + a], ordered_image(hi[a]));
            }
        }
    }
}

__global__ void __launch_bounds__(kBlock) ray_order_keys_kernel(const float *rays, int n, int wide, const unsigned int *box, uint64_t *keys, uint32_t *indices)
{
    const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    float r[6], lo[3], hi[3];
    load_ray_words(rays, i, wide, r);
#pragma unroll
    for (int a = 0; a < 3; ++a) { lo[a] = ordered_value(box[kRayLo + a]); hi[a] = ordered_value(box[kRayHi + a]); }
    keys[i] = ray_placed(r) ? ray_key(r, lo, hi) : kRayNotPlaced;      // (no placed ray: the box words are as the memsets left them, and unused)
    indices[i] = (uint32_t)i;
}

__global__ void __launch_bounds__(kBlock) ray_order_write_kernel(const uint32_t *sorted, int n, int32_t *order)
{
    const long long pos = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (pos >= n) return;
    order[pos] = (int32_t)sorted[pos];
}

}  // namespace

size_t ray_order_bytes(int n)
{
    if (n <= 0) return 0;
    return (mesh_build_sort_bytes(n) + kRayBoxWords * sizeof(unsigned int) + 7) & ~(size_t)7;
}

hipError_t launch_ray_order(const float *rays, int n, void *work, int32_t *order, hipStream_t stream)
{
    if (n <= 0) return hipSuccess;
    unsigned int *box = reinterpret_cast<unsigned int *>(static_cast<char *>(work) + mesh_build_sort_bytes(n));
    const int wide = (reinterpret_cast<uintptr_t>(rays) & 7u) == 0 ? 1 : 0;
    const unsigned int blocks = blocks_for(n);
    hipError_t e = hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(box + kRayLo), (int)0xffffffffu, kRayHi - kRayLo, stream);
    if (e == hipSuccess) e = hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(box + kRayHi), 0, kRayBoxWords - kRayHi, stream);
    if (e == hipSuccess) e = launch(ray_order_box_kernel, dim3(blocks < kBoxBlocks ? blocks : kBoxBlocks), dim3(kBlock), 0, stream, rays, n, wide, box);
    if (e == hipSuccess) e = launch(ray_order_keys_kernel, dim3(blocks), dim3(kBlock), 0, stream, rays, n, wide, box, sort_keys(work, n), sort_indices(work, n));
    const uint32_t *sorted = nullptr;
    if (e == hipSuccess) e = launch_sort_pairs(work, n, &sorted, stream);
    if (e == hipSuccess) e = launch(ray_order_write_kernel, dim3(blocks), dim3(kBlock), 0, stream, sorted, n, order);
    return e;
}

}  // namespace ptmi
