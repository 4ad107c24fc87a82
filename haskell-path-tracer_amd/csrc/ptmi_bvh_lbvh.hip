// ptmi_bvh_lbvh.hip -- the SPATIAL build of a sphere hierarchy on the device (ptmi_set_bvh_spheres under PTMI_OPT_BVH_DEVICE_BUILD =
// PTMI_BVH_BUILD_SPATIAL): the leaf order and the topology of ptmi_bvh_spatial.h, from ptmi_sphere records in device memory.  The
// kernels, in the order of their launches (validation before, records and boxes behind: ptmi_bvh_refit.hip):
//   bvh_spatial_keys_kernel     the key of every centre in cubic cells -- spatial_key, the one definition -- and its index;
//   (the radix sort of ptmi_mesh_build.hip, through launch_sort_pairs: no atomics, equal keys keep their index order)
//   per level, the root's first, two launches:
//   bvh_spatial_split_kernel    one lane per node of the level: where its range splits (spatial_split: the highest differing bit of its end
//                               keys, a binary search over the sorted keys, the depth guard), and per workgroup how many of its nodes'
//                               children are inner nodes;
//   bvh_spatial_number_kernel   the ids of those children -- the next level's nodes in id order: the sum of the workgroups before, a scan
//                               within the workgroup (wave shuffles, then the four wave totals), so the numbering is a function of the keys
//                               and of nothing else -- both references of every node, the children's ranges, the next level's count;
//   then, once the host has read the levels' counts and allocated the hierarchy,
//   bvh_spatial_finish_kernel   the references into the nodes (their boxes are bvh_level_kernel's) and the list of nodes by level, the
//                               deepest first, that the refit's launches walk.
// Every dependency is a launch boundary in stream order: no workgroup waits for another, and no value depends on the order of atomics
// (there are none).  A level is launched over the most nodes it can hold (spatial_level_bound); the kernels read its count on the device.
#include "ptmi_device.h"
#include "ptmi_bvh_spatial.h"

namespace ptmi {

namespace {

constexpr int kSphereWords = 10;                          // a ptmi_sphere
constexpr int kWaves = kBlock / 64;

struct CentreBox { float lo[3], hi[3]; };

__global__ void __launch_bounds__(kBlock) bvh_spatial_keys_kernel(const float *spheres, int n, CentreBox box, uint64_t *keys, uint32_t *indices)
{
    const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const float *s = spheres + (size_t)kSphereWords * i;
    const float c[3] = {s[0], s[1], s[2]};
    keys[i] = spatial_key(c, box.lo, spatial_den(box.lo, box.hi));
    indices[i] = (uint32_t)i;
}

// the sum of v over the workgroup, in every lane (sums: kWaves words of LDS; a barrier before they are reused)
__device__ __forceinline__ unsigned int block_sum(unsigned int v, unsigned int *sums)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += (unsigned int)__shfl_xor((int)v, off);
    if ((threadIdx.x & 63) == 0) sums[threadIdx.x >> 6] = v;
    __syncthreads();
    unsigned int total = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) total += sums[w];
    return total;
}

// where a level's nodes start and how many there are: the counts of the levels above, written by their launches (the root's own by its)
__device__ __forceinline__ void level_span(const int *count, int level, int &first, int &cnt)
{
    first = 0;
    for (int l = 0; l < level; ++l) first += count[l];
    cnt = level == 0 ? 1 : count[level];
}

__device__ __forceinline__ int inner_children(int b, int m, int e) { return (m - b > PTMI_BVH_LEAF_MAX ? 1 : 0) + (e - m > PTMI_BVH_LEAF_MAX ? 1 : 0); }

__global__ void __launch_bounds__(kBlock) bvh_spatial_split_kernel(const uint64_t *keys, int n, int level, const int *count, const int2 *range, int cap,
                                                                   int *split, unsigned int *inner_sums, unsigned int *fallback_sums)
{
    __shared__ unsigned int sums[2][kWaves];
    int first, cnt;
    level_span(count, level, first, cnt);
    if ((long long)blockIdx.x * kBlock >= cnt) return;     // (the whole workgroup: the launch covers the most the level can hold)
    const int k = blockIdx.x * kBlock + threadIdx.x;
    unsigned int inner = 0, fell = 0;
    if (k < cnt && first + k < cap) {
        int b = 0, e = n;
        if (level > 0) { const int2 r = range[first + k]; b = r.x; e = r.y; }
        int m = e;                                         // (a root of at most a leaf's spheres: everything in child 0)
        if (e - b > PTMI_BVH_LEAF_MAX && b >= 0 && e <= n) {
            int fb = 0;
            m = spatial_split(keys, b, e, level, &fb);
            fell = (unsigned int)fb;
        }
        split[k] = m;
        inner = (unsigned int)inner_children(b, m, e);
    }
    const unsigned int inner_total = block_sum(inner, sums[0]), fell_total = block_sum(fell, sums[1]);
    if (threadIdx.x == 0) { inner_sums[blockIdx.x] = inner_total; fallback_sums[blockIdx.x] = fell_total; }
}

__global__ void __launch_bounds__(kBlock) bvh_spatial_number_kernel(int n, int level, int *count, int2 *range, int cap, const int *split,
                                                                    const unsigned int *inner_sums, const unsigned int *fallback_sums, int2 *ref)
{
    __shared__ unsigned int sums[3][kWaves];
    int first, cnt;
    level_span(count, level, first, cnt);
    if ((long long)blockIdx.x * kBlock >= cnt) return;
    const int blocks = (cnt + kBlock - 1) / kBlock;
    const bool last = (int)blockIdx.x == blocks - 1;
    // the inner children of the workgroups before this one; the last workgroup also adds up the level's equal-count splits
    unsigned int before = 0, fell = 0;
    for (int j = threadIdx.x; j < (int)blockIdx.x; j += kBlock) before += inner_sums[j];
    if (last)
        for (int j = threadIdx.x; j < blocks; j += kBlock) fell += fallback_sums[j];
    before = block_sum(before, sums[0]);
    fell = block_sum(fell, sums[1]);
    const int k = blockIdx.x * kBlock + threadIdx.x;
    const bool live = k < cnt && first + k < cap;
    int b = 0, m = 0, e = 0;
    if (live) {
        e = n;
        if (level > 0) { const int2 r = range[first + k]; b = r.x; e = r.y; }
        m = split[k];
    }
    const unsigned int c0 = live && m - b > PTMI_BVH_LEAF_MAX ? 1u : 0u, c1 = live && e - m > PTMI_BVH_LEAF_MAX ? 1u : 0u, mine = c0 + c1;
    // the scan: within the wave by shuffles, then the totals of the waves before
    unsigned int incl = mine;
    const unsigned int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const unsigned int below = (unsigned int)__shfl_up((int)incl, off);
        if (lane >= (unsigned int)off) incl += below;
    }
    if (lane == 63) sums[2][wave] = incl;
    __syncthreads();
    unsigned int waves_before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) {
        waves_before += (unsigned int)w < wave ? sums[2][w] : 0u;
        total += sums[2][w];
    }
    if (live) {
        const long long child = (long long)first + cnt + before + waves_before + (incl - mine);     // the id of this node's first inner child
        int2 r;
        r.x = c0 ? (int)child : spatial_leaf_ref(b, m);
        r.y = c1 ? (int)(child + c0) : spatial_leaf_ref(m, e);
        if (c0 && child < cap) range[child] = int2{b, m};
        if (c1 && child + c0 < cap) range[child + c0] = int2{m, e};
        ref[first + k] = r;
    }
    if (last && threadIdx.x == 0) {
        if (level == 0) count[0] = 1;                     // (the root: what the levels below add up from)
        if (level + 1 < PTMI_BVH_MAX_DEPTH) count[level + 1] = (int)(before + total);
        count[kSpatialFallbacks] += (int)fell;            // (one writer per launch, the launches in stream order)
    }
}

struct SpatialLevels { int first[PTMI_BVH_MAX_DEPTH + 1]; int listed_at[PTMI_BVH_MAX_DEPTH]; int levels; };

__global__ void __launch_bounds__(kBlock) bvh_spatial_finish_kernel(const int2 *ref, int n_nodes, SpatialLevels lv, float4 *nodes, int32_t *level_nodes)
{
    const int id = blockIdx.x * kBlock + threadIdx.x;
    if (id >= n_nodes) return;
    const int2 r = ref[id];
    nodes[4 * (size_t)id + 3] = float4{u2f((uint32_t)r.x), u2f((uint32_t)r.y), 0.0f, 0.0f};
    int level = 0;
    while (level + 1 < lv.levels && id >= lv.first[level + 1]) ++level;
    level_nodes[lv.listed_at[level] + (id - lv.first[level])] = id;
}

}  // namespace

// The scratch of a build over n spheres: the ranges and references of the most nodes a tree can have, one split per node of the widest
// level, two sums per workgroup of that level, the words the host reads.
namespace {
struct SpatialWork { int2 *range, *ref; int *split; unsigned int *inner_sums, *fallback_sums; int *count; int cap, widest; };
SpatialWork carve(void *work, int n)
{
    SpatialWork w;
    w.cap = spatial_node_bound(n);
    w.widest = spatial_level_bound(n, PTMI_BVH_MAX_DEPTH);
    const size_t blocks = blocks_for(w.widest);
    w.range = static_cast<int2 *>(work);
    w.ref = w.range + w.cap;
    w.split = reinterpret_cast<int *>(w.ref + w.cap);
    w.inner_sums = reinterpret_cast<unsigned int *>(w.split + w.widest);
    w.fallback_sums = w.inner_sums + blocks;
    w.count = reinterpret_cast<int *>(w.fallback_sums + blocks);
    return w;
}
}  // namespace

size_t bvh_spatial_work_bytes(int n)
{
    const size_t cap = (size_t)spatial_node_bound(n), widest = (size_t)spatial_level_bound(n, PTMI_BVH_MAX_DEPTH);
    return 2 * cap * sizeof(int2) + widest * sizeof(int) + 2 * blocks_for((long long)widest) * sizeof(unsigned int) + kSpatialWords * sizeof(int);
}

const int *bvh_spatial_report(void *work, int n) { return carve(work, n).count; }

hipError_t launch_bvh_spatial_tree(const float *spheres, int n, const float lo[3], const float hi[3], void *scratch, void *work, const uint32_t **sorted,
                                   hipStream_t stream)
{
    const SpatialWork w = carve(work, n);
    hipError_t e = hipMemsetAsync(w.count, 0, kSpatialWords * sizeof(int), stream);
    const uint64_t *keys = nullptr;
    *sorted = nullptr;
    if (e == hipSuccess && n > 0) {
        CentreBox box;
        for (int a = 0; a < 3; ++a) { box.lo[a] = lo[a]; box.hi[a] = hi[a]; }
        e = launch(bvh_spatial_keys_kernel, dim3(blocks_for(n)), dim3(kBlock), 0, stream, spheres, n, box, sort_keys(scratch, n), sort_indices(scratch, n));
        if (e == hipSuccess) e = launch_sort_pairs(scratch, n, sorted, stream);
        // the sorted keys lie in the half of the key pairs in which the sorted indices lie
        if (e == hipSuccess) keys = sort_keys(scratch, n) + (*sorted - sort_indices(scratch, n));
    }
    const int levels = spatial_level_limit(n);
    for (int level = 0; level < levels && e == hipSuccess; ++level) {
        const dim3 grid(blocks_for(spatial_level_bound(n, level)));
        e = launch(bvh_spatial_split_kernel, grid, dim3(kBlock), 0, stream, keys, n, level, (const int *)w.count, (const int2 *)w.range, w.cap, w.split,
                   w.inner_sums, w.fallback_sums);
        if (e == hipSuccess)
            e = launch(bvh_spatial_number_kernel, grid, dim3(kBlock), 0, stream, n, level, w.count, w.range, w.cap, (const int *)w.split,
                       (const unsigned int *)w.inner_sums, (const unsigned int *)w.fallback_sums, w.ref);
    }
    return e;
}

hipError_t launch_bvh_spatial_finish(void *work, int n, const int *level_count, int levels, float4 *nodes, int32_t *level_nodes, hipStream_t stream)
{
    const SpatialWork w = carve(work, n);
    SpatialLevels lv{};
    lv.levels = levels;
    for (int l = 0; l < levels; ++l) lv.first[l + 1] = lv.first[l] + level_count[l];
    for (int l = levels - 1, at = 0; l >= 0; at += level_count[l], --l) lv.listed_at[l] = at;      // the deepest level first
    const int n_nodes = lv.first[levels];
    if (n_nodes <= 0 || n_nodes > w.cap) return hipErrorInvalidValue;
    return launch(bvh_spatial_finish_kernel, dim3(blocks_for(n_nodes)), dim3(kBlock), 0, stream, (const int2 *)w.ref, n_nodes, lv, nodes, level_nodes);
}

}  // namespace ptmi
