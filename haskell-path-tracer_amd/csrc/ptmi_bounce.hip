// ptmi_bounce.hip -- one bounce of a caller's paths (ptmi_bounce_rays_device, ptmi_bounce_rays_indexed_device) and the list of the rays that
// are still alive (ptmi_live_rays_device): the two parts of a wavefront path tracer the caller drives.
//
// THE STEP is one prepareRay (Trace.hs:359-383) on (ray_i, radiance_i, throughput_i, seed_i), every word in memory before and after:
//     nearZero throughput_i || isNothing (checkHit scene ray_i)  ->  throughput_i = 0; ray, radiance and seed are not written
//     otherwise computeRay: radiance_i += emittance * throughput_i; throughput_i *= tmod; ray_i = (hit + next ^* epsilon, next); seed_i = seed'
// with the render kernels' own arithmetic -- check_hit / check_hit_bvh / check_hit_mesh, hit_record / mesh_hit_record and shade -- and
// WITHOUT render Inline's shortcut for a shade that is certain to freeze (surely_frozen_after, finish_frozen): the next ray and the
// throughput that shortcut skips are outputs here.  A ray whose throughput is nearZero is not traced.  The optional outputs are
// ptmi_trace_rays_device's words for the INCOMING ray: t, the primitive, the position and normal that were shaded; the miss record (0, -1,
// six zeros) for a ray that missed or was not traced.
//   * one lane per ray, one wave per workgroup, one kernel per scene kind (RayScene, ptmi_ray_lane_device.h, whose frame this lane stands
//     in as the paths' does): a linear scene staged in LDS without and with shared-xy runs, a linear scene too big for LDS through scalar
//     loads, a BVH scene and a mesh scene on check_hit_bvh's LDS stack (their only static LDS: there is nothing to restart from);
//   * the index is lane_ray's wave-uniform null test: lane k < m takes i = index[k] and skips an entry outside [0, n).
// Memory: rays and hit records in three 8-byte pieces when their array is 8-byte aligned, a seed in one 16-byte piece when its array is
// 16-byte aligned, dwords otherwise; throughput and radiance three dwords each.
//
// THE LIVE LIST is a stable compaction in small launches, the shape of the builders' sort (histogram, scan, scatter), with no wait of one
// workgroup on another: [count] every block of kLiveBlock candidates writes each candidate -- or -1 when it is outside [0, n) or its
// throughput is nearZero -- into the workspace and the number of its live ones into counts[block]; [scan] blocks of kLiveBlock counts
// become exclusive prefixes in place, each block's total going one level up (two levels serve PTMI_LIVE_RAYS_MAX = kLiveBlock^3 / 4);
// [scatter] every live candidate goes to (its block's prefix + its rank in the block), every position from the total on gets -1.  The
// candidates are read from the caller's index in the first launch alone and from the workspace afterwards, which is what lets the list be
// written over the index it was made from.
#define PTMI_MESH_EXACT_INLINE __forceinline__
#include "ptmi_ray_lane_device.h"

namespace ptmi {

namespace {

constexpr int kWideSeeds = 4;    // beside kWideRays and kWideHit: the seeds are 16-byte aligned

struct BounceArgs {
    SceneView scene;
    float *rays;                 // [n][6], in/out
    const int32_t *index;        // [m], or null: lane k takes ray k
    int n, m;
    int flags;                   // kWideRays | kWideHit | kWideSeeds
    float *throughput;           // [n][3], in/out
    float *radiance;             // [n][3], in/out
    uint32_t *seed;              // [n][4]: a, b, c, counter; in/out
    float *t;                    // [n], [n], [n][6]: each may be null
    int32_t *idx;
    float *hit;
};

template <RayScene KIND>
__device__ __forceinline__ void bounce_lane(const BounceArgs &a, const MeshView &uniform_mesh)
{
    const int ns = a.scene.n_spheres, np = a.scene.n_planes;
    const float4 *S = stage_scene<KIND>(a.scene);
    const float4 *M = S + a.scene.geom_f4();

    // (the search behind a local name: called where it is made, the hierarchies' walks compile to other code)
    auto hit = [&](V3 o, V3 d) { return closest_hit<KIND, true, SphereFold::kStashSelect, SphereShare::kXY>(uniform_mesh, S, ns, np, a.scene.share_xy, o, d); };

    int ray;
    if (!lane_ray(a.index, a.n, a.m, ray)) return;
    const int i = ray;

    float *tp = a.throughput + 3 * (size_t)i;
    V3 throughput = mk(tp[0], tp[1], tp[2]);
    V3 o = mk(0.0f, 0.0f, 0.0f), d = o, pos = o, normal = o;
    HitSel h; h.t = 0.0f; h.idx = -1; h.just = false;
    if (!near_zero(throughput)) {                              // (a NaN throughput is not nearZero: the ray is traced)
        load_ray(a.rays, i, a.flags & kWideRays, o, d);
        h = hit(o, d);
    }
    if (h.just) {
        record_hit<KIND>(uniform_mesh, S, ns, np, h.idx, o, d, h.t, pos, normal);
        float *rp = a.radiance + 3 * (size_t)i;
        uint32_t *sp = a.seed + 4 * (size_t)i;
        V3 radiance = mk(rp[0], rp[1], rp[2]);
        Sfc32 seed;
        load_seed(sp, a.flags & kWideSeeds, seed);
        shade(M, h.idx, pos, normal, o, d, throughput, radiance, seed);          // computeRay + calcNextRay: o, d become the next ray
        store_hit(a.rays, i, a.flags & kWideRays, o, d);                          // (a ray's six words, laid out as a hit record's)
        rp[0] = radiance.x; rp[1] = radiance.y; rp[2] = radiance.z;
        store_seed(sp, a.flags & kWideSeeds, seed);
    } else {
        throughput = mk(0.0f, 0.0f, 0.0f);
        h.t = 0.0f; h.idx = -1;
    }
    tp[0] = throughput.x; tp[1] = throughput.y; tp[2] = throughput.z;
    if (a.t) a.t[i] = h.t;
    if (a.idx) a.idx[i] = h.idx;
    if (a.hit) store_hit(a.hit, i, a.flags & kWideHit, pos, normal);
}

// One kernel per scene kind, under a name that says which (a BVH scene's view travels in the mesh view's sphere part)
#define PTMI_BOUNCE_KERNEL(NAME, KIND, WAVES)                                                                                        \
    __global__ void __launch_bounds__(kRenderBlock, WAVES) bounce_rays_##NAME##_kernel(const BounceArgs a, const MeshView mesh)      \
    {                                                                                                                                \
        bounce_lane<KIND>(a, mesh);                                                                                                  \
    }
PTMI_BOUNCE_KERNEL(linear_lds, RayScene::kLinearLds, PTMI_INLINE_WAVES)
PTMI_BOUNCE_KERNEL(shared_xy_lds, RayScene::kSharedXyLds, PTMI_INLINE_WAVES)
PTMI_BOUNCE_KERNEL(linear_scalar, RayScene::kLinearScalar, PTMI_INLINE_WAVES)
PTMI_BOUNCE_KERNEL(bvh, RayScene::kBvh, PTMI_BVH_WAVES)
PTMI_BOUNCE_KERNEL(mesh, RayScene::kMesh, PTMI_BVH_WAVES)
#undef PTMI_BOUNCE_KERNEL

// ---- the live list ----
constexpr int kLiveBlock = 256;                                // candidates per block of the count and the scatter, counts per block of the scan
constexpr int kLiveWaves = kLiveBlock / 64;

// The lane's rank among the block's lanes with `flag`, and their number: the waves' ballots, summed over the block's waves in LDS
__device__ __forceinline__ int live_block_rank(bool flag, int &total)
{
    __shared__ int wave_count[kLiveWaves];
    const unsigned long long mask = __ballot(flag);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) wave_count[wave] = __popcll(mask);
    __syncthreads();
    int before = (int)rank_in(mask);
    total = 0;
    for (int w = 0; w < kLiveWaves; ++w) {
        const int c = wave_count[w];
        before += w < wave ? c : 0;
        total += c;
    }
    return before;
}

// cand[k] = candidate k when it is live, else -1; counts[block] = the block's live candidates
__global__ void __launch_bounds__(kLiveBlock) live_rays_count_kernel(const float *throughput, int n, const int32_t *index, int count, int32_t *cand, int32_t *counts)
{
    const int k = blockIdx.x * kLiveBlock + threadIdx.x;
    int i = -1;
    if (k < count) {
        i = index ? index[k] : k;
        if ((unsigned int)i >= (unsigned int)n) {
            i = -1;
        } else {
            const float *tp = throughput + 3 * (size_t)i;
            if (near_zero(mk(tp[0], tp[1], tp[2]))) i = -1;
        }
        cand[k] = i;
    }
    int total;
    (void)live_block_rank(i >= 0, total);
    if (threadIdx.x == 0) counts[blockIdx.x] = total;
}

// counts[block * kLiveBlock ..) -> their exclusive prefixes, in place; sums[block] = their total
__global__ void __launch_bounds__(kLiveBlock) live_rays_scan_kernel(int32_t *counts, int n_counts, int32_t *sums)
{
    __shared__ int lane_sum[2][kLiveBlock];
    const int k = blockIdx.x * kLiveBlock + threadIdx.x;
    const int own = k < n_counts ? counts[k] : 0;
    int from = 0;
    lane_sum[0][threadIdx.x] = own;
    __syncthreads();
    for (int step = 1; step < kLiveBlock; step <<= 1) {      // (Hillis and Steele: eight rounds, two buffers)
        const int v = lane_sum[from][threadIdx.x] + ((int)threadIdx.x >= step ? lane_sum[from][threadIdx.x - step] : 0);
        lane_sum[from ^ 1][threadIdx.x] = v;
        from ^= 1;
        __syncthreads();
    }
    if (k < n_counts) counts[k] = lane_sum[from][threadIdx.x] - own;
    if (threadIdx.x == kLiveBlock - 1) sums[blockIdx.x] = lane_sum[from][threadIdx.x];
}

// live[prefix of the block + rank in the block] = every live candidate; live[total ..count) = -1; *n_live = total.
// upper: the prefixes of the blocks of kLiveBlock counts, or null when one such block held them all.
__global__ void __launch_bounds__(kLiveBlock) live_rays_scatter_kernel(const int32_t *cand, int count, const int32_t *counts, const int32_t *upper, const int32_t *total,
                                                                        int32_t *live, int32_t *n_live)
{
    const int k = blockIdx.x * kLiveBlock + threadIdx.x;
    const int i = k < count ? cand[k] : -1;
    int in_block;
    const int rank = live_block_rank(i >= 0, in_block);
    const int all = *total;
    const int base = counts[blockIdx.x] + (upper ? upper[blockIdx.x / kLiveBlock] : 0);
    if (i >= 0) {
        const int at = base + rank;
        if (at < count) live[at] = i;                           // (always: at <= k)
    }
    if (k < count && k >= all) live[k] = -1;
    if (k == 0 && n_live) *n_live = all;
}

// the workspace: the candidates, then the counts of the three levels (each level's start 4-byte aligned; the whole rounded up to 8 bytes)
struct LiveLayout { size_t cand, counts, sums, top, bytes; int n_counts, n_sums; };
inline LiveLayout live_layout(int count)
{
    LiveLayout l;
    l.n_counts = (int)blocks_for(count, kLiveBlock);
    l.n_sums = (int)blocks_for(l.n_counts, kLiveBlock);
    l.cand = 0;
    l.counts = l.cand + 4 * (size_t)count;
    l.sums = l.counts + 4 * (size_t)l.n_counts;
    l.top = l.sums + 4 * (size_t)l.n_sums;
    l.bytes = (l.top + 4 + 7) & ~(size_t)7;
    return l;
}

}  // namespace

size_t live_rays_bytes(int count) { return count <= 0 ? 0 : live_layout(count).bytes; }

hipError_t launch_live_rays(const float *throughput, int n, const int32_t *index, int count, int32_t *live, int32_t *n_live, void *work, hipStream_t stream)
{
    if (count <= 0) return hipSuccess;
    static_assert((long long)kLiveBlock * kLiveBlock * kLiveBlock >= (1 << 22), "two levels of the scan serve PTMI_LIVE_RAYS_MAX");
    const LiveLayout l = live_layout(count);
    char *w = static_cast<char *>(work);
    int32_t *cand = reinterpret_cast<int32_t *>(w + l.cand), *counts = reinterpret_cast<int32_t *>(w + l.counts);
    int32_t *sums = reinterpret_cast<int32_t *>(w + l.sums), *top = reinterpret_cast<int32_t *>(w + l.top);
    const dim3 block(kLiveBlock);
    hipError_t e = launch(live_rays_count_kernel, dim3(l.n_counts), block, 0, stream, throughput, n, index, count, cand, counts);
    if (e != hipSuccess) return e;
    e = launch(live_rays_scan_kernel, dim3(l.n_sums), block, 0, stream, counts, l.n_counts, sums);
    if (e != hipSuccess) return e;
    const bool two_levels = l.n_sums > 1;                      // (n_sums <= kLiveBlock: one block scans the second level)
    if (two_levels) {
        e = launch(live_rays_scan_kernel, dim3(1), block, 0, stream, sums, l.n_sums, top);
        if (e != hipSuccess) return e;
    }
    return launch(live_rays_scatter_kernel, dim3(l.n_counts), block, 0, stream, (const int32_t *)cand, count, (const int32_t *)counts,
                  two_levels ? (const int32_t *)sums : (const int32_t *)nullptr, two_levels ? (const int32_t *)top : (const int32_t *)sums, live, n_live);
}

hipError_t launch_bounce_rays(SceneView scene, const BvhView *bvh, const MeshView *mesh, float *rays, int n, const int32_t *index, int m, float *throughput,
                              float *radiance, uint32_t *seed, float *t, int32_t *idx, float *hit, hipStream_t stream)
{
    const int lanes = index ? m : n;
    if (n <= 0 || lanes <= 0) return hipSuccess;
    BounceArgs a;
    a.scene = scene; a.rays = rays; a.index = index; a.n = n; a.m = m;
    a.flags = (aligned8(rays) ? kWideRays : 0) | (hit && aligned8(hit) ? kWideHit : 0) | (aligned16(seed) ? kWideSeeds : 0);
    a.throughput = throughput; a.radiance = radiance; a.seed = seed;
    a.t = t; a.idx = idx; a.hit = hit;
    return launch_by_scene(scene, bvh, mesh, bounce_rays_mesh_kernel, bounce_rays_bvh_kernel, bounce_rays_linear_scalar_kernel, bounce_rays_shared_xy_lds_kernel,
                           bounce_rays_linear_lds_kernel, lanes, stream, a);
}

}  // namespace ptmi
