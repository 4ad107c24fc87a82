// ptmi_bounce.cpp -- the stepped paths' calls of include/ptmi.h: ptmi_bounce_rays_device / ptmi_bounce_rays_indexed_device (argument checks
// and the launch of ptmi_bounce.hip's step), ptmi_live_rays_device (checks and the compaction's launches) and its host twin
// ptmi_live_rays, which takes host memory, uses no device and is the definition the device list is tested against.
#include "ptmi_ctx.h"

using namespace ptmi;

// One bounce: the refusals of ptmi_trace_paths_device (nothing enqueued, nothing written), then one launch on the context's stream.  The
// context's state planes, partition, camera and statistics are not touched.
static int bounce_rays(ptmi_ctx *c, float *d_rays, int n, const int32_t *d_index, int m, bool indexed, float *d_throughput, float *d_radiance, uint32_t *d_seed,
                       float *d_t, int32_t *d_idx, float *d_hit)
{
    if (!c) return PTMI_EINVAL;
    std::lock_guard<std::mutex> lock(c->mu);
    if (n < 0 || (n > 0 && (!d_rays || !d_throughput || !d_radiance || !d_seed)) || (indexed && (m < 0 || (m > 0 && !d_index))))
        return fail(c, PTMI_EINVAL, "bad ray-bounce arguments");
    if (!c->scene.packed.p) return fail(c, PTMI_ESTATE, "ptmi_set_scene has not been called");
    if (c->scene.has_glass) return fail(c, PTMI_EINVAL, "the scene holds a GLASS material: render Inline cannot split rays, use PTMI_STREAMS");
    if (n == 0 || (indexed && m == 0)) return PTMI_OK;
    PTMI_HIP(c, hipSetDevice(c->device));
    const RayCallScene r = ray_call_scene(c);
    PTMI_HIP(c, launch_bounce_rays(r.scene, r.bvh, r.mesh, d_rays, n, indexed ? d_index : nullptr, m, d_throughput, d_radiance, d_seed, d_t, d_idx, d_hit,
                                   c->stream));
    return PTMI_OK;
}

extern "C" int ptmi_bounce_rays_device(ptmi_ctx *c, float *d_rays, int n, float *d_throughput, float *d_radiance, uint32_t *d_seed, float *d_t, int32_t *d_idx,
                                       float *d_hit)
{
    return bounce_rays(c, d_rays, n, nullptr, 0, false, d_throughput, d_radiance, d_seed, d_t, d_idx, d_hit);
}

extern "C" int ptmi_bounce_rays_indexed_device(ptmi_ctx *c, float *d_rays, int n, const int32_t *d_index, int m, float *d_throughput, float *d_radiance,
                                               uint32_t *d_seed, float *d_t, int32_t *d_idx, float *d_hit)
{
    return bounce_rays(c, d_rays, n, d_index, m, true, d_throughput, d_radiance, d_seed, d_t, d_idx, d_hit);
}

extern "C" size_t ptmi_live_rays_bytes(int count) { return live_rays_bytes(count); }

// The definition: the candidates in order, those inside [0, n) whose throughput is not nearZero first, -1 behind them.  (A list written
// over its index is safe in one pass: the write position never passes the read position.)
extern "C" int ptmi_live_rays(const float *throughput, int n, const int32_t *index, int m, int32_t *live, int32_t *count)
{
    if (n < 0 || m < 0) return PTMI_EINVAL;
    const int candidates = index ? m : n;
    if (candidates > PTMI_LIVE_RAYS_MAX) return PTMI_ELIMIT;
    if (candidates == 0) return PTMI_OK;
    if (!live || (n > 0 && !throughput)) return PTMI_EINVAL;
    int found = 0;
    for (int k = 0; k < candidates; ++k) {
        const int32_t i = index ? index[k] : k;
        if ((uint32_t)i >= (uint32_t)n) continue;
        const float *t = throughput + 3 * (size_t)i;
        V3 v; v.x = t[0]; v.y = t[1]; v.z = t[2];
        if (!near_zero(v)) live[found++] = i;
    }
    for (int k = found; k < candidates; ++k) live[k] = -1;
    if (count) *count = found;
    return PTMI_OK;
}

// Refusals first (nothing enqueued, nothing written), then the launches on the context's stream -- no synchronisation, no allocation, no
// copy to the host.  No scene is needed: the list is a function of the throughputs and the index.
extern "C" int ptmi_live_rays_device(ptmi_ctx *c, const float *d_throughput, int n, const int32_t *d_index, int m, int32_t *d_live, int32_t *d_count, void *d_work,
                                     size_t work_bytes)
{
    if (!c) return PTMI_EINVAL;
    std::lock_guard<std::mutex> lock(c->mu);
    if (n < 0 || m < 0) return fail(c, PTMI_EINVAL, "bad live-rays arguments");
    const int candidates = d_index ? m : n;
    if (candidates > PTMI_LIVE_RAYS_MAX) return fail(c, PTMI_ELIMIT, "more candidates than PTMI_LIVE_RAYS_MAX");
    if (candidates == 0) return PTMI_OK;
    if (!d_live || !d_work || (n > 0 && !d_throughput)) return fail(c, PTMI_EINVAL, "bad live-rays arguments");
    if ((reinterpret_cast<uintptr_t>(d_work) & 7u) != 0) return fail(c, PTMI_EINVAL, "the live-rays workspace is not 8-byte aligned");
    if (work_bytes < live_rays_bytes(candidates)) return fail(c, PTMI_EINVAL, "the live-rays workspace is smaller than ptmi_live_rays_bytes(count)");
    PTMI_HIP(c, hipSetDevice(c->device));
    PTMI_HIP(c, launch_live_rays(d_throughput, n, d_index, candidates, d_live, d_count, d_work, c->stream));
    return PTMI_OK;
}
