// ptmi_trace_streams.cpp -- render Streams along a caller's rays: ptmi_trace_streams_bytes, ptmi_trace_streams_device and
// ptmi_trace_streams_indexed_device of include/ptmi.h (argument checks and the one launch of ptmi_trace_streams.hip).
#include "ptmi_ctx.h"

using namespace ptmi;

extern "C" size_t ptmi_trace_streams_bytes(int count) { return trace_streams_bytes(count); }

// The refusals (nothing enqueued, nothing written), then one launch on the context's stream -- no synchronisation, no allocation, no copy.
// The context's state planes, partition, camera, dispatch order and statistics are not touched: what the cap cut and a full stack dropped
// goes to d_lost.
static int trace_streams(ptmi_ctx *c, const float *d_rays, int n, const int32_t *d_index, int m, bool indexed, int n_spp, float *d_color, uint32_t *d_seed,
                         uint64_t *d_lost, void *d_work, size_t work_bytes)
{
    if (!c) return PTMI_EINVAL;
    std::lock_guard<std::mutex> lock(c->mu);
    if (n < 0 || (n > 0 && (!d_rays || !d_color || !d_seed)) || (indexed && (m < 0 || (m > 0 && !d_index)))) return fail(c, PTMI_EINVAL, "bad ray-stream arguments");
    if ((reinterpret_cast<uintptr_t>(d_lost) & 7u) != 0) return fail(c, PTMI_EINVAL, "d_lost is not 8-byte aligned");
    if (!c->scene.packed.p) return fail(c, PTMI_ESTATE, "ptmi_set_scene has not been called");
    if (c->scene.has_glass && c->opt_seed_rule == PTMI_SEED_FROM_RESULT)
        return fail(c, PTMI_EINVAL, "PTMI_SEED_FROM_RESULT is undefined when rays split (GLASS): several results race for one pixel's seed");
    const int lanes = indexed ? m : n;
    if (c->scene.has_glass && n > 0 && lanes > 0) {
        if (!d_work) return fail(c, PTMI_EINVAL, "bad ray-stream arguments");
        if ((reinterpret_cast<uintptr_t>(d_work) & 15u) != 0) return fail(c, PTMI_EINVAL, "the ray-stream workspace is not 16-byte aligned");
        if (work_bytes < trace_streams_bytes(lanes)) return fail(c, PTMI_EINVAL, "the ray-stream workspace is smaller than ptmi_trace_streams_bytes(lanes)");
    }
    if (n == 0 || n_spp <= 0 || (indexed && m == 0)) return PTMI_OK;
    PTMI_HIP(c, hipSetDevice(c->device));
    const RayCallScene r = ray_call_scene(c);
    PTMI_HIP(c, launch_trace_streams(r.scene, r.bvh, r.mesh, d_rays, n, indexed ? d_index : nullptr, m, n_spp, c->opt_step_cap,
                                     effective_seed_rule(c) == PTMI_SEED_FROM_RESULT, d_color, d_seed, reinterpret_cast<unsigned long long *>(d_lost),
                                     c->scene.has_glass ? d_work : nullptr, c->stream));
    return PTMI_OK;
}

extern "C" int ptmi_trace_streams_device(ptmi_ctx *c, const float *d_rays, int n, int n_spp, float *d_color, uint32_t *d_seed, uint64_t *d_lost, void *d_work,
                                         size_t work_bytes)
{
    return trace_streams(c, d_rays, n, nullptr, 0, false, n_spp, d_color, d_seed, d_lost, d_work, work_bytes);
}

extern "C" int ptmi_trace_streams_indexed_device(ptmi_ctx *c, const float *d_rays, int n, const int32_t *d_index, int m, int n_spp, float *d_color,
                                                 uint32_t *d_seed, uint64_t *d_lost, void *d_work, size_t work_bytes)
{
    return trace_streams(c, d_rays, n, d_index, m, true, n_spp, d_color, d_seed, d_lost, d_work, work_bytes);
}
