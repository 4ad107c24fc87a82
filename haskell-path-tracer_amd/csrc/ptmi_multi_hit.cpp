// ptmi_multi_hit.cpp -- the multi-hit calls of include/ptmi.h: ptmi_trace_rays_multi_device / ptmi_trace_rays_multi_indexed_device (argument
// checks and the launch of ptmi_multi_hit.hip's kernels).
#include "ptmi_ctx.h"

using namespace ptmi;

// The refusals of ptmi_trace_rays_device and k's (nothing enqueued, nothing written), then one launch on the context's stream -- no
// synchronisation, no allocation, no scratch.  The context's state planes, statistics and dispatch order are not touched.
static int trace_rays_multi(ptmi_ctx *c, const float *d_rays, const float *d_t_max, int n, const int32_t *d_index, int m, bool indexed, int k, float *d_t,
                            int32_t *d_idx, int32_t *d_count)
{
    if (!c) return PTMI_EINVAL;
    std::lock_guard<std::mutex> lock(c->mu);
    if (n < 0 || k < 1 || (n > 0 && (!d_rays || !d_t || !d_idx || !d_count)) || (indexed && (m < 0 || (m > 0 && !d_index))))
        return fail(c, PTMI_EINVAL, "bad multi-hit arguments");
    if (k > PTMI_MULTI_HIT_MAX) return fail(c, PTMI_ELIMIT, "k is larger than PTMI_MULTI_HIT_MAX");
    if (!c->scene.packed.p) return fail(c, PTMI_ESTATE, "ptmi_set_scene has not been called");
    if (n == 0 || (indexed && m == 0)) return PTMI_OK;
    PTMI_HIP(c, hipSetDevice(c->device));
    const RayCallScene r = ray_call_scene(c);
    PTMI_HIP(c, launch_trace_rays_multi(r.scene, r.bvh, r.mesh, d_rays, d_t_max, n, indexed ? d_index : nullptr, m, k, d_t, d_idx, d_count, c->stream));
    return PTMI_OK;
}

extern "C" int ptmi_trace_rays_multi_device(ptmi_ctx *c, const float *d_rays, const float *d_t_max, int n, int k, float *d_t, int32_t *d_idx, int32_t *d_count)
{
    return trace_rays_multi(c, d_rays, d_t_max, n, nullptr, 0, false, k, d_t, d_idx, d_count);
}

extern "C" int ptmi_trace_rays_multi_indexed_device(ptmi_ctx *c, const float *d_rays, const float *d_t_max, int n, const int32_t *d_index, int m, int k,
                                                    float *d_t, int32_t *d_idx, int32_t *d_count)
{
    return trace_rays_multi(c, d_rays, d_t_max, n, d_index, m, true, k, d_t, d_idx, d_count);
}
