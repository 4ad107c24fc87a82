// ptmi_ray_order.cpp -- the ray order's calls of include/ptmi.h: ptmi_ray_order_device (argument checks and the launches of
// ptmi_ray_order.hip) and its host twins ptmi_ray_order / ptmi_ray_order_keys, which take host memory, use no device and run the key of
// ptmi_ray_order.h -- the specification the device order is tested against.
#include "ptmi_ctx.h"

#include <algorithm>
#include <vector>

#include "ptmi_ray_order.h"

using namespace ptmi;

namespace {

// The keys of n host rays: the box of the placed rays' origins (smallest and largest ordered image per axis), then ray_key
void host_ray_keys(const float *rays, int n, uint64_t *keys)
{
    uint32_t box[kRayBoxWords];
    for (int a = 0; a < 3; ++a) { box[kRayLo + a] = 0xffffffffu; box[kRayHi + a] = 0u; }
    for (int i = 0; i < n; ++i) {
        const float *r = rays + 6 * (size_t)i;
        if (!ray_placed(r)) continue;
        for (int a = 0; a < 3; ++a) {
            box[kRayLo + a] = std::min(box[kRayLo + a], ordered_image(r[a]));
            box[kRayHi + a] = std::max(box[kRayHi + a], ordered_image(r[a]));
        }
    }
    float lo[3], hi[3];
    for (int a = 0; a < 3; ++a) { lo[a] = ordered_value(box[kRayLo + a]); hi[a] = ordered_value(box[kRayHi + a]); }
    for (int i = 0; i < n; ++i) {
        const float *r = rays + 6 * (size_t)i;
        keys[i] = ray_placed(r) ? ray_key(r, lo, hi) : kRayNotPlaced;
    }
}

}  // namespace

extern "C" size_t ptmi_ray_order_bytes(int n) { return ray_order_bytes(n); }

extern "C" int ptmi_ray_order_keys(const float *rays, int n, uint64_t *keys)
{
    if (n < 0 || (n > 0 && (!rays || !keys))) return PTMI_EINVAL;
    if (n > PTMI_RAY_ORDER_MAX) return PTMI_ELIMIT;
    host_ray_keys(rays, n, keys);
    return PTMI_OK;
}

extern "C" int ptmi_ray_order(const float *rays, int n, int32_t *order)
{
    if (n < 0 || (n > 0 && (!rays || !order))) return PTMI_EINVAL;
    if (n > PTMI_RAY_ORDER_MAX) return PTMI_ELIMIT;
    std::vector<uint64_t> keys((size_t)n);
    host_ray_keys(rays, n, keys.data());
    for (int i = 0; i < n; ++i) order[i] = i;
    const uint64_t *kp = keys.data();
    std::sort(order, order + n, [kp](int32_t x, int32_t y) { return kp[x] < kp[y] || (kp[x] == kp[y] && x < y); });
    return PTMI_OK;
}

// Refusals first (nothing enqueued, nothing written), then the launches on the context's stream -- no synchronisation, no allocation, no
// copy to the host.  No scene is needed: the key is a function of the rays.
extern "C" int ptmi_ray_order_device(ptmi_ctx *c, const float *d_rays, int n, int32_t *d_order, void *d_work, size_t work_bytes)
{
    if (!c) return PTMI_EINVAL;
    std::lock_guard<std::mutex> lock(c->mu);
    if (n < 0 || (n > 0 && (!d_rays || !d_order || !d_work))) return fail(c, PTMI_EINVAL, "bad ray-order arguments");
    if (n > PTMI_RAY_ORDER_MAX) return fail(c, PTMI_ELIMIT, "more rays than PTMI_RAY_ORDER_MAX");
    if (n == 0) return PTMI_OK;
    if ((reinterpret_cast<uintptr_t>(d_work) & 7u) != 0) return fail(c, PTMI_EINVAL, "the ray-order workspace is not 8-byte aligned");
    if (work_bytes < ray_order_bytes(n)) return fail(c, PTMI_EINVAL, "the ray-order workspace is smaller than ptmi_ray_order_bytes(n)");
    PTMI_HIP(c, hipSetDevice(c->device));
    PTMI_HIP(c, launch_ray_order(d_rays, n, d_work, d_order, c->stream));
    return PTMI_OK;
}
