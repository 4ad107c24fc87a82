// ptmi_ray_order.h -- the key a batch of rays is ordered by (ptmi_ray_order_device, ptmi_ray_order, ptmi_ray_order_keys), ONE definition
// for the host twins (ptmi_ray_order.cpp) and the device (ptmi_ray_order.hip): the two are bit-equal because they run these operations.
//
// A ray (o, d) is PLACED when its six words are finite and s = (|dx| + |dy|) + |dz| > 0.  lo / hi: the f32 box of the placed rays'
// origins.  Every operation in f64 and rounded on its own (the library is compiled without contraction), in exactly this order:
//   origin cell, per axis a, 8 bits:
//     qo[a] = hi[a] == lo[a] ? 0 : min(255, (int)floor(((double)o[a] - (double)lo[a]) * 256.0 / ((double)hi[a] - (double)lo[a])))
//             (the product first, then the IEEE division)
//   direction cell, the octahedral map, 10 bits per coordinate:
//     u = dx / s, v = dy / s
//     dz < 0:  (u, v) = ((1 - |v|) * sg(u), (1 - |u|) * sg(v)), both from the old values, sg(x) = x >= 0 ? 1 : -1
//     qu = min(1023, (int)floor((u * 0.5 + 0.5) * 1024.0)), qv likewise
//   key = morton3(qox, qoy, qoz) << 20 | morton2(qu, qv): bit i of qox is bit 3 i + 2 of morton3, of qoy bit 3 i + 1, of qoz bit 3 i;
//         bit i of qu is bit 2 i + 1 of morton2, of qv bit 2 i.  44 bits, origins major: bounce rays group by place, and rays that share
//         an origin (a camera's) by direction.
// A ray that is not placed has the key 1 << 44: behind every placed ray.  The order ascends by (key, original index).
#pragma once

#include "ptmi_mesh_box.h"

namespace ptmi {

constexpr int kRayOriginBits = 8, kRayDirectionBits = 10;                       // per axis, per coordinate
constexpr int kRayKeyBits = 3 * kRayOriginBits + 2 * kRayDirectionBits;          // 44
constexpr uint64_t kRayNotPlaced = 1ull << kRayKeyBits;

// The box of the placed rays' origins as ordered images (ptmi_mesh_box.h), the words behind the sort's part of the workspace: all
// ones in [kRayLo, kRayHi), zero in [kRayHi, kRayBoxWords) before the box kernel.
enum { kRayLo = 0, kRayHi = 3, kRayBoxWords = 6 };

PTMI_HD bool ray_placed(const float r[6])
{
    bool finite = true;
    for (int k = 0; k < 6; ++k) finite = finite && finite_f32(r[k]);
    const double s = (__builtin_fabs((double)r[3]) + __builtin_fabs((double)r[4])) + __builtin_fabs((double)r[5]);
    return finite && s > 0.0;
}

PTMI_HD uint64_t ray_spread(uint32_t q, int bits, int step)                    // bit i -> bit step * i
{
    uint64_t r = 0;
    for (int i = 0; i < bits; ++i) r |= (uint64_t)((q >> i) & 1u) << (step * i);
    return r;
}

PTMI_HD uint32_t ray_origin_cell(float o, float lo, float hi)
{
    if (hi == lo) return 0u;
    const double num = ((double)o - (double)lo) * 256.0;
    const int q = (int)__builtin_floor(num / ((double)hi - (double)lo));
    return (uint32_t)(q < 255 ? q : 255);
}

PTMI_HD uint32_t ray_direction_cell(double u)
{
    const int q = (int)__builtin_floor((u * 0.5 + 0.5) * 1024.0);
    return (uint32_t)(q < 1023 ? q : 1023);
}

// ... of a placed ray
PTMI_HD uint64_t ray_key(const float r[6], const float lo[3], const float hi[3])
{
    const double s = (__builtin_fabs((double)r[3]) + __builtin_fabs((double)r[4])) + __builtin_fabs((double)r[5]);
    double u = (double)r[3] / s, v = (double)r[4] / s;
    if (r[5] < 0.0f) {
        const double fu = (1.0 - __builtin_fabs(v)) * (u >= 0.0 ? 1.0 : -1.0), fv = (1.0 - __builtin_fabs(u)) * (v >= 0.0 ? 1.0 : -1.0);
        u = fu; v = fv;
    }
    const uint64_t origin = (ray_spread(ray_origin_cell(r[0], lo[0], hi[0]), kRayOriginBits, 3) << 2) |
                            (ray_spread(ray_origin_cell(r[1], lo[1], hi[1]), kRayOriginBits, 3) << 1) |
                            ray_spread(ray_origin_cell(r[2], lo[2], hi[2]), kRayOriginBits, 3);
    const uint64_t direction = (ray_spread(ray_direction_cell(u), kRayDirectionBits, 2) << 1) | ray_spread(ray_direction_cell(v), kRayDirectionBits, 2);
    return (origin << (2 * kRayDirectionBits)) | direction;
}

}  // namespace ptmi
