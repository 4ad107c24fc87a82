// ptmi_share.h -- which spheres of a linear scene repeat their predecessor's x-y work in check_hit's sphere test (ptmi_device.h,
// SphereShare::kXY).  A pure host function over plain floats: it includes nothing of HIP, so that a stand-alone program can call it
// (tests/cxx/shared_xy_mask_main.cpp).
#pragma once

#include <stddef.h>
#include <stdint.h>
#include <string.h>

namespace ptmi {

constexpr int kShareBits = 64;             // spheres from this index on never share

// Bit i is set iff 1 <= i < min(n_spheres, 64) and sphere i's cx and cy have the BIT PATTERNS of sphere i - 1's.  `centres` holds
// cx, cy at [stride * i] and [stride * i + 1].  Bits, not values: +0 and -0 do not share ((+0) - ox and (-0) - ox differ for ox = +-0);
// equal NaN patterns do (the same operations on the same bits give the same bits).
inline uint64_t shared_xy_mask(const float *centres, size_t stride, int n_spheres)
{
    uint64_t mask = 0;
    const int n = n_spheres < kShareBits ? n_spheres : kShareBits;
    for (int i = 1; i < n; ++i)
        if (memcmp(centres + stride * (size_t)i, centres + stride * (size_t)(i - 1), 2 * sizeof(float)) == 0) mask |= uint64_t{1} << i;
    return mask;
}

}  // namespace ptmi
