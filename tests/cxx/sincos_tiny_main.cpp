// sincos_tiny_main.cpp -- the per-angle form of the render kernels' fast sin/cos with the fix-up for |y| < 2^-12 (ptmi::sincos_quadrant_tiny,
// ptmi_core.h: sincos_quadrant followed by sincos_t's last line) against the literal restatement ptmi::sincos_t<false>, bitwise, on the host.
// A stand-alone program (tests/test_sincos_tiny_host.py builds it with AddressSanitizer + UndefinedBehaviorSanitizer and runs it):
//   * every pattern within 65 536 of +-0, of +-2^-12 and of the denormal boundary (+-0x00800000), both sides where there is one;
//   * every 1 024th pattern below 2^-12, both signs;
//   * the guards: sincos_quadrant_tiny_covers is sincos_quadrant_covers or tiny inside (T2n, T2p), refuses the thresholds, inf and NaN, and
//     sincos_is_tiny is sincos_t's `top < 0x398`.
// Prints SINCOS_TINY_OK and the counts; exit status 0 iff everything holds.
#include <cstdint>
#include <cstdio>
#include "ptmi_core.h"

namespace {

unsigned long long checked = 0, mismatches = 0, guard_errors = 0;
uint32_t first_bad = 0;

void compare(uint32_t bits)
{
    const float y = ptmi::u2f(bits);
    const bool tiny = ((bits >> 20) & 0x7ffu) < 0x398u;                       // sincos_t's own test
    if (ptmi::sincos_is_tiny(y) != tiny) ++guard_errors;
    if (ptmi::sincos_quadrant_tiny_covers(y) != (ptmi::sincos_quadrant_covers(y) || tiny)) ++guard_errors;
    if (!ptmi::sincos_quadrant_tiny_covers(y)) { ++guard_errors; return; }   // (every pattern this program visits is inside the range)
    float s0, c0, s1, c1;
    ptmi::sincos_t<false>(y, s0, c0);
    ptmi::sincos_quadrant_tiny(y, s1, c1);
    ++checked;
    if (ptmi::f2u(s0) != ptmi::f2u(s1) || ptmi::f2u(c0) != ptmi::f2u(c1)) {
        if (!mismatches) first_bad = bits;
        ++mismatches;
    }
    if (tiny && (ptmi::f2u(s1) != bits || ptmi::f2u(c1) != 0x3f800000u)) {   // (y, 1), the sign of a zero and denormals kept
        if (!mismatches) first_bad = bits;
        ++mismatches;
    }
}

void window(uint32_t centre)
{
    for (int64_t b = (int64_t)centre - 65536; b <= (int64_t)centre + 65536; ++b) {
        if (b < 0) continue;
        compare((uint32_t)b);
        compare((uint32_t)b | 0x80000000u);
    }
}

}  // namespace

int main()
{
    window(0u);
    window(ptmi::kQuadTiny);
    window(0x00800000u);                                                      // the smallest normal number
    for (uint32_t b = 0; b < ptmi::kQuadTiny; b += 1024) {
        compare(b);
        compare(b | 0x80000000u);
    }
    for (uint32_t b : {ptmi::kQuadT2p, ptmi::kQuadT2n, 0x7f800000u, 0xff800000u, 0x7fc00000u, 0xffc00000u, 0x7f800001u, 0xffffffffu, 0x42f00000u, 0xc2f00000u})
        if (ptmi::sincos_quadrant_tiny_covers(ptmi::u2f(b))) ++guard_errors;
    for (uint32_t b : {ptmi::kQuadT2p - 1u, ptmi::kQuadT2n - 1u, ptmi::kQuadT1p, ptmi::kQuadT1n})
        if (!ptmi::sincos_quadrant_tiny_covers(ptmi::u2f(b)) || ptmi::sincos_is_tiny(ptmi::u2f(b))) ++guard_errors;
    const bool ok = mismatches == 0 && guard_errors == 0 && checked >= 2ull * (3 * 65536 + (ptmi::kQuadTiny >> 10));
    printf("checked %llu mismatches %llu (first %#x) guard_errors %llu\n", checked, mismatches, first_bad, guard_errors);
    if (ok) printf("SINCOS_TINY_OK\n");
    return ok ? 0 : 1;
}
