// verify_sincos_quadrant.cpp -- the host side of the proof that the quadrant-by-comparison sin/cos (ptmi::sincos_quadrant, ptmi_core.h)
// returns what the literal restatement of glibc's algorithm (ptmi::sincos_t<false>) returns.  A stand-alone program, no GPU:
//   1. it re-derives, from reduce_fast's literal text, the first binary32 patterns at which the quadrant n changes 0 -> 1 -> 2 and
//      0 -> -1 -> -2 (every pattern with |y| < 4 is visited, n must be monotone) and refuses to pass unless they are the header's
//      kQuadT1p / kQuadT2p / kQuadT1n / kQuadT2n; every pattern sincos_quadrant_covers() accepts must have n in {-1, 0, 1} and |y| >= 2^-12,
//      every other pattern of the interval (T2n, T2p) must be one of the |y| < 2^-12, and inf / NaN / the thresholds must be refused;
//   2. it compares sine and cosine bitwise for the covered patterns:
//        --full   every one of them (2.2e8: the patterns below 2^-12 are nine tenths of the interval; seconds on 16 threads) -- the tool
//        (default) every 4096th, and all within 65 536 ulps of +-T1, +-T2, +-2^-12 and +-0 -- what tests/test_sincos_quadrant.py runs
// Host binary64 is IEEE and the flags keep contraction off; the FUSED polynomials are __builtin_fma (one rounding), as on the device.
// Prints one JSON line; exit status 0 iff everything holds.
// build: g++ -O2 -std=c++17 -ffp-contract=off -fno-fast-math -fopenmp -D__HIP_PLATFORM_AMD__ -I<rocm>/include -Ihaskell-path-tracer_amd/csrc
//        tools/verify_sincos_quadrant.cpp -o verify_sincos_quadrant          (OMP_NUM_THREADS <= 16)
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
#include <omp.h>
#include "ptmi_core.h"

namespace {

// sincosf.h reduce_fast(), the quadrant only
int quadrant_literal(float y)
{
    const double x = (double)y;
    const double r = x * 0x1.45F306DC9C883p+23;
    return ((int32_t)r + 0x800000) >> 24;
}

struct Step { uint32_t bits; int from, to; };

bool same(float a, float b) { return ptmi::f2u(a) == ptmi::f2u(b); }

}  // namespace

int main(int argc, char **argv)
{
    const bool full = argc > 1 && !strcmp(argv[1], "--full");
    if (omp_get_max_threads() > 16) omp_set_num_threads(16);
    const uint32_t kLimit = 0x40800000u;                     // 4.0: beyond the second step on either side
    const uint32_t tiny = ptmi::kQuadTiny;
    bool ok = true;

    // ---- 1. the thresholds, and what sincos_quadrant_covers accepts
    std::vector<Step> steps[2];
    unsigned long long cover_errors = 0;
    for (int sign = 0; sign < 2; ++sign) {
        const uint32_t s = sign ? 0x80000000u : 0u;
#pragma omp parallel for schedule(static) reduction(+ : cover_errors)
        for (int64_t chunk = 0; chunk < (int64_t)(kLimit >> 16); ++chunk) {
            const uint32_t first = (uint32_t)chunk << 16;
            int prev = quadrant_literal(ptmi::u2f(s | (first ? first - 1 : 0u)));
            for (uint32_t b = first; b < first + 0x10000u; ++b) {
                const float y = ptmi::u2f(s | b);
                const int n = quadrant_literal(y);
                if (n != prev) {
#pragma omp critical
                    steps[sign].push_back(Step{s | b, prev, n});
                    prev = n;
                }
                const bool inside = sign ? (s | b) < ptmi::kQuadT2n : b < ptmi::kQuadT2p;      // strictly inside (T2n, T2p) as numbers
                const bool want = inside && b >= tiny;
                if (ptmi::sincos_quadrant_covers(y) != want) ++cover_errors;
                if (want && (n < -1 || n > 1)) ++cover_errors;
            }
        }
        std::sort(steps[sign].begin(), steps[sign].end(), [](const Step &a, const Step &c) { return a.bits < c.bits; });
    }
    // beyond the scanned interval nothing may be covered: a stride over every larger magnitude, inf and NaN among them
    for (uint64_t b = kLimit; b < 0x80000000ull; b += 4093)
        if (ptmi::sincos_quadrant_covers(ptmi::u2f((uint32_t)b)) || ptmi::sincos_quadrant_covers(ptmi::u2f((uint32_t)b | 0x80000000u))) ++cover_errors;
    for (uint32_t b : {0x7f800000u, 0xff800000u, 0x7fc00000u, 0xffc00000u, 0x7f800001u, 0xffffffffu, 0x7fffffffu})
        if (ptmi::sincos_quadrant_covers(ptmi::u2f(b))) ++cover_errors;
    const uint32_t got[4] = {steps[0].size() > 0 ? steps[0][0].bits : 0u, steps[0].size() > 1 ? steps[0][1].bits : 0u,
                             steps[1].size() > 0 ? steps[1][0].bits : 0u, steps[1].size() > 1 ? steps[1][1].bits : 0u};
    const bool monotone = steps[0].size() >= 2 && steps[1].size() >= 2 &&
                          std::all_of(steps[0].begin(), steps[0].end(), [](const Step &t) { return t.to == t.from + 1; }) &&
                          std::all_of(steps[1].begin(), steps[1].end(), [](const Step &t) { return t.to == t.from - 1; }) &&
                          steps[0][0].from == 0 && steps[1][0].from == 0;
    const bool thresholds = monotone && got[0] == ptmi::kQuadT1p && got[1] == ptmi::kQuadT2p && got[2] == ptmi::kQuadT1n && got[3] == ptmi::kQuadT2n;
    ok = ok && thresholds && cover_errors == 0;

    // ---- 2. the core against the literal form
    unsigned long long checked = 0, mismatches = 0;
    uint32_t first_bad = 0xffffffffu;
    auto compare = [&](uint32_t bits, unsigned long long &n_checked, unsigned long long &n_bad, uint32_t &bad_at) {
        const float y = ptmi::u2f(bits);
        if (!ptmi::sincos_quadrant_covers(y)) return;
        float s0, c0, s1, c1;
        ptmi::sincos_t<false>(y, s0, c0);
        ptmi::sincos_quadrant(y, s1, c1);
        ++n_checked;
        if (!same(s0, s1) || !same(c0, c1)) { ++n_bad; if (bits < bad_at) bad_at = bits; }
    };
    if (full) {
#pragma omp parallel for schedule(static) reduction(+ : checked, mismatches) reduction(min : first_bad)
        for (int64_t chunk = 0; chunk < (int64_t)(kLimit >> 16) * 2; ++chunk) {
            const uint32_t s = (chunk & 1) ? 0x80000000u : 0u, first = (uint32_t)(chunk >> 1) << 16;
            for (uint32_t b = first; b < first + 0x10000u; ++b) compare(s | b, checked, mismatches, first_bad);
        }
    } else {
#pragma omp parallel for schedule(static) reduction(+ : checked, mismatches) reduction(min : first_bad)
        for (int64_t k = 0; k < (int64_t)(kLimit >> 12); ++k) {
            compare((uint32_t)k << 12, checked, mismatches, first_bad);
            compare(((uint32_t)k << 12) | 0x80000000u, checked, mismatches, first_bad);
        }
        const uint32_t centres[4] = {ptmi::kQuadT1p, ptmi::kQuadT2p, tiny, 0u};      // magnitudes; the negative thresholds lie within 2 ulps of them
#pragma omp parallel for schedule(static) reduction(+ : checked, mismatches) reduction(min : first_bad)
        for (int64_t k = 0; k < 4 * 2 * 131073; ++k) {
            const uint32_t centre = centres[k / (2 * 131073)], s = (k / 131073) & 1 ? 0x80000000u : 0u;
            const int64_t b = (int64_t)centre + (k % 131073) - 65536;
            if (b >= 0) compare(s | (uint32_t)b, checked, mismatches, first_bad);
        }
    }
    ok = ok && mismatches == 0 && checked > 0;
    printf("{\"mode\": \"%s\", \"T1p\": \"%#x\", \"T2p\": \"%#x\", \"T1n\": \"%#x\", \"T2n\": \"%#x\", \"thresholds_equal_header\": %s, \"quadrant_monotone\": %s, "
           "\"cover_errors\": %llu, \"checked\": %llu, \"mismatches\": %llu, \"first_mismatch\": \"%#x\", \"ok\": %s}\n",
           full ? "full" : "strided+windows", got[0], got[1], got[2], got[3], thresholds ? "true" : "false", monotone ? "true" : "false",
           cover_errors, checked, mismatches, mismatches ? first_bad : 0u, ok ? "true" : "false");
    return ok ? 0 : 1;
}
