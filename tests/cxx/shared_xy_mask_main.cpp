// shared_xy_mask_main.cpp -- shared_xy_mask (csrc/ptmi_share.h), the mask of spheres that repeat their predecessor's (cx, cy) bits, driven by a
// stand-alone program (tests/test_shared_xy_mask_host.py compiles it with AddressSanitizer + UndefinedBehaviorSanitizer and runs it).
// Every array is heap memory of exactly the size the call may read, so a read past n_spheres is a sanitizer report.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "ptmi_share.h"

namespace {

int failures = 0;

float bits(uint32_t u) { float f; memcpy(&f, &u, sizeof f); return f; }

// centres as the packed scene holds them: (cx, cy, cz, r*r), stride 4
uint64_t mask_of(const std::vector<float> &xy)
{
    const int n = (int)(xy.size() / 2);
    std::vector<float> rows((size_t)n * 4);
    for (int i = 0; i < n; ++i) { rows[4 * i] = xy[2 * i]; rows[4 * i + 1] = xy[2 * i + 1]; rows[4 * i + 2] = -6.0f - (float)i; rows[4 * i + 3] = 1.0f; }
    return ptmi::shared_xy_mask(rows.data(), 4, n);
}

void expect(const char *what, uint64_t got, uint64_t want)
{
    if (got == want) return;
    ++failures;
    printf("FAILED %s: mask %#llx, expected %#llx\n", what, (unsigned long long)got, (unsigned long long)want);
}

std::vector<float> repeat(int n, float x, float y)
{
    std::vector<float> v;
    for (int i = 0; i < n; ++i) { v.push_back(x); v.push_back(y); }
    return v;
}

}  // namespace

int main()
{
    // no sphere: nothing is read (a null array)
    expect("n = 0", ptmi::shared_xy_mask(nullptr, 4, 0), 0);
    expect("n = 1", mask_of({1.0f, 2.0f}), 0);
    // S16's layout: 5 loose spheres, then three runs of three
    {
        std::vector<float> v = {-3.0f, 0.0f, 6.0f, 0.0f, 0.0f, 1.0f, 1.0f, -2.0f, 0.0f, 9.0f};
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) { v.push_back(-6.0f + 6.0f * (float)i); v.push_back(0.0f); }
        expect("S16", mask_of(v), (3ull << 6) | (3ull << 9) | (3ull << 12));
    }
    // runs of length 1 .. 5 starting at every index modulo 4 (index 0 and the last sphere included), n_spheres 1 .. 9
    for (int n = 1; n <= 9; ++n)
        for (int start = 0; start < n; ++start)
            for (int len = 1; len <= 5 && start + len <= n; ++len) {
                std::vector<float> v;
                uint64_t want = 0;
                for (int i = 0; i < n; ++i) {
                    const bool in_run = i >= start && i < start + len;
                    v.push_back(in_run ? 2.5f : 10.0f + (float)i);
                    v.push_back(in_run ? -1.5f : 20.0f + (float)i);
                    if (in_run && i > start) want |= 1ull << i;
                }
                char what[64];
                snprintf(what, sizeof what, "n = %d, run of %d at %d", n, len, start);
                expect(what, mask_of(v), want);
            }
    // equal in cx only, in cy only: no sharing
    expect("cx only", mask_of({1.0f, 2.0f, 1.0f, 3.0f, 1.0f, 4.0f}), 0);
    expect("cy only", mask_of({1.0f, 2.0f, 3.0f, 2.0f, 4.0f, 2.0f}), 0);
    // +0 and -0 are equal values and different bits: no sharing, in cx or in cy; equal zeros share
    expect("+0 / -0 in cx", mask_of({0.0f, 1.0f, -0.0f, 1.0f, 0.0f, 1.0f}), 0);
    expect("+0 / -0 in cy", mask_of({1.0f, -0.0f, 1.0f, 0.0f}), 0);
    expect("-0 / -0", mask_of({-0.0f, -0.0f, -0.0f, -0.0f}), 2);
    // two fully coincident spheres share
    expect("coincident", mask_of({4.0f, 5.0f, 4.0f, 5.0f}), 2);
    // NaN: equal patterns share (the same operations on the same bits), different patterns do not, although neither compares equal
    {
        const float q = bits(0x7fc00000u), other = bits(0x7fc00001u);
        expect("equal NaN patterns", mask_of({q, 1.0f, q, 1.0f, q, 1.0f}), 6);
        expect("different NaN patterns", mask_of({q, 1.0f, other, 1.0f}), 0);
        expect("NaN in cy", mask_of({1.0f, q, 1.0f, q, 1.0f, 2.0f}), 2);
    }
    // 64 and 65 spheres of one run: bit 0 never, bits 1 .. 63, nothing from index 64 on (and no read past the array)
    expect("n = 64", mask_of(repeat(64, 1.0f, 2.0f)), ~1ull);
    expect("n = 65", mask_of(repeat(65, 1.0f, 2.0f)), ~1ull);
    expect("n = 200", mask_of(repeat(200, 1.0f, 2.0f)), ~1ull);
    {
        std::vector<float> v = repeat(65, 1.0f, 2.0f);
        v[2 * 63] = 7.0f;                                   // sphere 63 stands alone; 64 repeats nothing that counts
        expect("n = 65, break at 63", mask_of(v), ~1ull & ~(1ull << 63));
    }
    // another stride: bare (cx, cy) pairs
    {
        const std::vector<float> v = {1.0f, 2.0f, 1.0f, 2.0f, 3.0f, 2.0f};
        expect("stride 2", ptmi::shared_xy_mask(v.data(), 2, 3), 2);
    }
    if (failures) return 1;
    printf("SHARED_XY_MASK_OK\n");
    return 0;
}
