// verify_sincos_quadrant.hip -- proof by exhaustion, on the device, that the quadrant-by-comparison sin/cos the render kernels run for
// a bounce's three half angles (ptmi::sincos_quadrant, ptmi_core.h) returns the same binary32 sine and cosine as the literal
// restatement of glibc's algorithm (ptmi::sincos_t<false>) for EVERY binary32 argument the form covers (sincos_quadrant_covers:
// T2n < y < T2p, |y| >= 2^-12), and that every pattern it does not cover is one the wave guard refuses.  All 2^32 patterns are
// visited.  Prints a JSON line; exit status 0 iff 0 mismatches.  (tools/verify_sincos_quadrant.cpp is the same comparison on the host,
// and re-derives the thresholds.)
// build+run: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -Ihaskell-path-tracer_amd/csrc
//            tools/verify_sincos_quadrant.hip -o verify_sincos_quadrant_gpu && ./verify_sincos_quadrant_gpu
#include <hip/hip_runtime.h>
#include <cstdio>
#include "ptmi_core.h"

__global__ void __launch_bounds__(256) compare_all(unsigned long long *counts, unsigned int *first_bad)
{
    const unsigned int tid = blockIdx.x * 256u + threadIdx.x;          // 2^24 threads
    unsigned int bad = 0, covered = 0;
    for (unsigned int k = 0; k < 256u; ++k) {
        const unsigned int bits = (k << 24) | tid;                     // every pattern exactly once
        const float y = ptmi::u2f(bits);
        if (!ptmi::sincos_quadrant_covers(y)) continue;
        ++covered;
        float s0, c0, s1, c1;
        ptmi::sincos_t<false>(y, s0, c0);
        ptmi::sincos_quadrant(y, s1, c1);
        if (ptmi::f2u(s0) != ptmi::f2u(s1) || ptmi::f2u(c0) != ptmi::f2u(c1)) { ++bad; atomicMin(first_bad, bits); }
    }
    if (covered) atomicAdd(counts, (unsigned long long)covered);
    if (bad) atomicAdd(counts + 1, (unsigned long long)bad);
}

int main()
{
    unsigned long long *d_counts, h_counts[2] = {0, 0}; unsigned int *d_first, h_first = 0xffffffffu;
    if (hipMalloc(&d_counts, 16) != hipSuccess || hipMalloc(&d_first, 4) != hipSuccess) { printf("no device\n"); return 2; }
    (void)hipMemcpy(d_counts, h_counts, 16, hipMemcpyHostToDevice);
    (void)hipMemcpy(d_first, &h_first, 4, hipMemcpyHostToDevice);
    hipLaunchKernelGGL(compare_all, dim3(1u << 16), dim3(256), 0, 0, d_counts, d_first);
    if (hipDeviceSynchronize() != hipSuccess) { printf("kernel failed\n"); return 2; }
    (void)hipMemcpy(h_counts, d_counts, 16, hipMemcpyDeviceToHost);
    (void)hipMemcpy(&h_first, d_first, 4, hipMemcpyDeviceToHost);
    // the patterns the form covers: [2^-12, T2p) and the same magnitudes up to and excluding T2n's
    const unsigned long long expected = (unsigned long long)(ptmi::kQuadT2p - ptmi::kQuadTiny) + ((ptmi::kQuadT2n & 0x7fffffffu) - ptmi::kQuadTiny);
    printf("{\"patterns_visited\": 4294967296, \"covered\": %llu, \"covered_expected\": %llu, \"mismatches\": %llu, \"first_mismatch\": \"%#x\"}\n",
           h_counts[0], expected, h_counts[1], h_counts[1] ? h_first : 0u);
    return (h_counts[1] != 0 || h_counts[0] != expected) ? 1 : 0;
}
