// multi_hit_hostsan.cpp -- the host side of the multi-hit query (csrc/ptmi_multi_hit.cpp and the launcher of csrc/ptmi_multi_hit.hip) under
// AddressSanitizer + UBSan, as a stand-alone program: linked against the library built with its host code instrumented and against the
// HIP stand-in (tests/cxx/hip_stub.cpp: device memory is host memory, kernels do not run), run directly by
// tests/test_multi_hit_host_sanitized.py.  It provokes every refusal of ptmi_trace_rays_multi_device and
// ptmi_trace_rays_multi_indexed_device on a linear, a BVH and a mesh scene, calls both at every k on aligned and misaligned rows, and lets
// every runtime call of the two entries fail in turn; no refused or failed call writes to an output.
#include <climits>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include <hip/hip_runtime_api.h>

#include "ptmi.h"

extern "C" {
void hipstub_fail(int kind, long k);
long hipstub_calls(int kind);
}

#define CHECK(cond)                                                                              \
    do {                                                                                         \
        if (!(cond)) { std::fprintf(stderr, "FAILED line %d: %s\n", __LINE__, #cond); std::exit(1); } \
    } while (0)

namespace {

constexpr uint32_t kSentinel = 0x7FC0DEADu;
constexpr int kMaxK = PTMI_MULTI_HIT_MAX;

struct Buffers {
    int n, m;
    std::vector<float> rays, t_max;
    std::vector<int32_t> index;
    std::vector<uint32_t> t, idx, count;       // one word of slack in front: `+ 1` is a row array 4 bytes off
    Buffers(int n_, int m_) : n(n_), m(m_), rays(6 * (size_t)n_, 0.25f), t_max((size_t)n_, 5.0f), index((size_t)m_), t((size_t)n_ * kMaxK + 4),
                              idx((size_t)n_ * kMaxK + 4), count((size_t)n_ + 4)
    {
        for (int k = 0; k < m; ++k) index[(size_t)k] = k % 9 == 4 ? -1 - k : (k * 7) % n;
        fill();
    }
    void fill() { for (auto *v : {&t, &idx, &count}) for (auto &w : *v) w = kSentinel; }
    bool untouched() const
    {
        for (auto *v : {&t, &idx, &count}) for (auto w : *v) if (w != kSentinel) return false;
        return true;
    }
};

enum Kind { kLinear, kBvh, kMesh };

int set_scene(ptmi_ctx *c, Kind kind)
{
    std::vector<ptmi_sphere> s(kind == kLinear ? 12u : 300u);
    for (size_t i = 0; i < s.size(); ++i) {
        ptmi_sphere &x = s[i];
        std::memset(&x, 0, sizeof x);
        x.position[0] = 0.37f * (float)(i % 17); x.position[1] = 0.11f * (float)(i % 29); x.position[2] = -6.0f - 0.05f * (float)i;
        x.radius = 0.1f + 0.01f * (float)(i % 7);
        x.color[0] = x.color[1] = x.color[2] = 0.5f;
        x.brdf_tag = PTMI_MATTE; x.brdf_param = 0.8f;
    }
    ptmi_plane plane;
    std::memset(&plane, 0, sizeof plane);
    plane.position[1] = -3.0f; plane.direction[1] = 1.0f; plane.color[0] = 0.5f; plane.brdf_tag = PTMI_MATTE; plane.brdf_param = 1.0f;
    ptmi_triangle tri[2];
    std::memset(tri, 0, sizeof tri);
    for (int k = 0; k < 2; ++k) {
        tri[k].v1[0] = 1.0f + (float)k; tri[k].v2[1] = 1.0f; tri[k].v0[2] = tri[k].v1[2] = tri[k].v2[2] = -9.0f;
        tri[k].brdf_tag = PTMI_MATTE; tri[k].brdf_param = 1.0f;
    }
    if (kind == kMesh) return ptmi_set_scene_mesh(c, s.data(), (int)s.size(), tri, 2, &plane, 1);
    if (kind == kBvh) return ptmi_set_scene_bvh(c, s.data(), (int)s.size(), &plane, 1);
    return ptmi_set_scene(c, s.data(), (int)s.size(), &plane, 1);
}

// every runtime call of `call` failing in turn: PTMI_EHIP (or PTMI_ENOMEM), a message, nothing written.  Returns the failures injected.
template <class F> int walk_failures(ptmi_ctx *c, Buffers &b, F &&call)
{
    int injected = 0;
    for (int kind = 0; kind < 4; ++kind)
        for (long k = 1;; ++k) {
            b.fill();
            hipstub_fail(kind, k);
            const long calls = hipstub_calls(kind);
            const int rc = call();
            const bool hit = hipstub_calls(kind) - calls >= k;
            hipstub_fail(kind, 0);
            if (!hit) { CHECK(rc == PTMI_OK); break; }
            if (rc == PTMI_OK) continue;                   // (a failure the library may absorb)
            CHECK(rc == PTMI_EHIP || rc == PTMI_ENOMEM);
            CHECK(ptmi_last_error(c) && *ptmi_last_error(c));
            CHECK(b.untouched());                          // (kernels do not run on the stand-in: only the host side could have written)
            ++injected;
        }
    return injected;
}

int scenario(Kind kind)
{
    ptmi_ctx *c = nullptr;
    CHECK(ptmi_create(&c, 0) == PTMI_OK);
    Buffers b(130, 70);
    const int n = b.n, m = b.m, k = 4;
    const float *rays = b.rays.data(), *tm = b.t_max.data();
    const int32_t *index = b.index.data();
    float *t = reinterpret_cast<float *>(b.t.data());
    int32_t *idx = reinterpret_cast<int32_t *>(b.idx.data()), *cnt = reinterpret_cast<int32_t *>(b.count.data());
    auto P = [&](const float *r, const float *lim, int count, int kk, float *to, int32_t *io, int32_t *co) {
        return ptmi_trace_rays_multi_device(c, r, lim, count, kk, to, io, co);
    };
    auto X = [&](const float *r, const float *lim, int count, const int32_t *ix, int entries, int kk, float *to, int32_t *io, int32_t *co) {
        return ptmi_trace_rays_multi_indexed_device(c, r, lim, count, ix, entries, kk, to, io, co);
    };

    // before any scene
    CHECK(ptmi_trace_rays_multi_device(nullptr, rays, tm, n, k, t, idx, cnt) == PTMI_EINVAL);
    CHECK(ptmi_trace_rays_multi_indexed_device(nullptr, rays, tm, n, index, m, k, t, idx, cnt) == PTMI_EINVAL);
    CHECK(P(rays, tm, n, k, t, idx, cnt) == PTMI_ESTATE && X(rays, tm, n, index, m, k, t, idx, cnt) == PTMI_ESTATE);
    CHECK(P(rays, tm, -1, k, t, idx, cnt) == PTMI_EINVAL);                              // (the arguments are looked at first)
    CHECK(P(rays, tm, n, kMaxK + 1, t, idx, cnt) == PTMI_ELIMIT);

    CHECK(set_scene(c, kind) == PTMI_OK);
    const long launches = hipstub_calls(2);
    // every refusal
    CHECK(P(nullptr, tm, n, k, t, idx, cnt) == PTMI_EINVAL && std::strstr(ptmi_last_error(c), "multi-hit"));
    CHECK(P(rays, tm, n, k, nullptr, idx, cnt) == PTMI_EINVAL && P(rays, tm, n, k, t, nullptr, cnt) == PTMI_EINVAL && P(rays, tm, n, k, t, idx, nullptr) == PTMI_EINVAL);
    CHECK(P(rays, tm, -1, k, t, idx, cnt) == PTMI_EINVAL && P(rays, tm, INT_MIN, k, t, idx, cnt) == PTMI_EINVAL);
    CHECK(P(rays, tm, n, 0, t, idx, cnt) == PTMI_EINVAL && P(rays, tm, n, -1, t, idx, cnt) == PTMI_EINVAL && P(rays, tm, n, INT_MIN, t, idx, cnt) == PTMI_EINVAL);
    CHECK(P(rays, tm, n, kMaxK + 1, t, idx, cnt) == PTMI_ELIMIT && P(rays, tm, n, INT_MAX, t, idx, cnt) == PTMI_ELIMIT);
    CHECK(std::strstr(ptmi_last_error(c), "PTMI_MULTI_HIT_MAX"));
    CHECK(P(nullptr, nullptr, 0, 0, nullptr, nullptr, nullptr) == PTMI_EINVAL);        // k < 1 is refused whatever n
    CHECK(X(nullptr, tm, n, index, m, k, t, idx, cnt) == PTMI_EINVAL && X(rays, tm, n, index, m, k, nullptr, idx, cnt) == PTMI_EINVAL);
    CHECK(X(rays, tm, n, index, m, k, t, nullptr, cnt) == PTMI_EINVAL && X(rays, tm, n, index, m, k, t, idx, nullptr) == PTMI_EINVAL);
    CHECK(X(rays, tm, -1, index, m, k, t, idx, cnt) == PTMI_EINVAL && X(rays, tm, n, index, -1, k, t, idx, cnt) == PTMI_EINVAL);
    CHECK(X(rays, tm, n, nullptr, m, k, t, idx, cnt) == PTMI_EINVAL && X(rays, tm, n, index, INT_MIN, k, t, idx, cnt) == PTMI_EINVAL);
    CHECK(X(rays, tm, n, index, m, 0, t, idx, cnt) == PTMI_EINVAL && X(rays, tm, n, index, m, kMaxK + 1, t, idx, cnt) == PTMI_ELIMIT);
    // nothing to do
    CHECK(P(nullptr, nullptr, 0, k, nullptr, nullptr, nullptr) == PTMI_OK);
    CHECK(X(rays, tm, n, nullptr, 0, k, t, idx, cnt) == PTMI_OK && X(nullptr, nullptr, 0, index, m, k, nullptr, nullptr, nullptr) == PTMI_OK);
    CHECK(hipstub_calls(2) == launches);                                               // nothing was enqueued by any of these
    CHECK(b.untouched());
    // every k, with and without t_max, rows aligned and 4 bytes off, the largest counts
    for (int kk = 1; kk <= kMaxK; ++kk) {
        CHECK(P(rays, kk % 2 ? tm : nullptr, n, kk, t, idx, cnt) == PTMI_OK);
        CHECK(P(rays, tm, n - 1, kk, t + 1, idx + 1, cnt + 1) == PTMI_OK);
        CHECK(X(rays, nullptr, n, index, m, kk, t + 1, idx, cnt) == PTMI_OK);
    }
    CHECK(hipstub_calls(2) == launches + 3 * kMaxK);
    CHECK(X(rays, tm, INT_MAX, index, m, k, t, idx, cnt) == PTMI_OK);                   // lanes is m with an index
    CHECK(b.untouched());                                                              // (kernels do not run on the stand-in)

    int injected = walk_failures(c, b, [&] { return P(rays, tm, n, k, t, idx, cnt); });
    injected += walk_failures(c, b, [&] { return P(rays, nullptr, n, kMaxK, t, idx, cnt); });
    injected += walk_failures(c, b, [&] { return X(rays, tm, n, index, m, 5, t, idx, cnt); });
    ptmi_destroy(c);
    return injected;
}

}  // namespace

int main()
{
    int injected = 0;
    for (Kind kind : {kLinear, kBvh, kMesh}) injected += scenario(kind);
    CHECK(injected >= 6);
    std::printf("MULTI_HIT_HOSTSAN_OK %d failures injected\n", injected);
    return 0;
}
