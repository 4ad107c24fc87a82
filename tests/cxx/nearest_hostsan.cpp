// nearest_hostsan.cpp -- the host side of the nearest-primitive query (csrc/ptmi_nearest.cpp and the launcher of csrc/ptmi_nearest.hip) under
// AddressSanitizer + UBSan, as a stand-alone program: linked against the library built with its host code instrumented and against the
// HIP stand-in (tests/cxx/hip_stub.cpp: device memory is host memory, kernels do not run), run directly by
// tests/test_nearest_host_sanitized.py.  It provokes every refusal of ptmi_nearest_device and ptmi_nearest_indexed_device on a linear, a BVH
// and a mesh scene, calls both with and without r_max and locations on aligned and misaligned arrays, lets every runtime call of the two
// entries fail in turn (no refused or failed call writes to an output), and runs the host twin, ptmi_nearest: its refusals, its answers on
// a scene whose answers are known, non-finite points, every family of r_max, and enough work for its worker threads.
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
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

struct Buffers {
    int n, m;
    std::vector<float> points, r_max;
    std::vector<int32_t> index;
    std::vector<uint32_t> dist, idx, at;       // one word of slack in front: `+ 1` is an array 4 bytes off
    Buffers(int n_, int m_) : n(n_), m(m_), points(3 * (size_t)n_ + 4, 0.25f), r_max((size_t)n_ + 4, 5.0f), index((size_t)m_), dist((size_t)n_ + 4),
                              idx((size_t)n_ + 4), at(3 * (size_t)n_ + 4)
    {
        for (int k = 0; k < m; ++k) index[(size_t)k] = k % 9 == 4 ? -1 - k : (k * 7) % n;
        fill();
    }
    void fill() { for (auto *v : {&dist, &idx, &at}) for (auto &w : *v) w = kSentinel; }
    bool untouched() const
    {
        for (auto *v : {&dist, &idx, &at}) for (auto w : *v) if (w != kSentinel) return false;
        return true;
    }
};

enum Kind { kLinear, kBvh, kMesh };

void make_scene(Kind kind, std::vector<ptmi_sphere> &s, ptmi_plane &plane, ptmi_triangle tri[2])
{
    s.resize(kind == kLinear ? 12u : 300u);
    for (size_t i = 0; i < s.size(); ++i) {
        ptmi_sphere &x = s[i];
        std::memset(&x, 0, sizeof x);
        x.position[0] = 0.37f * (float)(i % 17); x.position[1] = 0.11f * (float)(i % 29); x.position[2] = -6.0f - 0.05f * (float)i;
        x.radius = 0.1f + 0.01f * (float)(i % 7);
        x.color[0] = x.color[1] = x.color[2] = 0.5f;
        x.brdf_tag = PTMI_MATTE; x.brdf_param = 0.8f;
    }
    std::memset(&plane, 0, sizeof plane);
    plane.position[1] = -3.0f; plane.direction[1] = 1.0f; plane.color[0] = 0.5f; plane.brdf_tag = PTMI_MATTE; plane.brdf_param = 1.0f;
    std::memset(tri, 0, 2 * sizeof tri[0]);
    for (int k = 0; k < 2; ++k) {
        tri[k].v1[0] = 1.0f + (float)k; tri[k].v2[1] = 1.0f; tri[k].v0[2] = tri[k].v1[2] = tri[k].v2[2] = -9.0f;
        tri[k].brdf_tag = PTMI_MATTE; tri[k].brdf_param = 1.0f;
    }
}

int set_scene(ptmi_ctx *c, Kind kind)
{
    std::vector<ptmi_sphere> s;
    ptmi_plane plane;
    ptmi_triangle tri[2];
    make_scene(kind, s, plane, tri);
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
    const int n = b.n, m = b.m;
    const float *pts = b.points.data(), *rm = b.r_max.data();
    const int32_t *index = b.index.data();
    float *dist = reinterpret_cast<float *>(b.dist.data()), *at = reinterpret_cast<float *>(b.at.data());
    int32_t *idx = reinterpret_cast<int32_t *>(b.idx.data());
    auto P = [&](const float *p, const float *lim, int count, float *d, int32_t *i, float *a) { return ptmi_nearest_device(c, p, lim, count, d, i, a); };
    auto X = [&](const float *p, const float *lim, int count, const int32_t *ix, int entries, float *d, int32_t *i, float *a) {
        return ptmi_nearest_indexed_device(c, p, lim, count, ix, entries, d, i, a);
    };

    // before any scene
    CHECK(ptmi_nearest_device(nullptr, pts, rm, n, dist, idx, at) == PTMI_EINVAL);
    CHECK(ptmi_nearest_indexed_device(nullptr, pts, rm, n, index, m, dist, idx, at) == PTMI_EINVAL);
    CHECK(P(pts, rm, n, dist, idx, at) == PTMI_ESTATE && X(pts, rm, n, index, m, dist, idx, at) == PTMI_ESTATE);
    CHECK(P(pts, rm, -1, dist, idx, at) == PTMI_EINVAL);                                // (the arguments are looked at first)

    CHECK(set_scene(c, kind) == PTMI_OK);
    const long launches = hipstub_calls(2);
    // every refusal
    CHECK(P(nullptr, rm, n, dist, idx, at) == PTMI_EINVAL && std::strstr(ptmi_last_error(c), "nearest"));
    CHECK(P(pts, rm, n, nullptr, idx, at) == PTMI_EINVAL && P(pts, rm, n, dist, nullptr, at) == PTMI_EINVAL);
    CHECK(P(pts, rm, -1, dist, idx, at) == PTMI_EINVAL && P(pts, rm, INT_MIN, dist, idx, at) == PTMI_EINVAL);
    CHECK(X(nullptr, rm, n, index, m, dist, idx, at) == PTMI_EINVAL && X(pts, rm, n, index, m, nullptr, idx, at) == PTMI_EINVAL);
    CHECK(X(pts, rm, n, index, m, dist, nullptr, at) == PTMI_EINVAL);
    CHECK(X(pts, rm, -1, index, m, dist, idx, at) == PTMI_EINVAL && X(pts, rm, n, index, -1, dist, idx, at) == PTMI_EINVAL);
    CHECK(X(pts, rm, n, nullptr, m, dist, idx, at) == PTMI_EINVAL && X(pts, rm, n, index, INT_MIN, dist, idx, at) == PTMI_EINVAL);
    // nothing to do
    CHECK(P(nullptr, nullptr, 0, nullptr, nullptr, nullptr) == PTMI_OK);
    CHECK(X(pts, rm, n, nullptr, 0, dist, idx, at) == PTMI_OK && X(nullptr, nullptr, 0, index, m, nullptr, nullptr, nullptr) == PTMI_OK);
    CHECK(hipstub_calls(2) == launches);                                               // nothing was enqueued by any of these
    CHECK(b.untouched());
    // with and without r_max and locations, arrays aligned and 4 bytes off, the largest counts
    CHECK(P(pts, rm, n, dist, idx, at) == PTMI_OK && P(pts, nullptr, n, dist, idx, nullptr) == PTMI_OK);
    CHECK(P(pts + 1, rm + 1, n - 1, dist + 1, idx + 1, at + 1) == PTMI_OK);
    CHECK(X(pts, nullptr, n, index, m, dist + 1, idx, at) == PTMI_OK && X(pts, rm, n, index, m, dist, idx, nullptr) == PTMI_OK);
    CHECK(hipstub_calls(2) == launches + 5);
    CHECK(X(pts, rm, INT_MAX, index, m, dist, idx, at) == PTMI_OK);                     // lanes is m with an index
    CHECK(b.untouched());                                                              // (kernels do not run on the stand-in)

    int injected = walk_failures(c, b, [&] { return P(pts, rm, n, dist, idx, at); });
    injected += walk_failures(c, b, [&] { return P(pts, nullptr, n, dist, idx, nullptr); });
    injected += walk_failures(c, b, [&] { return X(pts, rm, n, index, m, dist, idx, at); });
    ptmi_destroy(c);
    return injected;
}

// The host twin: no context, no device
void twin()
{
    std::vector<ptmi_sphere> s;
    ptmi_plane plane;
    ptmi_triangle tri[2];
    make_scene(kMesh, s, plane, tri);
    const int ns = (int)s.size();
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    float pts[7][3] = {{0.25f, 0.25f, -8.0f}, {0.0f, -2.5f, -100.0f}, {nan, 0.0f, 0.0f}, {0.0f, inf, 0.0f}, {0.25f, 0.25f, -8.0f}, {0.25f, 0.25f, -8.0f}, {0.25f, 0.25f, -8.0f}};
    float lim[7] = {inf, 100.0f, 1.0f, 1.0f, 0.5f, nan, -1.0f};
    float dist[7], at[7][3];
    int32_t idx[7];
    CHECK(ptmi_nearest(s.data(), ns, &plane, 1, tri, 2, &pts[0][0], lim, 7, dist, idx, &at[0][0]) == PTMI_OK);
    // (0.25, 0.25, -8) is one unit in front of triangle 0 (z = -9, facing +z) -- and nearer to some sphere of the field or not: whichever, under
    // r_max 0.5 the triangle no longer qualifies, and a NaN or negative r_max is a miss
    CHECK(idx[0] >= 0 && std::fabs(dist[0]) <= 1.0f);
    CHECK(idx[1] == ns && dist[1] == 0.5f && at[1][0] == 0.0f && at[1][1] == -3.0f && at[1][2] == -100.0f);      // the plane below
    CHECK(idx[2] == -1 && idx[3] == -1 && dist[2] == 0.0f && at[3][1] == 0.0f);
    CHECK(idx[4] == -1 || std::fabs(dist[4]) < 0.5f);
    CHECK(idx[5] == -1 && idx[6] == -1 && dist[5] == 0.0f && dist[6] == 0.0f);
    // the triangles alone: the first wins the tie with nothing, the foot is the location
    CHECK(ptmi_nearest(nullptr, 0, nullptr, 0, tri, 2, &pts[0][0], nullptr, 1, dist, idx, &at[0][0]) == PTMI_OK);
    CHECK(idx[0] == 0 && dist[0] == 1.0f && at[0][0] == 0.25f && at[0][1] == 0.25f && at[0][2] == -9.0f);
    CHECK(ptmi_nearest(nullptr, 0, nullptr, 0, tri, 2, &pts[0][0], nullptr, 1, dist, idx, nullptr) == PTMI_OK);  // point may be NULL
    // refusals: counts, pointers, an empty scene; with triangles what ptmi_set_scene_mesh refuses in the geometry
    CHECK(ptmi_nearest(s.data(), -1, &plane, 1, tri, 2, &pts[0][0], lim, 7, dist, idx, nullptr) == PTMI_EINVAL);
    CHECK(ptmi_nearest(nullptr, ns, &plane, 1, tri, 2, &pts[0][0], lim, 7, dist, idx, nullptr) == PTMI_EINVAL);
    CHECK(ptmi_nearest(s.data(), ns, nullptr, 1, tri, 2, &pts[0][0], lim, 7, dist, idx, nullptr) == PTMI_EINVAL);
    CHECK(ptmi_nearest(s.data(), ns, &plane, 1, nullptr, 2, &pts[0][0], lim, 7, dist, idx, nullptr) == PTMI_EINVAL);
    CHECK(ptmi_nearest(nullptr, 0, nullptr, 0, nullptr, 0, &pts[0][0], lim, 7, dist, idx, nullptr) == PTMI_EINVAL);
    CHECK(ptmi_nearest(s.data(), ns, &plane, 1, tri, 2, nullptr, lim, 7, dist, idx, nullptr) == PTMI_EINVAL);
    CHECK(ptmi_nearest(s.data(), ns, &plane, 1, tri, 2, &pts[0][0], lim, 7, nullptr, idx, nullptr) == PTMI_EINVAL);
    CHECK(ptmi_nearest(s.data(), ns, &plane, 1, tri, 2, &pts[0][0], lim, 7, dist, nullptr, nullptr) == PTMI_EINVAL);
    CHECK(ptmi_nearest(s.data(), ns, &plane, 1, tri, 2, &pts[0][0], lim, -1, dist, idx, nullptr) == PTMI_EINVAL);
    CHECK(ptmi_nearest(s.data(), ns, &plane, 1, tri, 2, nullptr, nullptr, 0, nullptr, nullptr, nullptr) == PTMI_OK);
    ptmi_triangle bad[2] = {tri[0], tri[1]};
    bad[1].v2[0] = nan;
    CHECK(ptmi_nearest(s.data(), ns, &plane, 1, bad, 2, &pts[0][0], lim, 7, dist, idx, nullptr) == PTMI_EINVAL);
    std::vector<ptmi_sphere> s2 = s;
    s2[5].radius = inf;
    CHECK(ptmi_nearest(s2.data(), ns, &plane, 1, tri, 2, &pts[0][0], lim, 7, dist, idx, nullptr) == PTMI_EINVAL);
    CHECK(ptmi_nearest(s2.data(), ns, &plane, 1, nullptr, 0, &pts[0][0], lim, 7, dist, idx, nullptr) == PTMI_OK);   // a linear scene takes it
    CHECK(idx[1] == ns);
    // enough work for the worker threads: 16 384 points x 303 primitives; every answer is what one call per point gives
    const int big = 16384;
    std::vector<float> p((size_t)big * 3), d((size_t)big), a((size_t)big * 3);
    std::vector<int32_t> ix((size_t)big);
    for (int i = 0; i < big; ++i) { p[3 * (size_t)i] = 0.001f * (float)(i % 5000); p[3 * (size_t)i + 1] = 0.5f; p[3 * (size_t)i + 2] = -6.0f - 0.001f * (float)i; }
    CHECK(ptmi_nearest(s.data(), ns, &plane, 1, tri, 2, p.data(), nullptr, big, d.data(), ix.data(), a.data()) == PTMI_OK);
    for (int i = 0; i < big; i += 997) {
        float d1, a1[3];
        int32_t i1;
        CHECK(ptmi_nearest(s.data(), ns, &plane, 1, tri, 2, &p[3 * (size_t)i], nullptr, 1, &d1, &i1, a1) == PTMI_OK);
        CHECK(std::memcmp(&d1, &d[(size_t)i], 4) == 0 && i1 == ix[(size_t)i] && std::memcmp(a1, &a[3 * (size_t)i], 12) == 0);
    }
}

}  // namespace

int main()
{
    int injected = 0;
    for (Kind kind : {kLinear, kBvh, kMesh}) injected += scenario(kind);
    CHECK(injected >= 6);
    twin();
    std::printf("NEAREST_HOSTSAN_OK %d failures injected\n", injected);
    return 0;
}
