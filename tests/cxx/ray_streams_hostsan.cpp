// ray_streams_hostsan.cpp -- the host side of render Streams along a caller's rays (csrc/ptmi_trace_streams.cpp and the launcher of
// csrc/ptmi_trace_streams.hip) under AddressSanitizer + UBSan, as a stand-alone program: linked against the library built with its host
// code instrumented and against the HIP stand-in (tests/cxx/hip_stub.cpp: device memory is host memory, kernels do not run), run directly
// by tests/test_ray_streams_host_sanitized.py.  It provokes every refusal of ptmi_trace_streams_device and
// ptmi_trace_streams_indexed_device on a linear, a BVH and a mesh scene with and without GLASS, checks the workspace arithmetic up to a
// count of INT_MAX, and lets every runtime call of the two entries fail in turn; no refused or failed call writes to an output.
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

std::vector<ptmi_sphere> spheres_of(int n, bool glass)
{
    std::vector<ptmi_sphere> s((size_t)n);
    for (int i = 0; i < n; ++i) {
        ptmi_sphere &x = s[(size_t)i];
        std::memset(&x, 0, sizeof x);
        x.position[0] = 0.37f * (float)(i % 17); x.position[1] = 0.11f * (float)(i % 29); x.position[2] = -6.0f - 0.05f * (float)i;
        x.radius = 0.1f + 0.01f * (float)(i % 7);
        x.color[0] = x.color[1] = x.color[2] = 0.5f;
        x.brdf_tag = PTMI_MATTE; x.brdf_param = 0.8f;
        if (glass && i % 5 == 2) { x.brdf_tag = PTMI_GLASS; x.brdf_param = 1.5f; }
    }
    return s;
}

struct Buffers {
    int n, m;
    std::vector<float> rays, color;
    std::vector<uint32_t> seed;
    std::vector<int32_t> index;
    std::vector<uint64_t> lost;                // (8-byte aligned by its element type)
    void *work = nullptr;                      // 16-byte aligned
    size_t work_bytes = 0;
    Buffers(int n_, int m_) : n(n_), m(m_), rays(6 * (size_t)n_, 0.25f), color(3 * (size_t)n_), seed(4 * (size_t)n_), index((size_t)m_), lost(2)
    {
        for (int k = 0; k < m; ++k) index[(size_t)k] = (k * 7) % n;
        work_bytes = ptmi_trace_streams_bytes(n > m ? n : m);
        CHECK(posix_memalign(&work, 16, work_bytes) == 0);
        fill();
    }
    ~Buffers() { std::free(work); }
    void fill()
    {
        uint32_t *c = reinterpret_cast<uint32_t *>(color.data());
        for (size_t k = 0; k < color.size(); ++k) c[k] = kSentinel;
        for (auto &w : seed) w = kSentinel;
        lost[0] = lost[1] = 0x7FC0DEAD7FC0DEADull;
        std::memset(work, 0x5A, work_bytes);
    }
    bool untouched() const
    {
        const uint32_t *c = reinterpret_cast<const uint32_t *>(color.data());
        for (size_t k = 0; k < color.size(); ++k) if (c[k] != kSentinel) return false;
        for (auto w : seed) if (w != kSentinel) return false;
        if (lost[0] != 0x7FC0DEAD7FC0DEADull || lost[1] != lost[0]) return false;
        const unsigned char *w = static_cast<const unsigned char *>(work);
        for (size_t k = 0; k < work_bytes; ++k) if (w[k] != 0x5A) return false;
        return true;
    }
};

void workspace_arithmetic()
{
    const size_t per_wave = 4u * 64u * 64u;                // kTreeFastLevels records of 64 bytes for each of a wave's 64 lanes
    CHECK(ptmi_trace_streams_bytes(0) == 0 && ptmi_trace_streams_bytes(-1) == 0 && ptmi_trace_streams_bytes(INT_MIN) == 0);
    CHECK(ptmi_trace_streams_bytes(1) == per_wave && ptmi_trace_streams_bytes(64) == per_wave && ptmi_trace_streams_bytes(65) == 2 * per_wave);
    CHECK(ptmi_trace_streams_bytes(1 << 22) == ((size_t)1 << 16) * per_wave);
    CHECK(ptmi_trace_streams_bytes(INT_MAX - 63) == (((size_t)1 << 25) - 1) * per_wave);
    CHECK(ptmi_trace_streams_bytes(INT_MAX - 62) == (((size_t)1 << 25)) * per_wave);
    CHECK(ptmi_trace_streams_bytes(INT_MAX) == ((size_t)1 << 25) * per_wave);     // (2^31 - 1 + 63) / 64 = 2^25, in 64 bits
    for (int count = 1; count < 1000; count += 37) CHECK(ptmi_trace_streams_bytes(count) == (size_t)((count + 63) / 64) * per_wave);
}

enum Kind { kLinear, kBvh, kMesh };

int set_scene(ptmi_ctx *c, Kind kind, bool glass)
{
    const std::vector<ptmi_sphere> s = spheres_of(kind == kLinear ? 12 : 300, glass);
    ptmi_plane plane;
    std::memset(&plane, 0, sizeof plane);
    plane.position[1] = -3.0f; plane.direction[1] = 1.0f; plane.color[0] = 0.5f; plane.brdf_tag = PTMI_MATTE; plane.brdf_param = 1.0f;
    ptmi_triangle tri[2];
    std::memset(tri, 0, sizeof tri);
    for (int k = 0; k < 2; ++k) {
        tri[k].v1[0] = 1.0f + (float)k; tri[k].v2[1] = 1.0f; tri[k].v0[2] = tri[k].v1[2] = tri[k].v2[2] = -9.0f;
        tri[k].brdf_tag = glass && k == 1 ? PTMI_GLASS : PTMI_MATTE; tri[k].brdf_param = glass && k == 1 ? 1.5f : 1.0f;
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
    const int n = b.n, m = b.m;
    float *rays = b.rays.data(), *col = b.color.data();
    uint32_t *sd = b.seed.data();
    int32_t *index = b.index.data();
    uint64_t *lost = b.lost.data();
    void *odd_lost = reinterpret_cast<char *>(lost) + 4, *odd_work = static_cast<char *>(b.work) + 8;
    auto P = [&](const float *r, int count, int spp, float *cl, uint32_t *s, void *l, void *w, size_t bytes) {
        return ptmi_trace_streams_device(c, r, count, spp, cl, s, static_cast<uint64_t *>(l), w, bytes);
    };
    auto X = [&](const float *r, int count, const int32_t *ix, int entries, int spp, float *cl, uint32_t *s, void *l, void *w, size_t bytes) {
        return ptmi_trace_streams_indexed_device(c, r, count, ix, entries, spp, cl, s, static_cast<uint64_t *>(l), w, bytes);
    };

    // before any scene
    CHECK(ptmi_trace_streams_device(nullptr, rays, n, 1, col, sd, lost, b.work, b.work_bytes) == PTMI_EINVAL);
    CHECK(P(rays, n, 1, col, sd, lost, b.work, b.work_bytes) == PTMI_ESTATE);
    CHECK(X(rays, n, index, m, 1, col, sd, lost, b.work, b.work_bytes) == PTMI_ESTATE);
    CHECK(P(rays, -1, 1, col, sd, lost, b.work, b.work_bytes) == PTMI_EINVAL);          // (the arguments are looked at first)

    // a scene with GLASS: every refusal
    CHECK(set_scene(c, kind, true) == PTMI_OK);
    CHECK(P(nullptr, n, 1, col, sd, lost, b.work, b.work_bytes) == PTMI_EINVAL);
    CHECK(P(rays, n, 1, nullptr, sd, lost, b.work, b.work_bytes) == PTMI_EINVAL);
    CHECK(P(rays, n, 1, col, nullptr, lost, b.work, b.work_bytes) == PTMI_EINVAL);
    CHECK(P(rays, -1, 1, col, sd, lost, b.work, b.work_bytes) == PTMI_EINVAL);
    CHECK(P(rays, INT_MIN, 1, col, sd, lost, b.work, b.work_bytes) == PTMI_EINVAL);
    CHECK(P(rays, n, 1, col, sd, odd_lost, b.work, b.work_bytes) == PTMI_EINVAL && std::strstr(ptmi_last_error(c), "d_lost"));
    CHECK(P(rays, n, 1, col, sd, lost, nullptr, b.work_bytes) == PTMI_EINVAL);
    CHECK(P(rays, n, 1, col, sd, lost, odd_work, b.work_bytes) == PTMI_EINVAL && std::strstr(ptmi_last_error(c), "16-byte"));
    CHECK(P(rays, n, 1, col, sd, lost, b.work, ptmi_trace_streams_bytes(n) - 1) == PTMI_EINVAL && std::strstr(ptmi_last_error(c), "ptmi_trace_streams_bytes"));
    CHECK(P(rays, n, 1, col, sd, lost, b.work, 0) == PTMI_EINVAL);
    CHECK(P(rays, INT_MAX, 1, col, sd, lost, b.work, b.work_bytes) == PTMI_EINVAL);     // (the workspace of 2^31 - 1 lanes is 512 GB: short)
    CHECK(X(nullptr, n, index, m, 1, col, sd, lost, b.work, b.work_bytes) == PTMI_EINVAL);
    CHECK(X(rays, n, index, m, 1, nullptr, sd, lost, b.work, b.work_bytes) == PTMI_EINVAL);
    CHECK(X(rays, n, index, m, 1, col, nullptr, lost, b.work, b.work_bytes) == PTMI_EINVAL);
    CHECK(X(rays, -1, index, m, 1, col, sd, lost, b.work, b.work_bytes) == PTMI_EINVAL);
    CHECK(X(rays, n, index, -1, 1, col, sd, lost, b.work, b.work_bytes) == PTMI_EINVAL);
    CHECK(X(rays, n, nullptr, m, 1, col, sd, lost, b.work, b.work_bytes) == PTMI_EINVAL);
    CHECK(X(rays, n, index, m, 1, col, sd, odd_lost, b.work, b.work_bytes) == PTMI_EINVAL);
    CHECK(X(rays, n, index, m, 1, col, sd, lost, nullptr, 0) == PTMI_EINVAL);
    CHECK(X(rays, n, index, m, 1, col, sd, lost, b.work, ptmi_trace_streams_bytes(m) - 1) == PTMI_EINVAL);
    CHECK(X(rays, n, index, INT_MAX, 1, col, sd, lost, b.work, b.work_bytes) == PTMI_EINVAL);
    CHECK(b.untouched());
    // nothing to do
    const long launches = hipstub_calls(2);
    CHECK(P(nullptr, 0, 1, nullptr, nullptr, nullptr, nullptr, 0) == PTMI_OK && P(rays, n, 0, col, sd, lost, b.work, b.work_bytes) == PTMI_OK);
    CHECK(P(rays, n, -3, col, sd, lost, b.work, b.work_bytes) == PTMI_OK);
    CHECK(X(rays, n, nullptr, 0, 1, col, sd, lost, b.work, b.work_bytes) == PTMI_OK && X(nullptr, 0, index, m, 1, nullptr, nullptr, nullptr, nullptr, 0) == PTMI_OK);
    CHECK(b.untouched());
    // lanes is m with an index: a workspace of m lanes serves n > m rays
    CHECK(X(rays, n, index, m, 1, col, sd, lost, b.work, ptmi_trace_streams_bytes(m)) == PTMI_OK);
    CHECK(P(rays, n, 2, col, sd, nullptr, b.work, b.work_bytes) == PTMI_OK);            // d_lost may be NULL
    // GLASS under an explicit PTMI_SEED_FROM_RESULT
    CHECK(ptmi_set_option(c, PTMI_OPT_STREAMS_SEED_RULE, PTMI_SEED_FROM_RESULT) == PTMI_OK);
    CHECK(P(rays, n, 1, col, sd, lost, b.work, b.work_bytes) == PTMI_EINVAL && std::strstr(ptmi_last_error(c), "PTMI_SEED_FROM_RESULT"));
    CHECK(X(rays, n, index, m, 1, col, sd, lost, b.work, b.work_bytes) == PTMI_EINVAL);
    CHECK(b.untouched());
    CHECK(ptmi_set_option(c, PTMI_OPT_STREAMS_SEED_RULE, PTMI_SEED_AUTO) == PTMI_OK);

    // every runtime call of the entries failing in turn, with GLASS and without
    int injected = walk_failures(c, b, [&] { return P(rays, n, 2, col, sd, lost, b.work, b.work_bytes); });
    injected += walk_failures(c, b, [&] { return X(rays, n, index, m, 2, col, sd, lost, b.work, b.work_bytes); });
    CHECK(set_scene(c, kind, false) == PTMI_OK);
    // without GLASS the workspace is ignored: NULL, misaligned, short
    CHECK(P(rays, n, 1, col, sd, lost, nullptr, 0) == PTMI_OK && P(rays, n, 1, col, sd, nullptr, odd_work, 3) == PTMI_OK);
    CHECK(X(rays, n, index, m, 1, col, sd, lost, nullptr, 0) == PTMI_OK);
    CHECK(P(rays, n, 1, col, sd, odd_lost, nullptr, 0) == PTMI_EINVAL);
    for (int rule : {PTMI_SEED_FROM_RESULT, PTMI_SEED_KEEP_ACCUMULATOR}) {
        CHECK(ptmi_set_option(c, PTMI_OPT_STREAMS_SEED_RULE, rule) == PTMI_OK);
        injected += walk_failures(c, b, [&] { return P(rays, n, 2, col, sd, lost, nullptr, 0); });
    }
    CHECK(hipstub_calls(2) > launches);
    ptmi_destroy(c);
    return injected;
}

}  // namespace

int main()
{
    workspace_arithmetic();
    int injected = 0;
    for (Kind kind : {kLinear, kBvh, kMesh}) injected += scenario(kind);
    CHECK(injected >= 6);
    std::printf("RAY_STREAMS_HOSTSAN_OK %d failures injected\n", injected);
    return 0;
}
