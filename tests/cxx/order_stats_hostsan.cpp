// order_stats_hostsan.cpp -- the cost-ordered dispatch (csrc/ptmi_order.cpp), the statistics and the option table of the C ABI under
// AddressSanitizer + UBSan, as a stand-alone program: linked against the library built with its host code instrumented and against the HIP
// stand-in (tests/cxx/hip_stub.cpp: device memory is host memory, kernels do not run), run directly by tests/test_order_stats_host_sanitized.py.
// It uses include/ptmi.h, the stand-in's handles and the layout of RenderArgs (csrc/ptmi_kernels.h) only.
//
//   order_stats_hostsan plain   one fixed scenario; after every ABI call what the call did to the runtime (the calls of every kind, the live
//                               device blocks, the launches and memsets in order), after every render whether the launch was handed the order
//                               and the cost words, after every order kernel its tail arguments; every option's accepted and refused values
//                               with their messages.  The record of the commit BEFORE the order, the statistics and the options got their
//                               owners is tests/golden/order_stats_calls.txt: a refactor leaves it as it is, line for line.
//   order_stats_hostsan walk    the lines of the record that begin "walked:" -- a context's creation, launches 0 to 4 at 64x16 and the
//                               statistics calls -- with the k-th runtime call of every kind failing, for every k.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <string>
#include <vector>

#include <hip/hip_runtime_api.h>

#include "ptmi.h"
#include "ptmi_kernels.h"      // RenderArgs: where quad_order and quad_cost lie in a render kernel's first argument

extern "C" {
void hipstub_fail(int kind, long k);
long hipstub_calls(int kind);
long hipstub_live_blocks(void);
long hipstub_live_host_blocks(void);
long hipstub_live_streams(void);
long hipstub_live_events(void);
long hipstub_launches(const char *name_part);
int hipstub_last_arg(const char *kernel_part, int index, void *dst, unsigned long long bytes);
const char *hipstub_log(void);
void hipstub_clear_log(void);
}

#define CHECK(cond)                                                                              \
    do {                                                                                         \
        if (!(cond)) { std::fprintf(stderr, "FAILED line %d: %s\n", __LINE__, #cond); std::exit(1); } \
    } while (0)

namespace {

constexpr int kKinds = 6;                      // hipMalloc, copies, launches, hipStreamSynchronize, hipHostMalloc, event / stream creation
constexpr int kVariantRows = 4;                // ptmi_set_variant: a wave = 64 consecutive pixels of a row (no tiles, no order)
const char *const kPerPixel = "render_", *const kStreamForm = "streams_pixels_kernel", *const kOrder = "quad_order_kernel";
bool g_plain = true;

ptmi_camera camera(float x = 0.0f)
{
    ptmi_camera cam;
    std::memset(&cam, 0, sizeof cam);
    cam.position[0] = x; cam.position[1] = 1.0f; cam.position[2] = 4.0f; cam.fov = 70;
    return cam;
}

enum Kind { Linear, Bvh, Mesh };
int set_scene(ptmi_ctx *c, Kind kind = Linear)
{
    ptmi_sphere s[2];
    std::memset(s, 0, sizeof s);
    for (int i = 0; i < 2; ++i) {
        s[i].position[0] = -1.0f + 2.0f * (float)i; s[i].position[1] = 1.0f; s[i].position[2] = -3.0f; s[i].radius = 0.9f;
        s[i].color[0] = s[i].color[1] = s[i].color[2] = 0.7f; s[i].brdf_tag = PTMI_MATTE; s[i].brdf_param = 0.8f;
    }
    ptmi_plane p;
    std::memset(&p, 0, sizeof p);
    p.direction[1] = 1.0f; p.color[0] = p.color[1] = p.color[2] = 0.5f; p.illuminance = 1.0f; p.brdf_tag = PTMI_MATTE; p.brdf_param = 1.0f;
    ptmi_triangle t;
    std::memset(&t, 0, sizeof t);
    t.v1[0] = 1.0f; t.v2[1] = 1.0f; t.color[0] = t.color[1] = t.color[2] = 0.6f; t.brdf_tag = PTMI_MATTE; t.brdf_param = 1.0f;
    if (kind == Bvh) return ptmi_set_scene_bvh(c, s, 2, &p, 1);
    if (kind == Mesh) return ptmi_set_scene_mesh(c, s, 2, &t, 1, &p, 1);
    return ptmi_set_scene(c, s, 2, &p, 1);
}

// ---- the record ------------------------------------------------------------------------------------------------------------------
long g_mark[kKinds];
void mark()
{
    for (int k = 0; k < kKinds; ++k) g_mark[k] = hipstub_calls(k);
    hipstub_clear_log();
}
void report(const std::string &what, int rc)
{
    if (!g_plain) return;
    std::printf("%s: rc %d calls", what.c_str(), rc);
    for (int k = 0; k < kKinds; ++k) std::printf(" %ld", hipstub_calls(k) - g_mark[k]);
    std::printf(" live %ld\n", hipstub_live_blocks());
    const std::string log = hipstub_log();
    for (size_t at = 0; at < log.size();) {
        const size_t end = log.find('\n', at);
        std::printf("  %s\n", log.substr(at, end - at).c_str());
        at = end == std::string::npos ? log.size() : end + 1;
    }
}

void check_clean_after_destroy()
{
    CHECK(hipstub_live_blocks() == 0 && hipstub_live_host_blocks() == 0 && hipstub_live_streams() == 0 && hipstub_live_events() == 0);
    CHECK(hipGetLastError() == hipSuccess);
}

// What the stand-in keeps of every launch from now on: the render kernels' RenderArgs and the order kernel's two tail arguments
void watch_arguments()
{
    ptmi::RenderArgs a;
    unsigned int *tail = nullptr; unsigned int permille = 0;
    CHECK(hipstub_last_arg(kPerPixel, 0, &a, sizeof a) == 0 && hipstub_last_arg(kStreamForm, 0, &a, sizeof a) == 0);
    CHECK(hipstub_last_arg(kOrder, 4, &tail, sizeof tail) == 0 && hipstub_last_arg(kOrder, 5, &permille, sizeof permille) == 0);
}

// One render and its record: the runtime calls, whether the launch of `kernel` took the order and the cost words, and what an order kernel took
int render(ptmi_ctx *c, const std::string &what, const ptmi_camera &cam, int algorithm, int limit, int expect = PTMI_OK, const char *kernel = kPerPixel, int spp = 1)
{
    const long orders = hipstub_launches(kOrder), renders = hipstub_launches(kernel);
    mark();
    const int rc = ptmi_render(c, &cam, algorithm, limit, spp);
    report(what, rc);
    CHECK(rc == expect);
    if (rc == PTMI_EHIP) {                                     // (the message of a runtime call that failed begins with the call's source text: only what follows it is recorded)
        const std::string message = ptmi_last_error(c);
        std::printf("  %s\n", message.substr(message.rfind(": ") + 2).c_str());
    } else if (rc != PTMI_OK) std::printf("  %s\n", ptmi_last_error(c));
    if (hipstub_launches(kernel) > renders) {
        ptmi::RenderArgs a;
        CHECK(hipstub_last_arg(kernel, 0, &a, sizeof a) == 1);
        std::printf("  order %s cost %s\n", a.quad_order ? "given" : "null", a.quad_cost ? "given" : "null");
    }
    if (hipstub_launches(kOrder) > orders) {
        unsigned int *tail = nullptr; unsigned int permille = 0;
        CHECK(hipstub_last_arg(kOrder, 4, &tail, sizeof tail) == 1 && hipstub_last_arg(kOrder, 5, &permille, sizeof permille) == 1);
        std::printf("  order kernel: tail_permille %u tail_start %s\n", permille, tail ? "given" : "null");
    }
    return rc;
}
void renders(ptmi_ctx *c, const char *what, int n, const ptmi_camera &cam, int algorithm, int limit, const char *kernel = kPerPixel)
{
    for (int i = 0; i < n; ++i) render(c, std::string(what) + ", launch " + std::to_string(i), cam, algorithm, limit, PTMI_OK, kernel);
}

ptmi_ctx *context(int w, int h, Kind kind = Linear)
{
    ptmi_ctx *c = nullptr;
    CHECK(ptmi_create(&c, 0) == PTMI_OK);
    CHECK(set_scene(c, kind) == PTMI_OK);
    if (w > 0) { CHECK(ptmi_resize(c, w, h) == PTMI_OK); CHECK(ptmi_init_output(c, 3) == PTMI_OK); }
    return c;
}
void resize(ptmi_ctx *c, int w, int h)
{
    mark();
    const int rc = ptmi_resize(c, w, h);
    report("resize to " + std::to_string(w) + "x" + std::to_string(h), rc);
    CHECK(rc == PTMI_OK && ptmi_init_output(c, 4) == PTMI_OK);
}
void finish(ptmi_ctx *c) { ptmi_destroy(c); check_clean_after_destroy(); }

// ---- the dispatch order ----------------------------------------------------------------------------------------------------------
void order_scenario()
{
    const ptmi_camera cam = camera(), other = camera(0.5f);
    ptmi_ctx *c = context(64, 16);
    renders(c, "Inline 64x16", 10, cam, PTMI_INLINE, 8);
    renders(c, "Streams 64x16, per-pixel form", 10, cam, PTMI_STREAMS, 8);
    renders(c, "Inline again: the key changed", 3, cam, PTMI_INLINE, 8);
    renders(c, "another camera", 3, other, PTMI_INLINE, 8);
    CHECK(set_scene(c) == PTMI_OK);
    renders(c, "the same scene committed again", 3, other, PTMI_INLINE, 8);
    renders(c, "another bounce limit", 3, other, PTMI_INLINE, 5);
    renders(c, "Inline, then Streams", 2, other, PTMI_STREAMS, 5);
    renders(c, "back to the first camera", 3, cam, PTMI_INLINE, 8);
    // a launch that fails: launches 0 to 2 have been made, launch 3 records -- the order kernel ran before launch 2, so fail that step's two launches in turn
    renders(c, "a fresh key before the failing launches", 2, other, PTMI_INLINE, 8);
    hipstub_fail(2, 1);
    render(c, "launch 2, its order kernel failing", other, PTMI_INLINE, 8, PTMI_EHIP);
    hipstub_fail(2, 2);
    render(c, "launch 2 again, its render kernel failing", other, PTMI_INLINE, 8, PTMI_EHIP);
    hipstub_fail(2, 0);
    renders(c, "launch 2 a third time, and on", 3, other, PTMI_INLINE, 8);
    // resize: the blocks grow, and do not shrink
    resize(c, 136, 40);
    renders(c, "136x40", 3, other, PTMI_INLINE, 8);
    resize(c, 64, 16);
    renders(c, "64x16 after 136x40", 3, other, PTMI_INLINE, 8);
    // ptmi_render1 with an explicit screen takes no order
    {
        const size_t n = 64 * 16;
        std::vector<float> f(n, 0.25f), fo(3 * n);
        std::vector<uint32_t> u(n, 7u), uo(4 * n);
        std::vector<int64_t> sx(n), sy(n);
        for (size_t i = 0; i < n; ++i) { sx[i] = (int64_t)(i % 64) - 32; sy[i] = (int64_t)(i / 64) - 8; }
        for (int i = 0; i < 2; ++i) {
            const long before = hipstub_launches(kPerPixel);
            mark();
            const int rc = ptmi_render1(c, &other, PTMI_INLINE, 8, 64, 16, sx.data(), sy.data(), f.data(), f.data(), f.data(), u.data(), u.data(), u.data(), u.data(),
                                        fo.data(), fo.data() + n, fo.data() + 2 * n, uo.data(), uo.data() + n, uo.data() + 2 * n, uo.data() + 3 * n);
            report("render1 with an explicit screen, call " + std::to_string(i), rc);
            ptmi::RenderArgs a;
            CHECK(rc == PTMI_OK && hipstub_launches(kPerPixel) == before + 1 && hipstub_last_arg(kPerPixel, 0, &a, sizeof a) == 1);
            std::printf("  order %s cost %s screen %s\n", a.quad_order ? "given" : "null", a.quad_cost ? "given" : "null", a.screen_x ? "given" : "null");
        }
    }
    mark();
    int rc = ptmi_set_variant(c, kVariantRows);
    report("set_variant rows", rc);
    CHECK(rc == PTMI_OK);
    renders(c, "variant rows", 2, other, PTMI_INLINE, 8);
    finish(c);

    for (int odd = 0; odd < 2; ++odd) {                        // below either of tiles_pay_dims' bounds: no order, and none of its blocks
        c = context(odd ? 63 : 64, odd ? 16 : 15);
        renders(c, odd ? "63x16" : "64x15", 2, cam, PTMI_INLINE, 8);
        renders(c, odd ? "63x16 Streams" : "64x15 Streams", 2, cam, PTMI_STREAMS, 8);
        finish(c);
    }

    c = context(0, 0);                                         // a part of 16 rows of a 64x32 image
    mark();
    rc = ptmi_set_partition(c, 8, 2, 1);
    report("set_partition 8 rows, part 1 of 2", rc);
    CHECK(rc == PTMI_OK);
    resize(c, 64, 32);
    renders(c, "part 1 of 2 of 64x32", 3, cam, PTMI_INLINE, 8);
    finish(c);

    c = context(64, 16);                                       // an allocation that fails while the quad blocks grow
    renders(c, "before the growth", 2, cam, PTMI_INLINE, 8);
    resize(c, 136, 40);
    hipstub_fail(0, 2);
    render(c, "136x40, the second quad block's allocation failing", cam, PTMI_INLINE, 8, PTMI_ENOMEM);
    hipstub_fail(0, 0);
    renders(c, "136x40 after the failure", 3, cam, PTMI_INLINE, 8);
    finish(c);

    // the stream form, and its tail
    c = context(64, 32);
    CHECK(ptmi_set_option(c, PTMI_OPT_STREAMS_FORM, PTMI_FORM_STREAM) == PTMI_OK);
    renders(c, "stream form 64x32", 4, cam, PTMI_STREAMS, 8, kStreamForm);
    const int64_t tails[3] = {0, 250, -1};
    for (int i = 0; i < 3; ++i) {
        mark();
        rc = ptmi_set_option(c, PTMI_OPT_STREAM_TAIL, tails[i]);
        report("stream tail " + std::to_string(tails[i]), rc);
        CHECK(rc == PTMI_OK);
        renders(c, "stream form under a new camera", 3, camera(1.0f + (float)i), PTMI_STREAMS, 8, kStreamForm);
    }
    hipstub_fail(2, 3);                                        // launch 3 of this key: no rebuild; its third launch is the persistent kernel's
    render(c, "stream form, the persistent launch failing", camera(3.0f), PTMI_STREAMS, 8, PTMI_EHIP, kStreamForm);
    hipstub_fail(2, 0);
    renders(c, "stream form after the failure", 2, camera(3.0f), PTMI_STREAMS, 8, kStreamForm);
    finish(c);
}

// ---- the statistics --------------------------------------------------------------------------------------------------------------
void print_stats(ptmi_ctx *c, const char *what, uint64_t nominal, uint64_t samples)
{
    ptmi_stats st;
    mark();
    const int rc = ptmi_get_stats(c, &st);
    report(std::string("get_stats ") + what, rc);
    CHECK(rc == PTMI_OK && st.nominal_bounces == nominal && st.samples == samples && st.last_render_ms >= 0.0f);
    std::printf("  stats: live %llu nominal %llu samples %llu iterations %u dropped %llu truncated %llu spilled %llu overflowed %llu\n", (unsigned long long)st.live_bounces,
                (unsigned long long)st.nominal_bounces, (unsigned long long)st.samples, st.stream_iterations, (unsigned long long)st.stream_rays_dropped,
                (unsigned long long)st.stream_rays_truncated, (unsigned long long)st.stream_rays_spilled, (unsigned long long)st.stream_rays_overflowed);
}
void stats_scenario()
{
    const ptmi_camera cam = camera();
    ptmi_ctx *c = context(64, 16);
    print_stats(c, "of a fresh context", 0, 0);
    uint32_t words[300];
    const int capacities[4] = {0, 10, 256, 300};
    for (int capacity : capacities) {
        mark();
        const int rc = ptmi_debug_counters_n(c, words, capacity);
        report("debug_counters_n, capacity " + std::to_string(capacity), rc);
    }
    mark();
    report("debug_counters_n, negative capacity", ptmi_debug_counters_n(c, words, -1));
    std::printf("  %s\n", ptmi_last_error(c));
    mark();
    report("debug_counters", ptmi_debug_counters(c, words));
    render(c, "Inline, 3 spp at limit 8", cam, PTMI_INLINE, 8, PTMI_OK, kPerPixel, 3);
    render(c, "Streams, 2 spp", cam, PTMI_STREAMS, 8, PTMI_OK, kPerPixel, 2);
    print_stats(c, "after two renders", 64ull * 16 * 3 * 8, 64ull * 16 * (3 + 2));
    CHECK(ptmi_set_timing(c, 1) == PTMI_OK);
    print_stats(c, "with timing on, nothing rendered since", 64ull * 16 * 3 * 8, 64ull * 16 * (3 + 2));
    render(c, "Inline with timing on, no sample", cam, PTMI_INLINE, 8, PTMI_OK, kPerPixel, 0);
    render(c, "Inline with timing on, 1 spp at limit 0", cam, PTMI_INLINE, 0);
    print_stats(c, "after a timed render", 64ull * 16 * 3 * 8, 64ull * 16 * (3 + 2 + 1));
    mark();
    int rc = ptmi_reset_stats(c);
    report("reset_stats", rc);
    CHECK(rc == PTMI_OK);
    print_stats(c, "after the reset", 0, 0);
    CHECK(ptmi_set_option(c, PTMI_OPT_STREAMS_FORM, PTMI_FORM_STREAM) == PTMI_OK);
    resize(c, 64, 32);
    render(c, "stream form, 4 spp", cam, PTMI_STREAMS, 8, PTMI_OK, kStreamForm, 4);
    print_stats(c, "after a stream-form render", 0, 64ull * 32 * 4);
    mark();
    rc = ptmi_reset_stats(c);
    report("reset_stats after the stream form", rc);
    print_stats(c, "after the second reset", 0, 0);
    mark();
    report("get_stats without a result", ptmi_get_stats(c, nullptr));
    std::printf("  %s\n", ptmi_last_error(c));
    finish(c);
}

// ---- the options -----------------------------------------------------------------------------------------------------------------
void options_scenario(Kind kind, const char *name)
{
    ptmi_ctx *c = context(64, 16, kind);
    const std::vector<int64_t> irregular = {0, 1, 2, 64, 65, 101, 102, 164, 165, 4096, 4097};
    const struct { int option; std::vector<int64_t> values; } rows[] = {
        {0, {0}},
        {PTMI_OPT_STREAMS_SEED_RULE, {-1, 0, 1, 2, 3}},
        {PTMI_OPT_STREAM_STEP_CAP, {0, 1, 2, 1 << 30, (1 << 30) + 1}},
        {PTMI_OPT_STREAM_CAPACITY, {0, 1, 4, 64, 65}},
        {PTMI_OPT_STREAMS_FORM, {-1, 0, 1, 2, 3}},
        {PTMI_OPT_STREAM_BATCH, {-1, 0, 8, 64, 65}},
        {PTMI_OPT_SPP_CHUNKS, {-1, 0, 8, 64, 65}},
        {PTMI_OPT_ARITHMETIC, {-1, 0, 1, 2}},
        {PTMI_OPT_STREAM_TAIL, {-2, -1, 0, 250, 1000, 1001}},
        {PTMI_OPT_ORDERED_PASSES, {-1, 0, 2, 64, 65}},
        {PTMI_OPT_GLASS_BATCH, {-1, 0, 2, 64, 65}},
        {PTMI_OPT_STREAM_GRADED, {-1, 0, 1, 2}},
        {PTMI_OPT_SNAPSHOT_BUDGET_MB, {-1, 0, 5, 1 << 20, (1 << 20) + 1}},
        {PTMI_OPT_STREAM_PASS_GROUPS, irregular},
        {PTMI_OPT_CHAIN_SLOTS, irregular},
        {PTMI_OPT_PASS_HANDOFF, {-1, 0, 1, 2}},
        {16, {0}},
        {PTMI_OPT_BVH_DEVICE_BUILD, {-1, 0, 1, 2}},
        {18, {0}},
    };
    for (const auto &row : rows) {
        std::vector<int64_t> values = row.values;
        values.push_back((1ll << 32) + 1);                     // (what an int would read as 1)
        for (int64_t value : values) {
            mark();
            const int rc = ptmi_set_option(c, row.option, value);
            report(std::string(name) + " scene, option " + std::to_string(row.option) + " = " + std::to_string(value), rc);
            if (rc != PTMI_OK) std::printf("  %s\n", ptmi_last_error(c));
            int64_t back = -12345;
            const int grc = ptmi_get_option(c, row.option, &back);
            std::printf("  get: rc %d value %lld%s%s\n", grc, (long long)back, grc != PTMI_OK ? " " : "", grc != PTMI_OK ? ptmi_last_error(c) : "");
        }
    }
    std::printf("get without a value: rc %d %s\n", ptmi_get_option(c, PTMI_OPT_STREAM_TAIL, nullptr), ptmi_last_error(c));
    const int variants[6] = {-1, 0, 1, kVariantRows, 9, 19};
    for (int variant : variants) {
        const int rc = ptmi_set_variant(c, variant);
        std::printf("%s scene, variant %d: rc %d %s\n", name, variant, rc, rc != PTMI_OK ? ptmi_last_error(c) : "");
    }
    CHECK(ptmi_set_variant(c, 0) == PTMI_OK);
    // (PTMI_OPT_ARITHMETIC was left at PTMI_ARITH_CONTRACTED: a BVH or mesh scene has no such kernel)
    const ptmi_camera cam = camera();
    render(c, std::string(name) + " scene, render Inline with contracted arithmetic", cam, PTMI_INLINE, 8, kind == Linear ? PTMI_OK : PTMI_EINVAL);
    render(c, std::string(name) + " scene, render Streams with contracted arithmetic", cam, PTMI_STREAMS, 8);
    const struct { int algorithm, limit, spp; } bad[] = {{7, 8, 1}, {PTMI_INLINE, -1, 1}, {PTMI_INLINE, 8, -1}};
    for (const auto &b : bad) std::printf("render(%d, %d, %d): rc %d %s\n", b.algorithm, b.limit, b.spp, ptmi_render(c, &cam, b.algorithm, b.limit, b.spp), ptmi_last_error(c));
    std::printf("render without a camera: rc %d %s\n", ptmi_render(c, nullptr, PTMI_INLINE, 8, 1), ptmi_last_error(c));
    finish(c);
}

// ---- the walked sequence ---------------------------------------------------------------------------------------------------------
// A context's creation, launches 0 to 4 of the per-pixel order and the statistics calls.  kind >= 0: the k-th runtime call of the kind fails.
// Returns whether there was a k-th call; *failed: an ABI call returned its error (the sequence ends there).
bool walked_sequence(int kind, long k, bool *failed)
{
    const ptmi_camera cam = camera();
    ptmi_ctx *c = nullptr;
    ptmi_stats st;
    uint32_t words[64];
    const long before = kind >= 0 ? hipstub_calls(kind) : 0;
    if (kind >= 0) hipstub_fail(kind, k);
    std::vector<std::pair<const char *, std::function<int()>>> steps = {
        {"create", [&] { return ptmi_create(&c, 0); }},
        {"set_scene", [&] { return set_scene(c); }},
        {"resize", [&] { return ptmi_resize(c, 64, 16); }},
        {"init_output", [&] { return ptmi_init_output(c, 3); }},
        {"get_stats", [&] { return ptmi_get_stats(c, &st); }},
    };
    for (int i = 0; i < 5; ++i) steps.push_back({"render", [&] { return ptmi_render(c, &cam, PTMI_INLINE, 8, 1); }});
    steps.push_back({"get_stats", [&] { return ptmi_get_stats(c, &st); }});
    steps.push_back({"debug_counters", [&] { return ptmi_debug_counters(c, words); }});
    steps.push_back({"reset_stats", [&] { return ptmi_reset_stats(c); }});
    steps.push_back({"render", [&] { return ptmi_render(c, &cam, PTMI_INLINE, 8, 1); }});
    steps.push_back({"get_stats", [&] { return ptmi_get_stats(c, &st); }});
    *failed = false;
    for (const auto &s : steps) {
        mark();
        const int rc = s.second();
        report(std::string("walked: ") + s.first, rc);
        if (rc == PTMI_OK) continue;
        CHECK(kind >= 0 && (rc == PTMI_EHIP || rc == PTMI_ENOMEM) && ptmi_last_error(c) && *ptmi_last_error(c));
        *failed = true;
        break;
    }
    const bool hit = kind >= 0 && hipstub_calls(kind) - before >= k;
    if (kind >= 0) hipstub_fail(kind, 0);
    CHECK(!*failed || hit);
    if (c && *failed) {                                        // the context is whole: it is sized anew, renders and says what it counted
        CHECK(set_scene(c) == PTMI_OK && ptmi_resize(c, 64, 16) == PTMI_OK && ptmi_init_output(c, 3) == PTMI_OK);
        for (int i = 0; i < 3; ++i) CHECK(ptmi_render(c, &cam, PTMI_INLINE, 8, 1) == PTMI_OK);
        CHECK(ptmi_get_stats(c, &st) == PTMI_OK && ptmi_reset_stats(c) == PTMI_OK);
    }
    if (c) ptmi_destroy(c);
    check_clean_after_destroy();
    return hit;
}

}  // namespace

int main(int argc, char **argv)
{
    g_plain = !(argc > 1 && std::strcmp(argv[1], "walk") == 0);
    watch_arguments();
    bool failed = false;
    if (g_plain) {
        walked_sequence(-1, 0, &failed);
        order_scenario();
        stats_scenario();
        options_scenario(Linear, "linear");
        options_scenario(Bvh, "BVH");
        options_scenario(Mesh, "mesh");
        std::printf("CHAIN_STREAM_HOSTSAN_OK\n");
        return 0;
    }
    int points = 0, calls_failed = 0;
    for (int kind = 0; kind < kKinds; ++kind)
        for (long k = 1; walked_sequence(kind, k, &failed); ++k) { ++points; calls_failed += failed ? 1 : 0; }
    std::printf("walk: %d failure points, %d calls failed\n", points, calls_failed);
    std::printf("CHAIN_STREAM_HOSTSAN_OK\n");
    return 0;
}
