// chain_stream_hostsan.cpp -- the chained closure (csrc/ptmi_chain.cpp) and the stream form's host loop (csrc/ptmi_stream_call.cpp) under
// AddressSanitizer + UBSan, as a stand-alone program: linked against the library built with its host code instrumented and against the HIP
// stand-in (tests/cxx/hip_stub.cpp: device memory is host memory, kernels do not run), run directly by tests/test_chain_stream_host_sanitized.py.
// It uses include/ptmi.h and the stand-in's handles only (and the counter layout of csrc/ptmi_kernels.h, for the read-backs it places).
//
//   chain_stream_hostsan plain   one fixed scenario; after every ABI call a record of what the call did to the runtime: the calls of every
//                                kind, the live device blocks, ptmi_chain_info, and the launches and memsets in order.  The record of the
//                                commit BEFORE the two units were cut out of ptmi_api.cpp is tests/golden/chain_stream_calls.txt: a refactor
//                                leaves it as it is, line for line.
//   chain_stream_hostsan walk    the same chain calls, and one stream-form call that is redone with longer streams, with the k-th runtime
//                                call of every kind failing, for every k.
//
// Kernels do not run, so a state's planes are what was uploaded into it or what the state it was made from held: every fetch is compared
// bit for bit with a model of that.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <map>
#include <string>
#include <vector>

#include <hip/hip_runtime_api.h>

#include "ptmi.h"
#include "ptmi_kernels.h"      // the stream form's counter lines (kLv*, kCounterStride): constants only

extern "C" {
void hipstub_fail(int kind, long k);
long hipstub_calls(int kind);
long hipstub_live_blocks(void);
long hipstub_live_host_blocks(void);
long hipstub_live_streams(void);
long hipstub_live_events(void);
void hipstub_poke(const char *kernel_part, long nth, unsigned long long offset, unsigned int value);
void hipstub_clear_pokes(void);
const char *hipstub_log(void);
void hipstub_clear_log(void);
}

#define CHECK(cond)                                                                              \
    do {                                                                                         \
        if (!(cond)) { std::fprintf(stderr, "FAILED line %d: %s\n", __LINE__, #cond); std::exit(1); } \
    } while (0)

namespace {

constexpr int kKinds = 6;                      // hipMalloc, copies, launches, hipStreamSynchronize, hipHostMalloc, event / stream creation
constexpr int kWa = 24, kHa = 10, kWb = 17, kHb = 9;      // the two image sizes of the chain part
bool g_plain = true;

ptmi_camera camera()
{
    ptmi_camera cam;
    std::memset(&cam, 0, sizeof cam);
    cam.position[1] = 1.0f; cam.position[2] = 4.0f; cam.fov = 70;
    return cam;
}

void set_scene(ptmi_ctx *c, bool glass)
{
    ptmi_sphere s[2];
    std::memset(s, 0, sizeof s);
    for (int i = 0; i < 2; ++i) {
        s[i].position[0] = -1.0f + 2.0f * (float)i; s[i].position[1] = 1.0f; s[i].position[2] = -3.0f; s[i].radius = 0.9f;
        s[i].color[0] = s[i].color[1] = s[i].color[2] = 0.7f; s[i].brdf_tag = PTMI_MATTE; s[i].brdf_param = 0.8f;
    }
    if (glass) { s[0].brdf_tag = PTMI_GLASS; s[0].brdf_param = 1.5f; }
    ptmi_plane p;
    std::memset(&p, 0, sizeof p);
    p.direction[1] = 1.0f; p.color[0] = p.color[1] = p.color[2] = 0.5f; p.illuminance = 1.0f; p.brdf_tag = PTMI_MATTE; p.brdf_param = 1.0f;
    CHECK(ptmi_set_scene(c, s, 2, &p, 1) == PTMI_OK);
}

// ---- the record ------------------------------------------------------------------------------------------------------------------
long g_mark[kKinds];
void mark()
{
    for (int k = 0; k < kKinds; ++k) g_mark[k] = hipstub_calls(k);
    hipstub_clear_log();
}
void report(const char *what, int rc, ptmi_ctx *c, bool chain)
{
    if (!g_plain) return;
    std::printf("%s: rc %d calls", what, rc);
    for (int k = 0; k < kKinds; ++k) std::printf(" %ld", hipstub_calls(k) - g_mark[k]);
    std::printf(" live %ld\n", hipstub_live_blocks());
    if (chain) {
        ptmi_chain_stats i;
        CHECK(ptmi_chain_info(c, &i) == PTMI_OK);
        std::printf("  chain: device %u host %u slots %u newest %ux%u chained %llu in_place %llu uploaded %llu evictions %llu fetches %llu\n",
                    i.states_on_device, i.states_on_host, i.device_slots, i.width, i.height, (unsigned long long)i.renders_chained,
                    (unsigned long long)i.renders_in_place, (unsigned long long)i.renders_uploaded, (unsigned long long)i.evictions, (unsigned long long)i.fetches);
    }
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

// ---- the chain part --------------------------------------------------------------------------------------------------------------
struct Image {
    int w = 0, h = 0;
    std::vector<uint32_t> plane[7];            // r g b sa sb sc sctr, as words
    size_t n() const { return (size_t)w * h; }
    bool operator==(const Image &o) const
    {
        for (int i = 0; i < 7; ++i) if (plane[i] != o.plane[i]) return false;
        return w == o.w && h == o.h;
    }
};
Image image(int w, int h, uint32_t seed, int planes = 7)      // `planes` of them filled, the others zero (what a fresh block reads as)
{
    Image im;
    im.w = w; im.h = h;
    for (int i = 0; i < 7; ++i) {
        im.plane[i].assign(im.n(), 0u);
        if (i >= planes) continue;
        for (size_t k = 0; k < im.n(); ++k) {
            const uint32_t word = seed * 2654435761u + (uint32_t)i * 40503u + (uint32_t)k * 69069u + 1u;
            const float f = (float)(word >> 8) * (1.0f / 16777216.0f);
            if (i < 3) std::memcpy(&im.plane[i][k], &f, 4); else im.plane[i][k] = word;
        }
    }
    return im;
}
const float *fl(const Image &im, int i) { return reinterpret_cast<const float *>(im.plane[i].data()); }
float *fl(Image &im, int i) { return reinterpret_cast<float *>(im.plane[i].data()); }

struct Chain {
    ptmi_ctx *c = nullptr;
    std::map<uint64_t, Image> held;            // what every token the caller holds fetches
    ptmi_camera cam = camera();
};

int fetch(Chain &s, uint64_t token, Image &out, unsigned mask = 0x7f)
{
    auto f = [&](int i) { return mask >> i & 1 ? fl(out, i) : nullptr; };
    auto u = [&](int i) { return mask >> i & 1 ? out.plane[i].data() : nullptr; };
    return ptmi_chain_fetch(s.c, token, f(0), f(1), f(2), u(3), u(4), u(5), u(6));
}

void verify(Chain &s)
{
    for (const auto &kv : s.held) {
        Image got = image(kv.second.w, kv.second.h, 0, 0);
        CHECK(fetch(s, kv.first, got) == PTMI_OK);
        CHECK(got == kv.second);
    }
    ptmi_chain_stats i;
    CHECK(ptmi_chain_info(s.c, &i) == PTMI_OK);
    CHECK(i.states_on_device + i.states_on_host == s.held.size());
}

// One ABI call of the scenario.  `call` returns the code and, on PTMI_OK, has brought the model up to date.  plain: recorded, the code is the
// expected one, every token fetches its planes.  walk: a call that fails where it should not was hit by the injected failure -- the code is
// a runtime error's, every token held before the call still fetches its planes bit for bit (but `given_up`, the input of a consuming call:
// it was the call's to spend, and is either whole or gone), the counts add up, and the context renders again; the scenario ends there.
bool step(Chain &s, const char *what, int expect, const std::function<int()> &call, uint64_t given_up = 0)
{
    mark();
    const int rc = call();
    if (g_plain) {
        report(what, rc, s.c, true);
        CHECK(rc == expect);
        verify(s);
        return true;
    }
    if (rc == expect) return true;
    CHECK(expect == PTMI_OK && (rc == PTMI_EHIP || rc == PTMI_ENOMEM));
    CHECK(ptmi_last_error(s.c) && *ptmi_last_error(s.c));
    if (given_up) {
        Image got = image(s.held.at(given_up).w, s.held.at(given_up).h, 0, 0);
        const int frc = fetch(s, given_up, got);
        CHECK(frc == PTMI_ESTALE || (frc == PTMI_OK && got == s.held.at(given_up)));
        if (frc == PTMI_ESTALE) s.held.erase(given_up);
    }
    verify(s);
    const Image again = image(kWa, kHa, 99);
    uint64_t t = 0;
    CHECK(ptmi_render1_chained(s.c, &s.cam, PTMI_INLINE, 4, kWa, kHa, 0, 0, fl(again, 0), fl(again, 1), fl(again, 2), again.plane[3].data(), again.plane[4].data(),
                               again.plane[5].data(), again.plane[6].data(), &t, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == PTMI_OK);
    s.held[t] = again;
    verify(s);
    return false;
}

// render1_chained: from `token` (0: from the host planes `in`), the new state under *out
int chained(Chain &s, int w, int h, uint64_t token, int flags, const Image *in, uint64_t *out, Image *planes_out = nullptr)
{
    Image result = token && s.held.count(token) ? s.held.at(token) : (in ? *in : Image{});
    const int rc = ptmi_render1_chained(s.c, &s.cam, PTMI_INLINE, 4, w, h, token, flags,
                                        in ? fl(*in, 0) : nullptr, in ? fl(*in, 1) : nullptr, in ? fl(*in, 2) : nullptr, in ? in->plane[3].data() : nullptr,
                                        in ? in->plane[4].data() : nullptr, in ? in->plane[5].data() : nullptr, in ? in->plane[6].data() : nullptr, out,
                                        planes_out ? fl(*planes_out, 0) : nullptr, planes_out ? fl(*planes_out, 1) : nullptr, planes_out ? fl(*planes_out, 2) : nullptr,
                                        planes_out ? planes_out->plane[3].data() : nullptr, planes_out ? planes_out->plane[4].data() : nullptr,
                                        planes_out ? planes_out->plane[5].data() : nullptr, planes_out ? planes_out->plane[6].data() : nullptr);
    if (rc != PTMI_OK) { CHECK(*out == 0); return rc; }
    CHECK(*out != 0 && !s.held.count(*out));
    if (planes_out) CHECK(*planes_out == result);
    if (flags & PTMI_CHAIN_CONSUME) s.held.erase(token);
    s.held[*out] = result;
    if (g_plain) std::printf("token %llx\n", (unsigned long long)*out);
    return rc;
}

// The chain part.  Returns whether it ran to its end.  walk: the k-th runtime call of `kind` that its chain calls make fails; *hit: there was one.
bool chain_scenario(int kind = -1, long k = 0, bool *hit = nullptr)
{
    Chain s;
    CHECK(ptmi_create(&s.c, 0) == PTMI_OK);
    set_scene(s.c, false);
    CHECK(ptmi_set_option(s.c, PTMI_OPT_CHAIN_SLOTS, 2) == PTMI_OK);
    const long calls_before = kind >= 0 ? hipstub_calls(kind) : 0;
    if (kind >= 0) hipstub_fail(kind, k);
    uint64_t t[16] = {0};
    const Image p1 = image(kWa, kHa, 1), p2 = image(kWa, kHa, 2), p3 = image(kWb, kHb, 3, 3), p4 = image(kWb, kHb, 4);
    auto init = [&](int w, int h, uint64_t *out) {
        const int rc = ptmi_chain_init_output(s.c, w, h, 7, out);
        if (rc == PTMI_OK) { s.held[*out] = image(w, h, 0, 0); if (g_plain) std::printf("token %llx\n", (unsigned long long)*out); }     // (a fresh block: zeros)
        return rc;
    };
    auto release = [&](uint64_t token) { s.held.erase(token); return ptmi_chain_release(s.c, token); };
    bool on = true;
    auto go = [&](const char *what, int expect, const std::function<int()> &call, uint64_t given_up = 0) { if (on) on = step(s, what, expect, call, given_up); };

    go("init_output A: allocation within the budget", PTMI_OK, [&] { return init(kWa, kHa, &t[0]); });
    go("chained A from seven host planes, planes out", PTMI_OK, [&] { Image out = image(kWa, kHa, 0, 0); return chained(s, kWa, kHa, 0, 0, &p1, &t[1], &out); });
    go("chained A from a held state: t0 leaves, its block is reused", PTMI_OK, [&] { return chained(s, kWa, kHa, t[1], 0, nullptr, &t[2]); });
    go("fetch r and sb of t0 from its host copy", PTMI_OK, [&] {
        Image got = image(kWa, kHa, 0, 0);
        const int rc = fetch(s, t[0], got, 0x11);
        if (rc == PTMI_OK) CHECK(got.plane[0] == s.held.at(t[0]).plane[0] && got.plane[4] == s.held.at(t[0]).plane[4]);
        return rc;
    });
    go("fetch g and sctr of t2 from the device", PTMI_OK, [&] {
        Image got = image(kWa, kHa, 0, 0);
        const int rc = fetch(s, t[2], got, 0x42);
        if (rc == PTMI_OK) CHECK(got.plane[1] == s.held.at(t[2]).plane[1] && got.plane[6] == s.held.at(t[2]).plane[6] && got.plane[0] == image(kWa, kHa, 0, 0).plane[0]);
        return rc;
    });
    go("fetch of no plane", PTMI_OK, [&] { Image got = image(kWa, kHa, 0, 0); return fetch(s, t[2], got, 0); });
    go("chained A from an evicted state: a copy", PTMI_OK, [&] { return chained(s, kWa, kHa, t[0], 0, nullptr, &t[3]); });
    go("chained A consuming an evicted state", PTMI_OK, [&] { return chained(s, kWa, kHa, t[1], PTMI_CHAIN_CONSUME, nullptr, &t[4]); }, t[1]);
    go("chained A consuming a state on the device: in place", PTMI_OK, [&] { return chained(s, kWa, kHa, t[3], PTMI_CHAIN_CONSUME, nullptr, &t[5]); }, t[3]);
    go("release t4", PTMI_OK, [&] { return release(t[4]); });
    go("release t4 again", PTMI_OK, [&] { return release(t[4]); });
    go("chained A from a held state: a free block of the size", PTMI_OK, [&] { return chained(s, kWa, kHa, t[5], 0, nullptr, &t[6]); });
    go("chained A, stale token with host planes: uploaded", PTMI_OK, [&] { return chained(s, kWa, kHa, t[4], 0, &p2, &t[7]); });
    go("chained A, stale token without host planes", PTMI_ESTALE, [&] { return chained(s, kWa, kHa, t[4], 0, nullptr, &t[15]); });
    go("chained A, neither token nor planes", PTMI_ESTALE, [&] { return chained(s, kWa, kHa, 0, 0, nullptr, &t[15]); });
    go("chained B, a token of another image size", PTMI_EINVAL, [&] { return chained(s, kWb, kHb, t[6], 0, nullptr, &t[15]); });
    go("chained A, unknown flag", PTMI_EINVAL, [&] { return chained(s, kWa, kHa, t[6], 2, nullptr, &t[15]); });
    CHECK(ptmi_set_option(s.c, PTMI_OPT_CHAIN_SLOTS, 3) == PTMI_OK);
    go("reseed B from three host planes: allocation within the budget of 3", PTMI_OK, [&] {
        const int rc = ptmi_chain_reseed(s.c, 11, kWb, kHb, 0, 0, fl(p3, 0), fl(p3, 1), fl(p3, 2), &t[8]);
        if (rc == PTMI_OK) { s.held[t[8]] = p3; if (g_plain) std::printf("token %llx\n", (unsigned long long)t[8]); }
        return rc;
    });
    go("release t7", PTMI_OK, [&] { return release(t[7]); });
    go("init_output B: the free block of size A is purged", PTMI_OK, [&] { return init(kWb, kHb, &t[9]); });
    go("reseed B from a held state: a state of size A leaves, its block is freed", PTMI_OK, [&] {
        const int rc = ptmi_chain_reseed(s.c, 12, kWb, kHb, t[8], 0, nullptr, nullptr, nullptr, &t[10]);
        if (rc == PTMI_OK) { s.held[t[10]] = s.held.at(t[8]); if (g_plain) std::printf("token %llx\n", (unsigned long long)t[10]); }
        return rc;
    });
    CHECK(ptmi_set_option(s.c, PTMI_OPT_CHAIN_SLOTS, 8) == PTMI_OK);
    go("chained B from host planes, the allocation within the budget failing: a state leaves instead", PTMI_OK, [&] {
        if (g_plain) hipstub_fail(0, 1);
        const int rc = chained(s, kWb, kHb, 0, 0, &p4, &t[11]);
        if (g_plain) hipstub_fail(0, 0);
        return rc;
    });
    go("chained A from an evicted state of the other size", PTMI_OK, [&] { return chained(s, kWa, kHa, t[2], 0, nullptr, &t[12]); });
    go("chained B consuming an evicted state of size B", PTMI_OK, [&] { return chained(s, kWb, kHb, t[8], PTMI_CHAIN_CONSUME, nullptr, &t[13]); }, t[8]);
    if (kind >= 0) { *hit = hipstub_calls(kind) - calls_before >= k; hipstub_fail(kind, 0); }
    if (on && !g_plain) verify(s);
    ptmi_destroy(s.c);
    check_clean_after_destroy();

    // nothing to move out: a context without a state, the allocation within the budget failing
    if (on && g_plain) {
        Chain e;
        CHECK(ptmi_create(&e.c, 0) == PTMI_OK);
        uint64_t token = 0;
        mark();
        hipstub_fail(0, 1);
        const int rc = ptmi_chain_init_output(e.c, kWa, kHa, 5, &token);
        hipstub_fail(0, 0);
        report("init_output A, nothing to evict, the first allocation failing", rc, e.c, true);
        CHECK(rc == PTMI_OK && token != 0);
        e.held[token] = image(kWa, kHa, 0, 0);
        verify(e);
        ptmi_destroy(e.c);
        check_clean_after_destroy();
    }
    return on;
}

// ---- the stream-form part --------------------------------------------------------------------------------------------------------
unsigned long long line(int n) { return (unsigned long long)n * ptmi::kCounterStride * 4; }           // byte offset of counter line n
unsigned long long level_line(int level, int i) { return line(ptmi::kLvCursor + ptmi::kLvPerLevel * level + i); }
const char *const kSplit = "streams_split_kernel", *const kLevel = "streams_level_kernel";

ptmi_ctx *stream_context(bool glass, int w, int h)
{
    ptmi_ctx *c = nullptr;
    CHECK(ptmi_create(&c, 0) == PTMI_OK);
    set_scene(c, glass);
    CHECK(ptmi_set_option(c, PTMI_OPT_STREAMS_FORM, PTMI_FORM_STREAM) == PTMI_OK);
    CHECK(ptmi_resize(c, w, h) == PTMI_OK);
    CHECK(ptmi_init_output(c, 3) == PTMI_OK);
    return c;
}

void render_step(ptmi_ctx *c, const char *what, int spp = 4)
{
    const ptmi_camera cam = camera();
    mark();
    const int rc = ptmi_render(c, &cam, PTMI_STREAMS, 8, spp);
    hipstub_clear_pokes();
    report(what, rc, c, false);
    CHECK(rc == PTMI_OK);
    ptmi_stats st;
    mark();
    CHECK(ptmi_get_stats(c, &st) == PTMI_OK);
    std::printf("  stats: live %llu samples %llu iterations %u dropped %llu truncated %llu spilled %llu overflowed %llu\n", (unsigned long long)st.live_bounces,
                (unsigned long long)st.samples, st.stream_iterations, (unsigned long long)st.stream_rays_dropped, (unsigned long long)st.stream_rays_truncated,
                (unsigned long long)st.stream_rays_spilled, (unsigned long long)st.stream_rays_overflowed);
}

void option_step(ptmi_ctx *c, const char *what, int option, int64_t value)
{
    mark();
    const int rc = ptmi_set_option(c, option, value);
    report(what, rc, c, false);
    CHECK(rc == PTMI_OK);
    int64_t back = 0;
    CHECK(ptmi_get_option(c, PTMI_OPT_STREAM_CAPACITY, &back) == PTMI_OK);
    std::printf("  stream capacity in force %lld\n", (long long)back);
}

void stream_scenario()
{
    ptmi_ctx *c = stream_context(true, 160, 96);
    render_step(c, "glass 160x96, first call");
    hipstub_poke(kSplit, 1, level_line(0, 0), 3);              // the stream's cursor
    hipstub_poke(kSplit, 1, level_line(0, 2), 3);              // the children stored (shard 0)
    render_step(c, "one overflow level");
    hipstub_poke(kSplit, 1, level_line(0, 0), 3);
    hipstub_poke(kSplit, 1, level_line(0, 3), 3);              // (another shard)
    hipstub_poke(kLevel, 1, level_line(1, 0), 2);
    hipstub_poke(kLevel, 1, level_line(1, 2), 2);
    render_step(c, "two overflow levels");
    CHECK(ptmi_reset_stats(c) == PTMI_OK);
    hipstub_poke(kSplit, 1, line(ptmi::kLvDropped), 5);
    render_step(c, "children dropped: redone with longer streams");
    hipstub_poke(kSplit, 1, line(ptmi::kLvDropped), 5);
    hipstub_poke(kSplit, 2, line(ptmi::kLvDropped), 1);
    render_step(c, "two redos in one call");
    option_step(c, "stream capacity 64", PTMI_OPT_STREAM_CAPACITY, 64);
    CHECK(ptmi_reset_stats(c) == PTMI_OK);
    hipstub_poke(kSplit, 1, line(ptmi::kLvDropped), 9);
    render_step(c, "drops at capacity 64 stand");
    mark();
    CHECK(ptmi_resize(c, 64, 32) == PTMI_OK);
    report("resize to 64x32", PTMI_OK, c, false);
    CHECK(ptmi_init_output(c, 4) == PTMI_OK);
    hipstub_poke(kSplit, 1, line(ptmi::kLvDropped), 2);
    render_step(c, "a smaller image");
    option_step(c, "stream capacity 2", PTMI_OPT_STREAM_CAPACITY, 2);
    hipstub_poke(kSplit, 1, line(ptmi::kLvDropped), 2);
    render_step(c, "after the capacity was set: streams carved anew, one redo");
    set_scene(c, false);
    render_step(c, "the scene lost its GLASS: the colour backup goes");
    ptmi_destroy(c);
    check_clean_after_destroy();

    c = stream_context(false, 160, 96);
    render_step(c, "ordered passes, first call: no order yet, no tail");
    render_step(c, "ordered passes, second call: the tail beside it");
    render_step(c, "ordered passes, third call");
    option_step(c, "no tail", PTMI_OPT_STREAM_TAIL, 0);
    render_step(c, "ordered passes without the tail");
    option_step(c, "two ordered passes", PTMI_OPT_ORDERED_PASSES, 2);
    render_step(c, "two ordered passes of 32 samples", 64);
    ptmi_destroy(c);
    check_clean_after_destroy();
}

// One stream-form call that is redone once, with the k-th runtime call of `kind` failing.  Returns whether the failure was reached.
bool stream_walk_once(int kind, long k, int *failed)
{
    ptmi_ctx *c = stream_context(true, 160, 96);
    const ptmi_camera cam = camera();
    CHECK(ptmi_render(c, &cam, PTMI_STREAMS, 8, 4) == PTMI_OK);
    hipstub_poke(kSplit, 1, line(ptmi::kLvDropped), 5);
    const long before = hipstub_calls(kind);
    hipstub_fail(kind, k);
    const int rc = ptmi_render(c, &cam, PTMI_STREAMS, 8, 4);
    const bool hit = hipstub_calls(kind) - before >= k;
    hipstub_fail(kind, 0);
    hipstub_clear_pokes();
    if (rc != PTMI_OK) {
        CHECK(hit && (rc == PTMI_EHIP || rc == PTMI_ENOMEM) && ptmi_last_error(c) && *ptmi_last_error(c));
        ++*failed;
    }
    CHECK(ptmi_render(c, &cam, PTMI_STREAMS, 8, 4) == PTMI_OK);      // the context renders again
    ptmi_stats st;
    CHECK(ptmi_get_stats(c, &st) == PTMI_OK);
    ptmi_destroy(c);
    check_clean_after_destroy();
    return hit;
}

}  // namespace

int main(int argc, char **argv)
{
    g_plain = !(argc > 1 && std::strcmp(argv[1], "walk") == 0);
    if (g_plain) {
        CHECK(chain_scenario());
        stream_scenario();
        std::printf("CHAIN_STREAM_HOSTSAN_OK\n");
        return 0;
    }
    int points = 0, ended_early = 0, stream_failed = 0;
    for (int kind = 0; kind < kKinds; ++kind)
        for (long k = 1;; ++k) {
            bool hit = false;
            const bool to_the_end = chain_scenario(kind, k, &hit);
            if (!hit) { CHECK(to_the_end); break; }
            ++points; ended_early += to_the_end ? 0 : 1;
        }
    for (int kind = 0; kind < kKinds; ++kind)
        for (long k = 1; stream_walk_once(kind, k, &stream_failed); ++k) ++points;
    // (20 of the scenario's calls reach the runtime, each with at least one call that can fail and is not absorbed; the redone stream-form
    // call makes two split launches, the seeds' launch, two read-backs and their synchronisations: ten at the least)
    CHECK(ended_early >= 20 && stream_failed >= 10);
    std::printf("walk: %d failure points, %d chain calls and %d stream-form calls failed\n", points, ended_early, stream_failed);
    std::printf("CHAIN_STREAM_HOSTSAN_OK\n");
    return 0;
}
