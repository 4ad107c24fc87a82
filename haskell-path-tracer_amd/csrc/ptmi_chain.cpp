// ptmi_chain.cpp -- the chained closure: states under tokens (include/ptmi.h, "the closure, chained"; ChainStore in ptmi_ctx.h).  A state's planes are a
// DeviceBlock like every other of the context: allocated, released and -- at ptmi_destroy -- found through each_block.  launch_render (ptmi_api.cpp) renders into it.
#include "ptmi_ctx.h"

#include <new>

using namespace ptmi;

namespace {

int find(const ChainStore &s, uint64_t token)
{
    if (token == 0) return -1;
    for (size_t i = s.states.size(); i-- > 0;)              // (the newest states are the ones asked for)
        if (s.states[i].token == token) return (int)i;
    return -1;
}

int chain_slots(const ptmi_ctx *c, size_t bytes)
{
    const size_t fit = (c->device_memory / 16) / (bytes ? bytes : 1);
    return c->opt_chain_slots > 0 ? c->opt_chain_slots : fit < 3 ? 3 : (fit > 64 ? 64 : (int)fit);
}

// A device block of `bytes` for a new state, into `out` (empty).  In this order: a block a released state left behind; a fresh allocation
// while fewer than PTMI_OPT_CHAIN_SLOTS blocks exist; the block of the OLDEST state still on the device (but `keep`), whose planes first
// move to host memory the library owns -- a state is never lost, only served from further away.
int take_block(ptmi_ctx *c, size_t bytes, uint64_t keep, DeviceBlock &out)
{
    ChainStore &s = c->chain;
    for (size_t i = 0; i < s.free_blocks.size(); ++i)
        if (s.free_blocks[i].bytes == bytes) { out = s.free_blocks[i]; s.free_blocks.erase(s.free_blocks.begin() + (long)i); return PTMI_OK; }
    if (!s.free_blocks.empty()) {                            // blocks of another image size: of no use any more
        PTMI_HIP(c, hipStreamSynchronize(c->stream));
        for (DeviceBlock &fb : s.free_blocks) release(fb);
        s.free_blocks.clear();
    }
    size_t on_device = 0;
    for (const ChainState &st : s.states) on_device += st.block.p ? 1 : 0;
    if ((int)on_device < chain_slots(c, bytes) && allocate(out, bytes) == hipSuccess) return PTMI_OK;
    for (ChainState &st : s.states) {                        // the budget is spent, or the device is full before it is: make room instead
        if (!st.block.p || st.token == keep) continue;
        st.host.reset(new (std::nothrow) char[st.block.bytes]);
        if (!st.host) return fail(c, PTMI_ENOMEM, "no host memory for a state of the chained closure that has to leave the device");
        const CopySpan whole{st.block.p, st.host.get(), st.block.bytes};
        PTMI_HIP(c, copy_to_host(c, &whole, 1));             // (drains the stream: nothing still reads the block)
        ++s.stats.evictions;
        out = st.block;
        st.block = DeviceBlock{};
        if (out.bytes == bytes) return PTMI_OK;
        release(out);
        break;
    }
    // room was made -- or there was nothing to move out (the budget is below what one call needs): allocate all the same
    const hipError_t e = allocate(out, bytes);
    return e == hipSuccess ? PTMI_OK : fail_hip(c, e, "hipMalloc(out, bytes)");      // (the text this failure has always had: callers may match it)
}

// A state that has no token yet, and the block taken for it.  Unless commit() puts it into the store under a new token, the block goes back
// to the free list (stream-ordered reuse: no wait) -- a failed call leaves no half-made state, and spends no token.
struct Pending {
    ChainStore &store;
    ChainState state;
    Pending(ChainStore &s, int width, int height) : store(s) { state.width = width; state.height = height; }
    Pending(const Pending &) = delete;
    ~Pending() { if (state.block.p) store.free_blocks.push_back(state.block); }
    Planes planes() const { return carve(state.block.p, (size_t)state.width * state.height); }
    uint64_t commit()       // Token = (the context's serial number << 40) | a counter that starts at 1: never 0, never reused, another context's never matches.
    {
        state.token = (store.serial << 40) | (++store.counter & ((1ull << 40) - 1));
        store.states.push_back(std::move(state));
        state.block = DeviceBlock{};
        return store.states.back().token;
    }
};

// The planes of the state a call WRITES, into `fresh`: token_in's in a block of its own (device-to-device copy, or in place when the caller
// gives the input up), or -- token_in not held -- the caller's host planes uploaded (`planes_in`: the first n_planes of seven; none: the
// block as it comes).
int begin(ptmi_ctx *c, Pending &fresh, uint64_t token_in, int flags, const void *const *planes_in, int n_planes)
{
    ChainStore &s = c->chain;
    const int width = fresh.state.width, height = fresh.state.height;
    if (width <= 0 || height <= 0) return fail(c, PTMI_EINVAL, "width and height must be positive");
    if (too_many_pixels(width, height)) return fail(c, PTMI_ELIMIT, "image too large");
    if (flags & ~PTMI_CHAIN_CONSUME) return fail(c, PTMI_EINVAL, "unknown flag");
    const size_t n = (size_t)width * height, bytes = planes_bytes(n);
    const int in = find(s, token_in);
    ChainState *src = in >= 0 ? &s.states[(size_t)in] : nullptr;
    if (src && (src->width != width || src->height != height)) return fail(c, PTMI_EINVAL, "the token names a state of another image size");
    for (int i = 0; !src && i < n_planes; ++i)               // the copy path: the RenderResult comes from the host
        if (!planes_in || !planes_in[i])
            return fail(c, PTMI_ESTALE, token_in ? "the token names no state this context holds, and no host planes were given to take its place"
                                                 : "neither a token nor host planes were given");
    const bool consume = src && (flags & PTMI_CHAIN_CONSUME);
    if (consume && src->block.p) fresh.state.block = src->block;      // the caller gives the input up: its block becomes the output
    else {                                                   // (a source that fails to come back from the host stands as it was)
        if (int rc = take_block(c, bytes, src ? src->token : 0, fresh.state.block)) return rc;
        CopySpan spans[7] = {{fresh.state.block.p, src ? src->host.get() : nullptr, bytes}};      // an evicted source: its host copy, whole
        const int n_spans = src ? 1 : (n_planes ? plane_spans(fresh.planes(), planes_in, n, spans) : 0);
        hipError_t e = hipSuccess;                           // (`e`: the text a failure here has always quoted)
        if (src && src->block.p) e = hipMemcpyAsync(fresh.state.block.p, src->block.p, bytes, hipMemcpyDeviceToDevice, c->stream);
        else if (n_spans && (e = copy_to_device(c, spans, n_spans)) == hipSuccess) e = hipStreamSynchronize(c->stream);   // host memory is borrowed for the call only
        PTMI_HIP(c, e);
    }
    if (consume) s.states.erase(s.states.begin() + in);
    if (src) { ++s.stats.renders_chained; s.stats.renders_in_place += consume ? 1 : 0; }
    else if (n_planes) ++s.stats.renders_uploaded;
    return PTMI_OK;
}

int download(ptmi_ctx *c, const ChainState &st, const void *const dst[7])
{
    const size_t n = (size_t)st.width * st.height;
    CopySpan spans[7];
    const int k = plane_spans(carve(st.block.p ? st.block.p : st.host.get(), n), dst, n, spans);      // (a null pointer: that plane is not asked for)
    if (!k) return PTMI_OK;
    ++c->chain.stats.fetches;
    if (st.block.p) PTMI_HIP(c, copy_to_host(c, spans, k));  // stream-ordered behind the renders; returns with the planes filled
    else for (int i = 0; i < k; ++i) std::memcpy(spans[i].host, spans[i].dev, spans[i].bytes);
    return PTMI_OK;
}

// ptmi_chain_init_output (no input at all) and ptmi_chain_reseed: a state's planes, then its seeds
int seeded(ptmi_ctx *c, uint64_t seed0, bool clear, int width, int height, uint64_t token_in, int flags, const void *const *planes_in, int n_planes, uint64_t *token_out)
{
    if (!c) return PTMI_EINVAL;
    std::lock_guard<std::mutex> lock(c->mu);
    if (!token_out) return fail(c, PTMI_EINVAL, "token_out is NULL");
    *token_out = 0;
    PTMI_HIP(c, hipSetDevice(c->device));
    Pending fresh(c->chain, width, height);
    if (int rc = begin(c, fresh, token_in, flags, planes_in, n_planes)) return rc;
    const hipError_t e = launch_seed(fresh.planes(), width, height, height, 1, 0, seed0, clear, c->stream);
    PTMI_HIP(c, e);
    *token_out = fresh.commit();
    return PTMI_OK;
}

}  // namespace

extern "C" {

int ptmi_render1_chained(ptmi_ctx *c, const ptmi_camera *camera, int algorithm, int bounce_limit, int width, int height, uint64_t token_in, int flags,
                         const float *r_in, const float *g_in, const float *b_in, const uint32_t *sa_in, const uint32_t *sb_in, const uint32_t *sc_in, const uint32_t *sctr_in,
                         uint64_t *token_out, float *r_out, float *g_out, float *b_out, uint32_t *sa_out, uint32_t *sb_out, uint32_t *sc_out, uint32_t *sctr_out)
{
    if (!c) return PTMI_EINVAL;
    std::lock_guard<std::mutex> lock(c->mu);
    if (!token_out) return fail(c, PTMI_EINVAL, "token_out is NULL");
    *token_out = 0;
    if (int rc = check_render_args(c, camera, algorithm, bounce_limit, 1)) return rc;
    PTMI_HIP(c, hipSetDevice(c->device));
    const void *const planes_in[7] = {r_in, g_in, b_in, sa_in, sb_in, sc_in, sctr_in}, *const dst[7] = {r_out, g_out, b_out, sa_out, sb_out, sc_out, sctr_out};
    Pending fresh(c->chain, width, height);
    if (int rc = begin(c, fresh, token_in, flags, planes_in, 7)) return rc;
    if (int rc = launch_render(c, RenderTarget::whole(fresh.planes(), width, height), camera, algorithm, bounce_limit, 1)) return rc;
    if (int rc = download(c, fresh.state, dst)) return rc;
    *token_out = fresh.commit();
    return PTMI_OK;
}

int ptmi_chain_init_output(ptmi_ctx *c, int width, int height, uint64_t seed0, uint64_t *token_out) { return seeded(c, seed0, true, width, height, 0, 0, nullptr, 0, token_out); }

int ptmi_chain_reseed(ptmi_ctx *c, uint64_t seed0, int width, int height, uint64_t token_in, int flags,
                      const float *r_in, const float *g_in, const float *b_in, uint64_t *token_out)
{
    const void *const planes_in[7] = {r_in, g_in, b_in, nullptr, nullptr, nullptr, nullptr};
    return seeded(c, seed0, false, width, height, token_in, flags, planes_in, 3, token_out);
}

int ptmi_chain_fetch(ptmi_ctx *c, uint64_t token, float *r, float *g, float *b, uint32_t *sa, uint32_t *sb, uint32_t *sc, uint32_t *sctr)
{
    if (!c) return PTMI_EINVAL;
    std::lock_guard<std::mutex> lock(c->mu);
    const int idx = find(c->chain, token);
    if (idx < 0) return fail(c, PTMI_ESTALE, "the token names no state this context holds");
    PTMI_HIP(c, hipSetDevice(c->device));
    const void *const dst[7] = {r, g, b, sa, sb, sc, sctr};
    return download(c, c->chain.states[(size_t)idx], dst);
}

int ptmi_chain_release(ptmi_ctx *c, uint64_t token)
{
    if (!c) return PTMI_EINVAL;
    std::lock_guard<std::mutex> lock(c->mu);
    ChainStore &s = c->chain;
    const int idx = find(s, token);
    if (idx < 0) return PTMI_OK;
    if (s.states[(size_t)idx].block.p) s.free_blocks.push_back(s.states[(size_t)idx].block);     // stream-ordered reuse: no wait
    s.states.erase(s.states.begin() + idx);
    return PTMI_OK;
}

int ptmi_chain_info(ptmi_ctx *c, ptmi_chain_stats *out)
{
    if (!c) return PTMI_EINVAL;
    std::lock_guard<std::mutex> lock(c->mu);
    if (!out) return fail(c, PTMI_EINVAL, "out is NULL");
    const ChainStore &s = c->chain;
    *out = s.stats;                                          // (the counts of states are zero in there: filled in here)
    for (const ChainState &st : s.states) { if (st.block.p) ++out->states_on_device; else ++out->states_on_host; }
    out->width = s.states.empty() ? 0 : (uint32_t)s.states.back().width;
    out->height = s.states.empty() ? 0 : (uint32_t)s.states.back().height;
    out->device_slots = (uint32_t)chain_slots(c, planes_bytes((size_t)(out->width ? out->width : 1) * (out->height ? out->height : 1)));
    return PTMI_OK;
}

}  // extern "C"
