// ptmi_api.cpp -- the C ABI of include/ptmi.h: context, device planes, the option table, launches, their statistics (RenderStats) and the
// queries (the scene's calls are ptmi_scene.cpp's, the chained closure's ptmi_chain.cpp's, the stream form of Streams is ptmi_stream_call.cpp,
// the cost-ordered dispatch ptmi_order.cpp; ptmi_ctx.h is what they share).
// Compiled with hipcc together with the kernel units (ptmi_*.hip) into libptmi.so.  There is no CPU
// fallback here: without a HIP device ptmi_create fails with PTMI_ENODEVICE.
#include "ptmi_ctx.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <algorithm>
#include <atomic>
#include <new>

using namespace ptmi;

// render Inline with contracted arithmetic: the second object made from ptmi_inline.hip (see its last lines)
extern "C" int ptmi_contracted_launch_inline(const void *args, int variant, void *stream);

namespace {

thread_local std::string g_create_error;
// The message of a failed call is the calling THREAD's (several threads may share a context -- the application has three, app/Main.hs:178-180
// -- and two of them may fail at once: a pointer into the context's own string would be freed under the first reader by the second failure).
thread_local std::string t_error;               // this thread's last failure on a context ...
thread_local const ptmi_ctx *t_error_of = nullptr;   // ... and which

}  // namespace

int ptmi::fail(ptmi_ctx *c, int code, const std::string &msg)
{
    if (c) { c->err = msg; t_error = msg; t_error_of = c; }      // (c->err: under c->mu, which every caller with a context holds)
    else g_create_error = msg;
    return code;
}

int ptmi::fail_hip(ptmi_ctx *c, hipError_t e, const char *call)
{
    (void)hipGetLastError();
    return fail(c, e == hipErrorOutOfMemory ? PTMI_ENOMEM : PTMI_EHIP, std::string(call) + ": " + hipGetErrorString(e));
}

hipError_t ptmi::allocate(DeviceBlock &b, size_t bytes)
{
    const hipError_t e = hipMalloc(&b.p, bytes);
    if (e == hipSuccess) b.bytes = bytes;
    else { (void)hipGetLastError(); b.p = nullptr; }
    return e;
}

void ptmi::release(DeviceBlock &b)
{
    if (b.p) (void)hipFree(b.p);
    b = DeviceBlock{};
}

int ptmi::grow(ptmi_ctx *c, DeviceBlock &b, size_t bytes, const char *what)
{
    if (bytes <= b.bytes) return PTMI_OK;
    if (b.p) {
        PTMI_HIP(c, hipStreamSynchronize(c->stream));
        release(b);
    }
    const hipError_t e = allocate(b, bytes);
    if (e != hipSuccess)
        return fail(c, e == hipErrorOutOfMemory ? PTMI_ENOMEM : PTMI_EHIP,
                    std::string(what) + ": hipMalloc of " + std::to_string(bytes) + " bytes: " + hipGetErrorString(e));
    return PTMI_OK;
}

static hipError_t copy_spans(ptmi_ctx *c, const CopySpan *spans, int n, bool to_host)
{
    size_t total = 0;
    for (int i = 0; i < n; ++i) total += spans[i].bytes;
    if (c->stager.threads() > 0 && total >= Stager::kMinBytes) return to_host ? c->stager.to_host(spans, n, c->stream) : c->stager.to_device(spans, n, c->stream);
    for (int i = 0; i < n; ++i) {
        if (!spans[i].bytes) continue;
        const hipError_t e = to_host ? hipMemcpyAsync(spans[i].host, spans[i].dev, spans[i].bytes, hipMemcpyDeviceToHost, c->stream)
                                     : hipMemcpyAsync(spans[i].dev, spans[i].host, spans[i].bytes, hipMemcpyHostToDevice, c->stream);
        if (e != hipSuccess) return e;
    }
    return to_host ? hipStreamSynchronize(c->stream) : hipSuccess;
}
hipError_t ptmi::copy_to_device(ptmi_ctx *c, const CopySpan *spans, int n) { return copy_spans(c, spans, n, false); }
hipError_t ptmi::copy_to_host(ptmi_ctx *c, const CopySpan *spans, int n) { return copy_spans(c, spans, n, true); }

// PTMI_SEED_AUTO: `combine new old` (the seed of the result) wherever the reference defines the outcome -- no ray-splitting
// material -- and the accumulator's seed with GLASS, where several results of one step would race for it
int ptmi::effective_seed_rule(const ptmi_ctx *c)
{
    if (c->opt_seed_rule != PTMI_SEED_AUTO) return c->opt_seed_rule;
    return c->scene.has_glass ? PTMI_SEED_KEEP_ACCUMULATOR : PTMI_SEED_FROM_RESULT;
}

SceneView ptmi::scene_view(const SceneState &s)
{
    SceneView v;
    v.packed = s.packed.as<float4>(); v.n_spheres = (int)s.rows.ns; v.n_planes = (int)s.rows.np;
    v.share_xy = s.share_xy;
    return v;
}

RayCallScene ptmi::ray_call_scene(const ptmi_ctx *c)
{
    const SceneState &s = c->scene;
    return {scene_view(s), s.kind == SceneKind::Bvh ? &s.bvh : nullptr, s.kind == SceneKind::Mesh ? &s.mesh : nullptr};
}

namespace {

// A refusal that a BVH scene and a mesh scene share but for their names: "a BVH" / "a mesh", then `rest`
int refuse_kind(ptmi_ctx *c, const char *rest)
{
    return fail(c, PTMI_EINVAL, std::string(c->scene.kind == SceneKind::Bvh ? "a BVH" : "a mesh") + rest);
}

// PTMI_OPT_STREAMS_FORM resolved: does `render Streams` run in its stream ("wavefront") form?  AUTO: only where it pays and costs nothing that
// was promised -- a scene with GLASS (no reference semantics, no defined addition order in Accelerate's permute either) on ONE PART of a
// partitioned image at >= 256 samples per call: the multi-GPU job is as fast as its slowest part, and that part is 5 % faster in the stream
// form (profiles/r05_c5_part.json: part 6 of C5 29.1 against 30.7 ms; imbalance 1.02 against 1.03-1.14).  n_spp < 0: "for some sample count".
bool uses_stream_form(const ptmi_ctx *c, int algorithm, int n_parts, int n_spp)
{
    if (algorithm != PTMI_STREAMS) return false;
    if (c->scene.hierarchical()) return false;     // (a BVH or mesh scene renders through the per-pixel kernels only)
    if (c->opt_form == PTMI_FORM_STREAM || c->variant == kVariantStreamForm) return true;
    if (c->opt_form == PTMI_FORM_PIXEL) return false;
    return c->scene.has_glass && n_parts > 1 && (n_spp < 0 || n_spp >= 256);
}

int effective_stripe(const ptmi_ctx *c) { return c->stripe_rows > 0 ? c->stripe_rows : (c->height > 0 ? c->height : 1); }

int rows_of_part(int height, int stripe, int n_parts, int part)
{
    const long long cycle = (long long)stripe * n_parts;
    long long rows = (height / cycle) * stripe;
    long long rem = height % cycle - (long long)part * stripe;
    if (rem > stripe) rem = stripe;
    if (rem > 0) rows += rem;
    return (int)rows;
}

}  // namespace

Planes ptmi::carve(void *block, size_t n)
{
    Planes p;
    char *b = static_cast<char *>(block);
    const size_t plane = ((n * 4 + 255) / 256) * 256;
    p.r = reinterpret_cast<float *>(b);
    p.g = reinterpret_cast<float *>(b + plane);
    p.b = reinterpret_cast<float *>(b + 2 * plane);
    p.sa = reinterpret_cast<uint32_t *>(b + 3 * plane);
    p.sb = reinterpret_cast<uint32_t *>(b + 4 * plane);
    p.sc = reinterpret_cast<uint32_t *>(b + 5 * plane);
    p.sctr = reinterpret_cast<uint32_t *>(b + 6 * plane);
    return p;
}
size_t ptmi::planes_bytes(size_t n) { return 7 * (((n * 4 + 255) / 256) * 256); }
// (two ints multiply to 2^62: seven planes of that would wrap a size_t.  2^40 pixels are 28 TB of planes -- beyond any device, within size_t)
constexpr unsigned long long kMaxPixels = 1ull << 40;
bool ptmi::too_many_pixels(int width, int height) { return (unsigned long long)width * (unsigned long long)height > kMaxPixels; }

int ptmi::plane_spans(const Planes &p, const void *const host[7], size_t n, CopySpan spans[7])
{
    void *const dev[7] = {p.r, p.g, p.b, p.sa, p.sb, p.sc, p.sctr};
    int k = 0;
    for (int i = 0; i < 7; ++i)
        if (host[i]) spans[k++] = CopySpan{dev[i], const_cast<void *>(host[i]), n * 4};
    return k;
}

namespace {

Planes &active(ptmi_ctx *c) { return c->use_bound ? c->bound : c->owned; }

// primaryRays' per-launch values (src/Scene/Trace.hs:205-242), evaluated on the host with
// the same arithmetic definitions as the device code (ptmi_core.h); tan is the host libm's.
PrimaryUniforms make_uniforms(const ptmi_camera &cam, int width, int height)
{
    PrimaryUniforms u;
    const float c_fov = (float)cam.fov;
    const float screen_angle = (c_fov * kPi / 180.0f) / 2.0f;
    const float screen_distance = 1.0f / tanf(screen_angle);
    const float screen_half_width = tanf(screen_angle) * screen_distance;
    const V3 c_pos = mk(cam.position[0], cam.position[1], cam.position[2]);
    const V3 c_rot = mk(cam.rotation[0], cam.rotation[1], cam.rotation[2]);
    const V3 c_dir = rotate(angles_to_quaternion(c_rot), mk(0.0f, 0.0f, -1.0f));   // Util.hs:48-50, :96-97
    const float screen_aspect = (float)width / (float)height;                        // Util.hs:192-193
    const V3 center = c_pos + scale_r(c_dir, screen_distance);
    const V3 center_offset = center - c_pos;
    const V3 right = div_r(normalize(cross(center_offset, mk(0.0f, 1.0f, 0.0f))), screen_half_width);
    const V3 top = div_r(cross(c_dir, right), screen_aspect);
    u.pos = c_pos; u.center = center; u.right = right; u.top = top;
    u.size_x = (float)width; u.size_y = (float)(-height);                            // Util.hs:198-200
    return u;
}

}  // namespace

// ---- the statistics (RenderStats, ptmi_ctx.h)
hipError_t RenderStats::create(hipStream_t stream, const char **failed_call)
{
    hipError_t e;
    *failed_call = "hipEventCreate";
    if ((e = hipEventCreate(&ev0)) != hipSuccess || (e = hipEventCreate(&ev1)) != hipSuccess) return e;
    *failed_call = "hipMalloc";
    for (int i : {Live, Work, Iters, StreamCounters})
        if ((e = allocate(block[i], kBytes[i])) != hipSuccess) return e;
    *failed_call = "hipMemsetAsync";      // stream-ordered fills: the context's stream is non-blocking, so a NULL-stream hipMemset would race with it
    for (int i : {StreamCounters, Live, Work, Iters})
        if ((e = hipMemsetAsync(block[i].p, 0, kBytes[i], stream)) != hipSuccess) return e;
    return hipSuccess;
}

int RenderStats::reset(ptmi_ctx *c)
{
    for (int i : {Live, Iters, Work, StreamCounters}) PTMI_HIP(c, hipMemsetAsync(block[i].p, 0, kBytes[i], c->stream));
    nominal = 0; samples = 0;
    return PTMI_OK;
}

int RenderStats::read(ptmi_ctx *c, ptmi_stats *out)
{
    unsigned long long live = 0, sc[kScWords] = {0, 0, 0, 0}; unsigned int iters = 0;
    std::vector<unsigned long long> live_shards((size_t)kStatShards * kStatStride);     // the sharded statistics: sum / maximum over the shards
    std::vector<unsigned int> iter_shards((size_t)kStatShards * 2 * kStatStride);
    const std::pair<void *, int> reads[3] = {{live_shards.data(), Live}, {sc, StreamCounters}, {iter_shards.data(), Iters}};
    for (const auto &[host, i] : reads) PTMI_HIP(c, hipMemcpyAsync(host, block[i].p, kBytes[i], hipMemcpyDeviceToHost, c->stream));
    PTMI_HIP(c, hipStreamSynchronize(c->stream));
    for (int k = 0; k < kStatShards; ++k) {
        live += live_shards[(size_t)k * kStatStride];
        iters = std::max(iters, iter_shards[(size_t)k * 2 * kStatStride]);
    }
    const StreamFormState::Totals &form = c->stream_form.totals;
    out->live_bounces = live + form.live_host; out->nominal_bounces = nominal; out->samples = samples;
    out->stream_iterations = iters;
    out->stream_rays_dropped = form.rays_dropped + sc[kScDropped];
    out->stream_rays_truncated = form.rays_truncated + sc[kScTruncated];
    out->stream_rays_spilled = form.rays_spilled;
    out->stream_rays_overflowed = form.rays_overflowed;
    out->last_render_ms = 0.0f;
    if (timing && ev_valid) PTMI_HIP(c, hipEventElapsedTime(&out->last_render_ms, ev0, ev1));
    return PTMI_OK;
}

int RenderStats::launches_begin(ptmi_ctx *c, RenderArgs &a)
{
    a.live_counter = block[Live].as<unsigned long long>(); a.work_counter = block[Work].as<unsigned int>(); a.stream_iterations = block[Iters].as<unsigned int>();
    a.stream_counters = block[StreamCounters].as<unsigned long long>();
    if (timing) PTMI_HIP(c, hipEventRecord(ev0, c->stream));
    return PTMI_OK;
}
int RenderStats::launches_end(ptmi_ctx *c, uint64_t samples_made, uint64_t bounces_nominal)
{
    if (timing) { PTMI_HIP(c, hipEventRecord(ev1, c->stream)); ev_valid = true; }
    samples += samples_made; nominal += bounces_nominal;
    return PTMI_OK;
}

int ptmi::launch_render(ptmi_ctx *c, const RenderTarget &target, const ptmi_camera *camera, int algorithm, int bounce_limit, int n_spp)
{
    const auto &[planes, width, height, rows_local, stripe_rows, n_parts, part, sx, sy] = target;
    RenderArgs a{};
    a.cam = make_uniforms(*camera, width, height);
    a.scene = scene_view(c->scene);
    a.planes = planes;
    a.screen_x = sx; a.screen_y = sy;
    a.width = width; a.height = height; a.rows_local = rows_local;
    a.stripe_rows = stripe_rows; a.n_parts = n_parts; a.part = part;
    a.bounce_limit = bounce_limit; a.n_spp = n_spp;
    a.cus = c->cus;
    a.stream_step_cap = c->opt_step_cap; a.seed_from_result = effective_seed_rule(c) == PTMI_SEED_FROM_RESULT;
    const bool stream_form = uses_stream_form(c, algorithm, n_parts, n_spp);
    // Which launches take the cost-ordered dispatch (DispatchOrder, ptmi_order.cpp): the tiled per-pixel kernels', and the stream form's,
    // which orders its start-hit list the same way
#ifdef PTMI_STREAM_NO_ORDER
    const bool stream_order = false;
#else
    const bool stream_order = quad_positions(width, rows_local) > 0 && !sx;
#endif
    const bool ordered = stream_form ? stream_order : uses_quad_order(a, algorithm == PTMI_INLINE, c->variant);
    if (ordered)
        if (int rc = c->order.before_launches(c, *camera, c->scene.version, target, bounce_limit, algorithm, stream_form, a)) return rc;
    if (!stream_form) {
        // one word per tile workgroup for the sample chunks of the tiled per-pixel kernels (ptmi_device.h: enter_sample_chunk)
        const unsigned int need = ((unsigned int)(((width + 7) / 8) * ((rows_local + 7) / 8)) + 31u) & ~31u;
        if (int rc = grow(c, c->d_chunk_done, ((size_t)need + 32) * sizeof(unsigned int), "the sample chunks")) return rc;     // + the ticket counter's line
        a.chunk_done = c->d_chunk_done.as<unsigned int>(); a.chunk_capacity = c->chunk_capacity();
        a.spp_chunks = sx ? 1 : c->opt_spp_chunks;
    }
    if (int rc = c->stats.launches_begin(c, a)) return rc;
    const BvhView *bvh = ray_call_scene(c).bvh;            // the per-pixel kernels' BVH instantiations (check_render_args refused the rest)
    if (algorithm == PTMI_INLINE && c->opt_arithmetic == PTMI_ARITH_CONTRACTED) {
        PTMI_HIP(c, (hipError_t)ptmi_contracted_launch_inline(&a, c->variant == kVariantStreamForm ? kVariantAuto : c->variant, c->stream));
    } else if (algorithm == PTMI_INLINE && c->scene.kind == SceneKind::Mesh) {
        PTMI_HIP(c, launch_render_inline_mesh(a, c->scene.mesh, c->stream));
    } else if (algorithm == PTMI_INLINE) {
        PTMI_HIP(c, launch_render_inline(a, bvh, c->variant, c->stream));
    } else if (stream_form) {                              // rays travel through streams in HBM (PTMI_OPT_STREAMS_FORM; kVariantStreamForm)
        if (int rc = render_streams_wavefront(c, a, n_spp, *camera)) return rc;
    } else if (c->scene.has_glass) {                             // rays may split: the per-pixel tree walk
        // the first waiting children of every lane as 64-byte records in global memory (ptmi_streams_tree.hip): 16 KB per tile
        const size_t want = (size_t)tree_workgroups(width, rows_local) * kTreeFastLevels * 64 * 64;
        if (int rc = grow(c, c->tree_stack, want, "the tree walk's records of waiting children")) return rc;
        a.tree_stack = c->tree_stack.as<float4>();
        if (c->scene.kind == SceneKind::Mesh) PTMI_HIP(c, launch_render_streams_tree_mesh(a, c->scene.mesh, c->stream));
        else PTMI_HIP(c, launch_render_streams_tree(a, bvh, c->variant, c->stream));
    } else if (c->scene.kind == SceneKind::Mesh) {
        PTMI_HIP(c, launch_render_streams_mesh(a, c->scene.mesh, c->stream));
    } else {
        PTMI_HIP(c, launch_render_streams(a, bvh, c->variant, c->stream));
    }
    const uint64_t samples = (uint64_t)rows_local * (uint64_t)width * (uint64_t)(n_spp > 0 ? n_spp : 0);
    // (Streams ignores the limit, Trace.hs:166-170: no nominal count)
    if (int rc = c->stats.launches_end(c, samples, algorithm == PTMI_INLINE ? samples * (uint64_t)(bounce_limit > 0 ? bounce_limit : 0) : 0)) return rc;
    if (ordered) c->order.launches_went_out();
    return PTMI_OK;
}

int ptmi::check_render_args(ptmi_ctx *c, const ptmi_camera *camera, int algorithm, int bounce_limit, int n_spp)
{
    if (!camera) return fail(c, PTMI_EINVAL, "camera is NULL");
    if (algorithm != PTMI_INLINE && algorithm != PTMI_STREAMS) return fail(c, PTMI_EINVAL, "unknown algorithm");
    if (bounce_limit < 0) return fail(c, PTMI_EINVAL, "bounce_limit < 0");
    if (n_spp < 0) return fail(c, PTMI_EINVAL, "n_spp < 0");
    if (!c->scene.packed.p) return fail(c, PTMI_ESTATE, "ptmi_set_scene has not been called");
    // "features that require diverging rays like light refraction" need the stream algorithm (Trace.hs:56-67)
    if (algorithm == PTMI_INLINE && c->scene.has_glass)
        return fail(c, PTMI_EINVAL, "the scene holds a GLASS material: render Inline cannot split rays, use PTMI_STREAMS");
    if (algorithm == PTMI_STREAMS && c->scene.has_glass && c->opt_seed_rule == PTMI_SEED_FROM_RESULT)
        return fail(c, PTMI_EINVAL, "PTMI_SEED_FROM_RESULT is undefined when rays split (GLASS): several results race for one pixel's seed");
    if (c->scene.hierarchical() && algorithm == PTMI_INLINE && c->opt_arithmetic == PTMI_ARITH_CONTRACTED)
        return refuse_kind(c, " scene has no contracted-arithmetic kernel (PTMI_OPT_ARITHMETIC)");
    return PTMI_OK;
}

void ptmi::context_size(const ptmi_ctx *cc, int *width, int *height)
{
    ptmi_ctx *c = const_cast<ptmi_ctx *>(cc);
    std::lock_guard<std::mutex> lock(c->mu);
    *width = c->width; *height = c->height;
}

namespace {

// ---- the options: one row each.  A value is accepted within [lo, hi] unless `but` says otherwise; it is the context's `member`, set and
// read as it is -- or through the row's hooks, where setting does more than that or the value lives elsewhere.
struct Option {
    int id;
    int ptmi_ctx::*member;
    int64_t lo, hi;
    const char *refusal;
    bool (*but)(int64_t value);                 // within [lo, hi] and refused all the same
    int (*set)(ptmi_ctx *c, int value);         // instead of the plain store (the value is an accepted one)
    int64_t (*get)(ptmi_ctx *c);                // instead of the plain read
};
const Option kOptions[] = {
    {PTMI_OPT_STREAMS_SEED_RULE, &ptmi_ctx::opt_seed_rule, PTMI_SEED_KEEP_ACCUMULATOR, PTMI_SEED_AUTO, "unknown seed rule"},
    {PTMI_OPT_STREAM_STEP_CAP, &ptmi_ctx::opt_step_cap, 1, 1 << 30, "step cap must be in [1, 2^30]"},
    {PTMI_OPT_STREAM_CAPACITY, &ptmi_ctx::opt_capacity, 1, 64, "stream capacity must be in [1, 64] rays per pixel-sample", nullptr,
     [](ptmi_ctx *c, int value) { c->opt_capacity = value; return c->stream_form.forget_streams(c); },
     [](ptmi_ctx *c) { return (int64_t)c->stream_form.rays_per_pixel(c->opt_capacity); }},      // (what an earlier call grew the streams to counts)
    {PTMI_OPT_STREAMS_FORM, &ptmi_ctx::opt_form, PTMI_FORM_AUTO, PTMI_FORM_PIXEL, "unknown Streams form", nullptr,
     [](ptmi_ctx *c, int value) {
         if (c->scene.hierarchical() && value == PTMI_FORM_STREAM) return refuse_kind(c, " scene has no stream form (PTMI_FORM_STREAM)");
         return c->opt_form = value, (int)PTMI_OK;
     }},
    {PTMI_OPT_STREAM_BATCH, &ptmi_ctx::opt_batch, 0, 64, "stream batch must be in [0, 64] samples"},
    {PTMI_OPT_SPP_CHUNKS, &ptmi_ctx::opt_spp_chunks, 0, 64, "sample chunks must be in [0, 64]"},
    {PTMI_OPT_ARITHMETIC, &ptmi_ctx::opt_arithmetic, PTMI_ARITH_EXACT, PTMI_ARITH_CONTRACTED, "unknown arithmetic mode"},
    {PTMI_OPT_STREAM_TAIL, nullptr, -1, 1000, "stream tail must be -1 (automatic) or thousandths in [0, 1000]", nullptr,      // the dispatch order's
     [](ptmi_ctx *c, int value) { c->order.tail_option() = value; return (int)PTMI_OK; }, [](ptmi_ctx *c) { return (int64_t)c->order.tail_option(); }},
    {PTMI_OPT_ORDERED_PASSES, &ptmi_ctx::opt_ordered_passes, 0, 64, "ordered passes must be 0 (automatic), 1 (off) or k in [2, 64]"},
    {PTMI_OPT_GLASS_BATCH, &ptmi_ctx::opt_glass_batch, 0, 64, "glass batch must be 0 (automatic), 1 (off) or k in [2, 64] lanes"},
    {PTMI_OPT_STREAM_GRADED, &ptmi_ctx::opt_graded, 0, 1, "graded passes are on (1) or off (0)"},
    {PTMI_OPT_SNAPSHOT_BUDGET_MB, &ptmi_ctx::opt_snapshot_mb, 0, 1 << 20, "snapshot budget must be 0 (automatic) or megabytes in [1, 2^20]"},
    {PTMI_OPT_STREAM_PASS_GROUPS, &ptmi_ctx::opt_pass_groups, 0, 164,
     "pass groups must be 0 (automatic), 1 (every pass on its own), k in [2, 64] or 100 + g, g in [2, 64]", [](int64_t value) { return value > 64 && value < 102; }},
    {PTMI_OPT_CHAIN_SLOTS, &ptmi_ctx::opt_chain_slots, 0, 4096, "chain slots must be 0 (automatic) or in [2, 4096]", [](int64_t value) { return value == 1; }},
    {PTMI_OPT_PASS_HANDOFF, &ptmi_ctx::opt_pass_handoff, PTMI_HANDOFF_FENCED, PTMI_HANDOFF_FENCE_FREE, "unknown pass hand-off"},
    {PTMI_OPT_BVH_DEVICE_BUILD, &ptmi_ctx::opt_bvh_build, PTMI_BVH_BUILD_EQUAL_COUNT, PTMI_BVH_BUILD_SPATIAL, "unknown device build of the sphere hierarchy"},
};
const Option *find_option(int id)
{
    for (const Option &o : kOptions)
        if (o.id == id) return &o;
    return nullptr;
}

}  // namespace

extern "C" {

int ptmi_version(void) { return PTMI_VERSION; }

const char *ptmi_strerror(int code)
{
    switch (code) {
    case PTMI_OK: return "ok";
    case PTMI_EINVAL: return "invalid argument";
    case PTMI_ENODEVICE: return "no usable HIP device";
    case PTMI_EHIP: return "HIP runtime error";
    case PTMI_ENOMEM: return "out of memory";
    case PTMI_ESTATE: return "call order violated";
    case PTMI_ELIMIT: return "scene exceeds PTMI_MAX_PRIMITIVES";
    case PTMI_ESTALE: return "the token names no state this context holds";
    default: return "unknown error";
    }
}

const char *ptmi_last_error(const ptmi_ctx *ctx)
{
    if (!ctx) return g_create_error.c_str();
    if (t_error_of == ctx) return t_error.c_str();             // the caller's own failure: nobody else writes this string
    thread_local std::string copy;                             // a failure another thread saw (a group's member threads): copied under the lock
    std::lock_guard<std::mutex> lock(const_cast<ptmi_ctx *>(ctx)->mu);
    copy = ctx->err;
    return copy.c_str();
}

int ptmi_create(ptmi_ctx **out, int device)
{
    if (!out) return fail(nullptr, PTMI_EINVAL, "out is NULL");
    *out = nullptr;
    int count = 0;
    hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess || count <= 0)
        return fail(nullptr, PTMI_ENODEVICE, std::string("hipGetDeviceCount: ") +
                    (e != hipSuccess ? hipGetErrorString(e) : "0 devices") + " (libptmi has no CPU path)");
    if (device < 0 || device >= count) return fail(nullptr, PTMI_ENODEVICE, "device index out of range");
    ptmi_ctx *c = new (std::nothrow) ptmi_ctx;
    if (!c) return fail(nullptr, PTMI_ENOMEM, "host allocation failed");
    c->device = device;
    static std::atomic<uint64_t> contexts_made{0};
    c->chain.serial = ++contexts_made;
    auto bail = [&](hipError_t err, const char *what) {
        g_create_error = std::string(what) + ": " + hipGetErrorString(err);
        ptmi_destroy(c);                                     // (also takes the error out of the runtime's sticky slot)
        return PTMI_EHIP;
    };
    if ((e = hipSetDevice(device)) != hipSuccess) return bail(e, "hipSetDevice");
    if ((e = hipDeviceGetAttribute(&c->cus, hipDeviceAttributeMultiprocessorCount, device)) != hipSuccess) return bail(e, "hipDeviceGetAttribute");
    {
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) == hipSuccess && total_b) c->device_memory = total_b;
    }
    if ((e = hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking)) != hipSuccess) return bail(e, "hipStreamCreate");
    c->stream = c->own_stream;
    if ((e = hipEventCreateWithFlags(&c->ev_snap, hipEventDisableTiming)) != hipSuccess) return bail(e, "hipEventCreate");
    const char *failed_call = nullptr;
    if ((e = c->stats.create(c->stream, &failed_call)) != hipSuccess) return bail(e, failed_call);
    if ((e = hipStreamSynchronize(c->stream)) != hipSuccess) return bail(e, "hipStreamSynchronize");
    *out = c;
    return PTMI_OK;
}

void ptmi_destroy(ptmi_ctx *c)
{
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->own_stream) (void)hipStreamSynchronize(c->own_stream);
    c->each_block([](DeviceBlock &b) { release(b); });
    c->stream_form.destroy_handles();
    if (c->stats.ev0) (void)hipEventDestroy(c->stats.ev0);
    if (c->stats.ev1) (void)hipEventDestroy(c->stats.ev1);
    if (c->ev_snap) (void)hipEventDestroy(c->ev_snap);
    if (c->own_stream) (void)hipStreamDestroy(c->own_stream);
    (void)hipGetLastError();                                 // whatever failed above was ignored on purpose: it is nobody else's to find
    delete c;
}

int ptmi_set_partition(ptmi_ctx *c, int stripe_rows, int n_parts, int part)
{
    if (!c) return PTMI_EINVAL;
    std::lock_guard<std::mutex> lock(c->mu);
    if (stripe_rows <= 0 || n_parts <= 0 || part < 0 || part >= n_parts)
        return fail(c, PTMI_EINVAL, "bad partition");
    if (c->owned_block.p) return fail(c, PTMI_ESTATE, "ptmi_set_partition must precede ptmi_resize");
    c->stripe_rows = stripe_rows; c->n_parts = n_parts; c->part = part;
    return PTMI_OK;
}

int ptmi_resize(ptmi_ctx *c, int width, int height)
{
    if (!c) return PTMI_EINVAL;
    std::lock_guard<std::mutex> lock(c->mu);
    if (width <= 0 || height <= 0) return fail(c, PTMI_EINVAL, "width and height must be positive");
    if (too_many_pixels(width, height)) return fail(c, PTMI_ELIMIT, "image too large");
    PTMI_HIP(c, hipSetDevice(c->device));
    PTMI_HIP(c, hipStreamSynchronize(c->stream));
    release(c->owned_block);
    c->stream_form.image_resized();
    // The old planes are gone (first: the new ones may need their room).  Until the new ones stand the context is UNSIZED -- a failure below
    // must not leave it pointing into the block just freed: every call that needs planes then answers PTMI_ESTATE.
    c->owned = Planes{};
    c->width = c->height = c->rows_local = 0;
    c->use_bound = false;
    const int rows_local = rows_of_part(height, effective_stripe(c), c->n_parts, c->part);
    const size_t n = (size_t)rows_local * (size_t)width;
    const size_t bytes = planes_bytes(n > 0 ? n : 1);
    DeviceBlock block;
    PTMI_HIP(c, allocate(block, bytes));
    hipError_t e = hipMemsetAsync(block.p, 0, bytes, c->stream);       // ordered before anything launched on the stream
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) { release(block); PTMI_HIP(c, e); }
    c->owned_block = block;
    c->owned = carve(block.p, n > 0 ? n : 1);
    c->width = width; c->height = height; c->rows_local = rows_local;
    return PTMI_OK;
}

int ptmi_local_rows(const ptmi_ctx *cc)
{
    if (!cc) return PTMI_EINVAL;
    ptmi_ctx *c = const_cast<ptmi_ctx *>(cc);
    std::lock_guard<std::mutex> lock(c->mu);
    if (c->width <= 0) return PTMI_ESTATE;
    return c->rows_local;
}

int ptmi_global_row(const ptmi_ctx *cc, int local_row)
{
    if (!cc) return PTMI_EINVAL;
    ptmi_ctx *c = const_cast<ptmi_ctx *>(cc);
    std::lock_guard<std::mutex> lock(c->mu);
    if (c->width <= 0) return PTMI_ESTATE;
    if (local_row < 0 || local_row >= c->rows_local) return PTMI_EINVAL;
    const int s = effective_stripe(c);
    return ((local_row / s) * c->n_parts + c->part) * s + local_row % s;
}

int ptmi_bind_planes(ptmi_ctx *c, float *r, float *g, float *b, uint32_t *sa, uint32_t *sb, uint32_t *sc, uint32_t *sctr)
{
    if (!c) return PTMI_EINVAL;
    std::lock_guard<std::mutex> lock(c->mu);
    if (c->width <= 0) return fail(c, PTMI_ESTATE, "ptmi_resize has not been called");
    const int n_null = !r + !g + !b + !sa + !sb + !sc + !sctr;
    if (n_null == 7) { c->use_bound = false; return PTMI_OK; }
    if (n_null != 0) return fail(c, PTMI_EINVAL, "bind either all seven planes or none");
    c->bound = Planes{r, g, b, sa, sb, sc, sctr};
    c->use_bound = true;
    return PTMI_OK;
}

int ptmi_get_planes(ptmi_ctx *c, float **r, float **g, float **b, uint32_t **sa, uint32_t **sb, uint32_t **sc, uint32_t **sctr)
{
    if (!c) return PTMI_EINVAL;
    std::lock_guard<std::mutex> lock(c->mu);
    if (c->width <= 0) return fail(c, PTMI_ESTATE, "ptmi_resize has not been called");
    const Planes &p = active(c);
    if (r) *r = p.r; if (g) *g = p.g; if (b) *b = p.b;
    if (sa) *sa = p.sa; if (sb) *sb = p.sb; if (sc) *sc = p.sc; if (sctr) *sctr = p.sctr;
    return PTMI_OK;
}

int ptmi_set_stream(ptmi_ctx *c, void *hip_stream)
{
    if (!c) return PTMI_EINVAL;
    std::lock_guard<std::mutex> lock(c->mu);
    PTMI_HIP(c, hipSetDevice(c->device));
    PTMI_HIP(c, hipStreamSynchronize(c->stream));
    c->stream = hip_stream ? static_cast<hipStream_t>(hip_stream) : c->own_stream;
    c->stats.ev_valid = false;
    return PTMI_OK;
}

int ptmi_set_timing(ptmi_ctx *c, int enabled)
{
    if (!c) return PTMI_EINVAL;
    std::lock_guard<std::mutex> lock(c->mu);
    c->stats.timing = enabled != 0;
    c->stats.ev_valid = false;
    return PTMI_OK;
}

int ptmi_set_variant(ptmi_ctx *c, int variant)
{
    if (!c) return PTMI_EINVAL;
    std::lock_guard<std::mutex> lock(c->mu);
    if (variant < 0 || variant >= kVariantCount) return fail(c, PTMI_EINVAL, "unknown variant");
    if (!variant_available(variant)) return fail(c, PTMI_EINVAL, "this variant is an ablation kernel: build libptmi with -DPTMI_ABLATIONS");
    if (c->scene.hierarchical() && variant != kVariantAuto) return refuse_kind(c, " scene renders through the default kernels only (variant 0)");
    c->variant = variant;
    return PTMI_OK;
}

int ptmi_set_option(ptmi_ctx *c, int option, int64_t value)
{
    if (!c) return PTMI_EINVAL;
    std::lock_guard<std::mutex> lock(c->mu);
    const Option *o = find_option(option);
    if (!o) return fail(c, PTMI_EINVAL, "unknown option");
    if (value < o->lo || value > o->hi || (o->but && o->but(value))) return fail(c, PTMI_EINVAL, o->refusal);
    if (o->set) return o->set(c, (int)value);
    c->*o->member = (int)value;
    return PTMI_OK;
}

int ptmi_get_option(ptmi_ctx *c, int option, int64_t *value)
{
    if (!c) return PTMI_EINVAL;
    std::lock_guard<std::mutex> lock(c->mu);
    if (!value) return fail(c, PTMI_EINVAL, "value is NULL");
    const Option *o = find_option(option);
    if (!o) return fail(c, PTMI_EINVAL, "unknown option");
    *value = o->get ? o->get(c) : c->*o->member;
    return PTMI_OK;
}

static int seed_common(ptmi_ctx *c, uint64_t seed0, bool clear)
{
    if (!c) return PTMI_EINVAL;
    std::lock_guard<std::mutex> lock(c->mu);
    if (c->width <= 0) return fail(c, PTMI_ESTATE, "ptmi_resize has not been called");
    PTMI_HIP(c, hipSetDevice(c->device));
    PTMI_HIP(c, launch_seed(active(c), c->width, c->rows_local, effective_stripe(c), c->n_parts, c->part,
                            seed0, clear, c->stream));
    return PTMI_OK;
}

int ptmi_init_output(ptmi_ctx *c, uint64_t seed0) { return seed_common(c, seed0, true); }
int ptmi_reseed(ptmi_ctx *c, uint64_t seed0) { return seed_common(c, seed0, false); }

int ptmi_create_with(ptmi_ctx *c, const uint32_t *w0, const uint32_t *w1, const uint32_t *w2)
{
    if (!c) return PTMI_EINVAL;
    std::lock_guard<std::mutex> lock(c->mu);
    if (c->width <= 0) return fail(c, PTMI_ESTATE, "ptmi_resize has not been called");
    if (!w0 || !w1 || !w2) return fail(c, PTMI_EINVAL, "word planes are NULL");
    PTMI_HIP(c, hipSetDevice(c->device));
    const size_t n = (size_t)c->rows_local * c->width;
    if (int rc = grow(c, c->scratch, 3 * n * 4, "scratch")) return rc;
    uint32_t *d = c->scratch.as<uint32_t>();
    PTMI_HIP(c, hipStreamSynchronize(c->stream));
    const CopySpan words[3] = {{d, const_cast<uint32_t *>(w0), n * 4}, {d + n, const_cast<uint32_t *>(w1), n * 4},
                               {d + 2 * n, const_cast<uint32_t *>(w2), n * 4}};
    PTMI_HIP(c, copy_to_device(c, words, 3));
    PTMI_HIP(c, launch_create_with(active(c), d, d + n, d + 2 * n, (int64_t)n, c->stream));
    PTMI_HIP(c, hipStreamSynchronize(c->stream));
    return PTMI_OK;
}

// The active planes from (upload) or into seven host planes; a null pointer: that plane stays as it is, or is not asked for
static int copy_state(ptmi_ctx *c, bool upload, const void *const host[7])
{
    if (!c) return PTMI_EINVAL;
    std::lock_guard<std::mutex> lock(c->mu);
    if (c->width <= 0) return fail(c, PTMI_ESTATE, "ptmi_resize has not been called");
    PTMI_HIP(c, hipSetDevice(c->device));
    PTMI_HIP(c, hipStreamSynchronize(c->stream));
    CopySpan spans[7];
    const int n_spans = plane_spans(active(c), host, (size_t)c->rows_local * c->width, spans);
    if (!upload) PTMI_HIP(c, copy_to_host(c, spans, n_spans));
    else {
        PTMI_HIP(c, copy_to_device(c, spans, n_spans));
        PTMI_HIP(c, hipStreamSynchronize(c->stream));
    }
    return PTMI_OK;
}

int ptmi_upload_state(ptmi_ctx *c, const float *r, const float *g, const float *b, const uint32_t *sa, const uint32_t *sb, const uint32_t *sc, const uint32_t *sctr)
{
    const void *const src[7] = {r, g, b, sa, sb, sc, sctr};
    return copy_state(c, true, src);
}
int ptmi_download_state(ptmi_ctx *c, float *r, float *g, float *b, uint32_t *sa, uint32_t *sb, uint32_t *sc, uint32_t *sctr)
{
    const void *const dst[7] = {r, g, b, sa, sb, sc, sctr};
    return copy_state(c, false, dst);
}
int ptmi_download_color(ptmi_ctx *c, float *r, float *g, float *b) { return ptmi_download_state(c, r, g, b, nullptr, nullptr, nullptr, nullptr); }

int ptmi_render(ptmi_ctx *c, const ptmi_camera *camera, int algorithm, int bounce_limit, int n_spp)
{
    if (!c) return PTMI_EINVAL;
    std::lock_guard<std::mutex> lock(c->mu);
    if (int rc = check_render_args(c, camera, algorithm, bounce_limit, n_spp)) return rc;
    if (c->width <= 0) return fail(c, PTMI_ESTATE, "ptmi_resize has not been called");
    PTMI_HIP(c, hipSetDevice(c->device));
    const RenderTarget resident{active(c), c->width, c->height, c->rows_local, effective_stripe(c), c->n_parts, c->part, nullptr, nullptr};
    return launch_render(c, resident, camera, algorithm, bounce_limit, n_spp);
}

/* 1 when ptmi_render with this algorithm returns only after device work it waits for (the stream form with a ray-splitting
 * scene or unordered items reads its overflow counters back), 0 when it only enqueues.  ptmi_group_render gives such members a
 * host thread each. */
int ptmi_render_blocks(ptmi_ctx *c, int algorithm)
{
    if (!c) return PTMI_EINVAL;
    std::lock_guard<std::mutex> lock(c->mu);
    const bool stream_form = uses_stream_form(c, algorithm, c->n_parts, -1);        // (for some sample count: the automatic choice looks at it)
    const bool ordered = !c->scene.has_glass && (c->opt_batch == 0 || effective_seed_rule(c) == PTMI_SEED_FROM_RESULT);
    return stream_form && !ordered ? 1 : 0;
}

int ptmi_synchronize(ptmi_ctx *c)
{
    if (!c) return PTMI_EINVAL;
    std::lock_guard<std::mutex> lock(c->mu);
    PTMI_HIP(c, hipSetDevice(c->device));
    PTMI_HIP(c, hipStreamSynchronize(c->stream));
    return PTMI_OK;
}

int ptmi_render1(ptmi_ctx *c, const ptmi_camera *camera, int algorithm, int bounce_limit,
                 int width, int height, const int64_t *screen_x, const int64_t *screen_y,
                 const float *r_in, const float *g_in, const float *b_in,
                 const uint32_t *sa_in, const uint32_t *sb_in, const uint32_t *sc_in, const uint32_t *sctr_in,
                 float *r_out, float *g_out, float *b_out,
                 uint32_t *sa_out, uint32_t *sb_out, uint32_t *sc_out, uint32_t *sctr_out)
{
    if (!c) return PTMI_EINVAL;
    std::lock_guard<std::mutex> lock(c->mu);
    if (int rc = check_render_args(c, camera, algorithm, bounce_limit, 1)) return rc;
    if (width <= 0 || height <= 0) return fail(c, PTMI_EINVAL, "width and height must be positive");
    if (too_many_pixels(width, height)) return fail(c, PTMI_ELIMIT, "image too large");
    if (!r_in || !g_in || !b_in || !sa_in || !sb_in || !sc_in || !sctr_in ||
        !r_out || !g_out || !b_out || !sa_out || !sb_out || !sc_out || !sctr_out)
        return fail(c, PTMI_EINVAL, "a plane pointer is NULL");
    if ((screen_x == nullptr) != (screen_y == nullptr)) return fail(c, PTMI_EINVAL, "give both screen planes or neither");
    if (screen_x && algorithm == PTMI_STREAMS) return fail(c, PTMI_EINVAL, "Streams takes the implicit screen only");
    PTMI_HIP(c, hipSetDevice(c->device));
    const size_t n = (size_t)width * height;
    const size_t pb = planes_bytes(n);
    const size_t sb = screen_x ? 2 * n * sizeof(int64_t) : 0;
    if (int rc = grow(c, c->scratch, pb + sb, "scratch")) return rc;
    Planes p = carve(c->scratch.p, n);
    int64_t *dsx = screen_x ? reinterpret_cast<int64_t *>(c->scratch.as<char>() + pb) : nullptr;
    int64_t *dsy = screen_x ? dsx + n : nullptr;
    PTMI_HIP(c, hipStreamSynchronize(c->stream));
    const void *const src[7] = {r_in, g_in, b_in, sa_in, sb_in, sc_in, sctr_in};       // (none of the fourteen is null: refused above)
    const void *const dst[7] = {r_out, g_out, b_out, sa_out, sb_out, sc_out, sctr_out};
    CopySpan in[9];
    plane_spans(p, src, n, in);
    if (screen_x) {
        in[7] = CopySpan{dsx, const_cast<int64_t *>(screen_x), n * sizeof(int64_t)};
        in[8] = CopySpan{dsy, const_cast<int64_t *>(screen_y), n * sizeof(int64_t)};
    }
    PTMI_HIP(c, copy_to_device(c, in, screen_x ? 9 : 7));
    if (int rc = launch_render(c, RenderTarget::whole(p, width, height, dsx, dsy), camera, algorithm, bounce_limit, 1)) return rc;
    CopySpan out[7];
    plane_spans(p, dst, n, out);
    PTMI_HIP(c, copy_to_host(c, out, 7));           // stream-ordered behind the kernel; returns with the planes filled
    return PTMI_OK;
}

int ptmi_present(ptmi_ctx *c, int iterations, float *rgb32f_out, uint8_t *rgba8_out)
{
    if (!c) return PTMI_EINVAL;
    std::lock_guard<std::mutex> lock(c->mu);
    if (c->width <= 0) return fail(c, PTMI_ESTATE, "ptmi_resize has not been called");
    if (iterations <= 0) return fail(c, PTMI_EINVAL, "iterations must be positive");
    if (!rgb32f_out && !rgba8_out) return PTMI_OK;
    PTMI_HIP(c, hipSetDevice(c->device));
    const size_t n = (size_t)c->rows_local * c->width;
    if (n == 0) return PTMI_OK;
    const size_t rgb_bytes = ((n * 12 + 255) / 256) * 256;
    if (int rc = grow(c, c->scratch, rgb_bytes + n * 4, "scratch")) return rc;
    float *d_rgb = c->scratch.as<float>();
    uint32_t *d_rgba = reinterpret_cast<uint32_t *>(c->scratch.as<char>() + rgb_bytes);
    PTMI_HIP(c, launch_present(active(c), (long long)n, iterations, rgb32f_out ? d_rgb : nullptr,
                               rgba8_out ? d_rgba : nullptr, c->stream));
    CopySpan out[2];
    int n_out = 0;
    if (rgb32f_out) out[n_out++] = CopySpan{d_rgb, rgb32f_out, n * 12};
    if (rgba8_out) out[n_out++] = CopySpan{d_rgba, rgba8_out, n * 4};
    PTMI_HIP(c, copy_to_host(c, out, n_out));
    return PTMI_OK;
}

int ptmi_snapshot_color(ptmi_ctx *c, float *dst_device, void *hip_stream)
{
    if (!c) return PTMI_EINVAL;
    std::lock_guard<std::mutex> lock(c->mu);
    if (c->width <= 0) return fail(c, PTMI_ESTATE, "ptmi_resize has not been called");
    if (!dst_device) return fail(c, PTMI_EINVAL, "dst_device is NULL");
    PTMI_HIP(c, hipSetDevice(c->device));
    const size_t bytes = (size_t)c->rows_local * c->width * 4;
    hipStream_t s = hip_stream ? static_cast<hipStream_t>(hip_stream) : c->stream;
    if (s != c->stream) {                                      // order the copy behind the renders already issued
        PTMI_HIP(c, hipEventRecord(c->ev_snap, c->stream));
        PTMI_HIP(c, hipStreamWaitEvent(s, c->ev_snap, 0));
    }
    Planes &p = active(c);
    const float *src[3] = {p.r, p.g, p.b};
    for (int k = 0; k < 3 && bytes; ++k)
        PTMI_HIP(c, hipMemcpyAsync(reinterpret_cast<char *>(dst_device) + (size_t)k * bytes, src[k], bytes, hipMemcpyDeviceToDevice, s));
    return PTMI_OK;
}

int ptmi_get_stats(ptmi_ctx *c, ptmi_stats *out)
{
    if (!c) return PTMI_EINVAL;
    std::lock_guard<std::mutex> lock(c->mu);
    if (!out) return fail(c, PTMI_EINVAL, "out is NULL");
    PTMI_HIP(c, hipSetDevice(c->device));
    PTMI_HIP(c, hipStreamSynchronize(c->stream));
    return c->stats.read(c, out);
}

int ptmi_debug_counters_n(ptmi_ctx *c, uint32_t *out, int capacity)
{
    if (!c) return PTMI_EINVAL;
    std::lock_guard<std::mutex> lock(c->mu);
    if (!out) return fail(c, PTMI_EINVAL, "out is NULL");
    if (capacity < 0) return fail(c, PTMI_EINVAL, "capacity is negative");
    const int words = capacity < kWorkWords ? capacity : kWorkWords;
    PTMI_HIP(c, hipSetDevice(c->device));
    if (words > 0) PTMI_HIP(c, hipMemcpyAsync(out, c->stats.block[RenderStats::Work].p, (size_t)words * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    PTMI_HIP(c, hipStreamSynchronize(c->stream));
    return words;
}

int ptmi_debug_counters(ptmi_ctx *c, uint32_t out[64])
{
    const int rc = ptmi_debug_counters_n(c, out, 64);
    return rc < 0 ? rc : PTMI_OK;
}

int ptmi_reset_stats(ptmi_ctx *c)
{
    if (!c) return PTMI_EINVAL;
    std::lock_guard<std::mutex> lock(c->mu);
    PTMI_HIP(c, hipSetDevice(c->device));
    PTMI_HIP(c, hipStreamSynchronize(c->stream));
    if (int rc = c->stats.reset(c)) return rc;
    c->stream_form.reset_totals();
    return PTMI_OK;
}

static int eval_prims(ptmi_ctx *c, const void *prims, int words, const float *rays, int n,
                      int32_t *is_just, float *t, float *normalp, bool sphere)
{
    if (!c) return PTMI_EINVAL;
    std::lock_guard<std::mutex> lock(c->mu);
    if (n < 0 || (n > 0 && (!prims || !rays || !is_just || !t))) return fail(c, PTMI_EINVAL, "bad point-query arguments");
    if (n == 0) return PTMI_OK;
    PTMI_HIP(c, hipSetDevice(c->device));
    const size_t nb = (size_t)n;
    const size_t bytes = nb * (words * 4 + 6 * 4 + 4 + 4 + 6 * 4);
    if (int rc = grow(c, c->scratch, bytes, "scratch")) return rc;
    float *d_prims = c->scratch.as<float>();
    float *d_rays = d_prims + nb * words;
    int32_t *d_just = reinterpret_cast<int32_t *>(d_rays + nb * 6);
    float *d_t = reinterpret_cast<float *>(d_just + nb);
    float *d_np = d_t + nb;
    PTMI_HIP(c, hipStreamSynchronize(c->stream));
    PTMI_HIP(c, hipMemcpyAsync(d_prims, prims, nb * words * 4, hipMemcpyHostToDevice, c->stream));
    PTMI_HIP(c, hipMemcpyAsync(d_rays, rays, nb * 6 * 4, hipMemcpyHostToDevice, c->stream));
    if (sphere) PTMI_HIP(c, launch_eval_sphere(d_prims, d_rays, n, d_just, d_t, d_np, c->stream));
    else        PTMI_HIP(c, launch_eval_plane(d_prims, d_rays, n, d_just, d_t, d_np, c->stream));
    PTMI_HIP(c, hipStreamSynchronize(c->stream));
    PTMI_HIP(c, hipMemcpyAsync(is_just, d_just, nb * 4, hipMemcpyDeviceToHost, c->stream));
    PTMI_HIP(c, hipMemcpyAsync(t, d_t, nb * 4, hipMemcpyDeviceToHost, c->stream));
    if (normalp) PTMI_HIP(c, hipMemcpyAsync(normalp, d_np, nb * 24, hipMemcpyDeviceToHost, c->stream));
    PTMI_HIP(c, hipStreamSynchronize(c->stream));
    return PTMI_OK;
}

int ptmi_eval_distance_to_sphere(ptmi_ctx *c, const ptmi_sphere *spheres, const float *rays, int n,
                                 int32_t *is_just, float *t, float *hit_normalp)
{
    return eval_prims(c, spheres, 10, rays, n, is_just, t, hit_normalp, true);
}

int ptmi_eval_distance_to_plane(ptmi_ctx *c, const ptmi_plane *planes, const float *rays, int n,
                                int32_t *is_just, float *t, float *hit_normalp)
{
    return eval_prims(c, planes, 12, rays, n, is_just, t, hit_normalp, false);
}

int ptmi_eval_check_hit(ptmi_ctx *c, const float *rays, int n, float *t_out, int32_t *idx_out, int32_t *just_out)
{
    if (!c) return PTMI_EINVAL;
    std::lock_guard<std::mutex> lock(c->mu);
    if (n < 0 || (n > 0 && (!rays || !t_out || !idx_out || !just_out))) return fail(c, PTMI_EINVAL, "bad point-query arguments");
    if (!c->scene.packed.p) return fail(c, PTMI_ESTATE, "ptmi_set_scene has not been called");
    if (n == 0) return PTMI_OK;
    PTMI_HIP(c, hipSetDevice(c->device));
    const size_t nb = (size_t)n;
    if (int rc = grow(c, c->scratch, nb * (6 * 4 + 3 * 4), "scratch")) return rc;
    float *d_rays = c->scratch.as<float>();
    float *d_t = d_rays + nb * 6;
    int32_t *d_idx = reinterpret_cast<int32_t *>(d_t + nb), *d_just = d_idx + nb;
    PTMI_HIP(c, hipStreamSynchronize(c->stream));
    PTMI_HIP(c, hipMemcpyAsync(d_rays, rays, nb * 6 * 4, hipMemcpyHostToDevice, c->stream));
    const RayCallScene r = ray_call_scene(c);
    if (r.mesh) PTMI_HIP(c, launch_eval_check_hit_mesh(r.scene, *r.mesh, d_rays, n, d_t, d_idx, d_just, c->stream));
    else PTMI_HIP(c, launch_eval_check_hit(r.scene, r.bvh, d_rays, n, d_t, d_idx, d_just, c->stream));
    PTMI_HIP(c, hipMemcpyAsync(t_out, d_t, nb * 4, hipMemcpyDeviceToHost, c->stream));
    PTMI_HIP(c, hipMemcpyAsync(idx_out, d_idx, nb * 4, hipMemcpyDeviceToHost, c->stream));
    PTMI_HIP(c, hipMemcpyAsync(just_out, d_just, nb * 4, hipMemcpyDeviceToHost, c->stream));
    PTMI_HIP(c, hipStreamSynchronize(c->stream));
    return PTMI_OK;
}

// The ray queries on the caller's device arrays: refusals first (nothing enqueued, nothing written), then one launch on the context's
// stream -- no synchronisation, no allocation, no scratch.
int ptmi_trace_rays_device(ptmi_ctx *c, const float *d_rays, int n, float *d_t, int32_t *d_idx, float *d_hit)
{
    if (!c) return PTMI_EINVAL;
    std::lock_guard<std::mutex> lock(c->mu);
    if (n < 0 || (n > 0 && (!d_rays || !d_t || !d_idx))) return fail(c, PTMI_EINVAL, "bad ray-query arguments");
    if (!c->scene.packed.p) return fail(c, PTMI_ESTATE, "ptmi_set_scene has not been called");
    if (n == 0) return PTMI_OK;
    PTMI_HIP(c, hipSetDevice(c->device));
    const RayCallScene r = ray_call_scene(c);
    PTMI_HIP(c, launch_trace_rays(r.scene, r.bvh, r.mesh, d_rays, n, d_t, d_idx, d_hit, c->stream));
    return PTMI_OK;
}

int ptmi_occluded_device(ptmi_ctx *c, const float *d_rays, const float *d_t_max, int n, int32_t *d_occluded)
{
    if (!c) return PTMI_EINVAL;
    std::lock_guard<std::mutex> lock(c->mu);
    if (n < 0 || (n > 0 && (!d_rays || !d_t_max || !d_occluded))) return fail(c, PTMI_EINVAL, "bad ray-query arguments");
    if (!c->scene.packed.p) return fail(c, PTMI_ESTATE, "ptmi_set_scene has not been called");
    if (n == 0) return PTMI_OK;
    PTMI_HIP(c, hipSetDevice(c->device));
    const RayCallScene r = ray_call_scene(c);
    PTMI_HIP(c, launch_occluded(r.scene, r.bvh, r.mesh, c->scene.sphere_reach, d_rays, d_t_max, n, d_occluded, c->stream));
    return PTMI_OK;
}

// ... and through an index: the plain entries' refusals, then the index's
int ptmi_trace_rays_indexed_device(ptmi_ctx *c, const float *d_rays, int n, const int32_t *d_index, int m, float *d_t, int32_t *d_idx, float *d_hit)
{
    if (!c) return PTMI_EINVAL;
    std::lock_guard<std::mutex> lock(c->mu);
    if (n < 0 || (n > 0 && (!d_rays || !d_t || !d_idx)) || m < 0 || (m > 0 && !d_index)) return fail(c, PTMI_EINVAL, "bad ray-query arguments");
    if (!c->scene.packed.p) return fail(c, PTMI_ESTATE, "ptmi_set_scene has not been called");
    if (n == 0 || m == 0) return PTMI_OK;
    PTMI_HIP(c, hipSetDevice(c->device));
    const RayCallScene r = ray_call_scene(c);
    PTMI_HIP(c, launch_trace_rays_indexed(r.scene, r.bvh, r.mesh, d_rays, n, d_index, m, d_t, d_idx, d_hit, c->stream));
    return PTMI_OK;
}

int ptmi_occluded_indexed_device(ptmi_ctx *c, const float *d_rays, const float *d_t_max, int n, const int32_t *d_index, int m, int32_t *d_occluded)
{
    if (!c) return PTMI_EINVAL;
    std::lock_guard<std::mutex> lock(c->mu);
    if (n < 0 || (n > 0 && (!d_rays || !d_t_max || !d_occluded)) || m < 0 || (m > 0 && !d_index)) return fail(c, PTMI_EINVAL, "bad ray-query arguments");
    if (!c->scene.packed.p) return fail(c, PTMI_ESTATE, "ptmi_set_scene has not been called");
    if (n == 0 || m == 0) return PTMI_OK;
    PTMI_HIP(c, hipSetDevice(c->device));
    const RayCallScene r = ray_call_scene(c);
    PTMI_HIP(c, launch_occluded_indexed(r.scene, r.bvh, r.mesh, c->scene.sphere_reach, d_rays, d_t_max, n, d_index, m,
                                        d_occluded, c->stream));
    return PTMI_OK;
}

// Paths along the caller's rays: the ray queries' refusals and render Inline's (a GLASS material), then one launch.  The context's state
// planes, partition, camera and statistics are not touched.
static int trace_paths(ptmi_ctx *c, const float *d_rays, int n, const int32_t *d_index, int m, bool indexed, int bounce_limit, int n_spp, float *d_color,
                       uint32_t *d_seed)
{
    if (!c) return PTMI_EINVAL;
    std::lock_guard<std::mutex> lock(c->mu);
    if (n < 0 || (n > 0 && (!d_rays || !d_color || !d_seed)) || (indexed && (m < 0 || (m > 0 && !d_index)))) return fail(c, PTMI_EINVAL, "bad ray-path arguments");
    if (!c->scene.packed.p) return fail(c, PTMI_ESTATE, "ptmi_set_scene has not been called");
    if (c->scene.has_glass) return fail(c, PTMI_EINVAL, "the scene holds a GLASS material: render Inline cannot split rays, use PTMI_STREAMS");
    if (n == 0 || n_spp <= 0 || (indexed && m == 0)) return PTMI_OK;
    PTMI_HIP(c, hipSetDevice(c->device));
    const RayCallScene r = ray_call_scene(c);
    PTMI_HIP(c, launch_trace_paths(r.scene, r.bvh, r.mesh, d_rays, n, indexed ? d_index : nullptr, m, bounce_limit, n_spp, d_color, d_seed, c->stream));
    return PTMI_OK;
}

int ptmi_path_seeds_device(ptmi_ctx *c, uint64_t seed0, uint64_t first_index, int n, uint32_t *d_seed)
{
    if (!c) return PTMI_EINVAL;
    std::lock_guard<std::mutex> lock(c->mu);
    if (n < 0 || (n > 0 && !d_seed)) return fail(c, PTMI_EINVAL, "bad ray-path arguments");
    if (n == 0) return PTMI_OK;
    PTMI_HIP(c, hipSetDevice(c->device));
    PTMI_HIP(c, launch_path_seeds(seed0, first_index, n, d_seed, c->stream));
    return PTMI_OK;
}

int ptmi_trace_paths_device(ptmi_ctx *c, const float *d_rays, int n, int bounce_limit, int n_spp, float *d_color, uint32_t *d_seed)
{
    return trace_paths(c, d_rays, n, nullptr, 0, false, bounce_limit, n_spp, d_color, d_seed);
}

int ptmi_trace_paths_indexed_device(ptmi_ctx *c, const float *d_rays, int n, const int32_t *d_index, int m, int bounce_limit, int n_spp, float *d_color,
                                    uint32_t *d_seed)
{
    return trace_paths(c, d_rays, n, d_index, m, true, bounce_limit, n_spp, d_color, d_seed);
}

int ptmi_eval_sincos(ptmi_ctx *c, const float *x, int n, float *sin_out, float *cos_out)
{
    if (!c) return PTMI_EINVAL;
    std::lock_guard<std::mutex> lock(c->mu);
    if (n < 0 || (n > 0 && (!x || !sin_out || !cos_out))) return fail(c, PTMI_EINVAL, "bad sincos arguments");
    if (n == 0) return PTMI_OK;
    PTMI_HIP(c, hipSetDevice(c->device));
    const size_t nb = (size_t)n;
    if (int rc = grow(c, c->scratch, nb * 12, "scratch")) return rc;
    float *dx = c->scratch.as<float>(), *ds = dx + nb, *dc = ds + nb;
    PTMI_HIP(c, hipStreamSynchronize(c->stream));
    PTMI_HIP(c, hipMemcpyAsync(dx, x, nb * 4, hipMemcpyHostToDevice, c->stream));
    PTMI_HIP(c, launch_eval_sincos(dx, n, ds, dc, c->stream));
    PTMI_HIP(c, hipStreamSynchronize(c->stream));
    PTMI_HIP(c, hipMemcpyAsync(sin_out, ds, nb * 4, hipMemcpyDeviceToHost, c->stream));
    PTMI_HIP(c, hipMemcpyAsync(cos_out, dc, nb * 4, hipMemcpyDeviceToHost, c->stream));
    PTMI_HIP(c, hipStreamSynchronize(c->stream));
    return PTMI_OK;
}

int ptmi_eval_quaternion(ptmi_ctx *c, const float *half_angles, int n, float *q_out)
{
    if (!c) return PTMI_EINVAL;
    std::lock_guard<std::mutex> lock(c->mu);
    if (n < 0 || (n > 0 && (!half_angles || !q_out))) return fail(c, PTMI_EINVAL, "bad quaternion arguments");
    if (n == 0) return PTMI_OK;
    PTMI_HIP(c, hipSetDevice(c->device));
    const size_t nb = (size_t)n;
    if (int rc = grow(c, c->scratch, nb * 28, "scratch")) return rc;
    float *da = c->scratch.as<float>(), *dq = da + nb * 3;
    PTMI_HIP(c, hipStreamSynchronize(c->stream));
    PTMI_HIP(c, hipMemcpyAsync(da, half_angles, nb * 12, hipMemcpyHostToDevice, c->stream));
    PTMI_HIP(c, launch_eval_quaternion(da, n, dq, c->stream));
    PTMI_HIP(c, hipStreamSynchronize(c->stream));
    PTMI_HIP(c, hipMemcpyAsync(q_out, dq, nb * 16, hipMemcpyDeviceToHost, c->stream));
    PTMI_HIP(c, hipStreamSynchronize(c->stream));
    return PTMI_OK;
}

}  // extern "C"
