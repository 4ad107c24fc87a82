// ptmi_order.cpp -- the cost-ordered dispatch of the tiled kernels (DispatchOrder, ptmi_ctx.h): its blocks, its key, the schedule of its
// rebuilds and the launch of the order kernel.  launch_render (ptmi_api.cpp) decides which calls are ordered; the kernels that read the
// order and add their costs are the per-pixel ones and the stream form's (ptmi_device.h: lane_pixel); the order kernel is ptmi_small.hip's.
#include "ptmi_ctx.h"

#include <algorithm>

using namespace ptmi;

// The schedule of the cost-ordered dispatch: `launches` = launches made so far with one (camera, scene, shape, limit, algorithm).
// The order is REBUILT from the recorded costs before launch 1, 2, 4, 8, ... -- and never again once the limit is reached: the state stops
// there, it is a power of two itself, and a rebuild bumps the order's generation, which would make the stream form re-run its primary kernel
// on every later call of a standing camera.  A launch RECORDS its costs only if the NEXT launch rebuilds -- launch 0, 1, 3, 7, 15, ... (the
// sums stay far from 2^32) -- since round 5: a recorded cost is an atomic per wave, or per item in the stream form, on words that all XCDs share
// (32 bytes of write traffic each, tools/traffic_terms.py), and between two rebuilds nobody reads them; every rebuild still sees one more
// launch than the one before it, and a standing camera's steady state records nothing.
extern "C" int ptmi_order_schedule(int launches, int stream_form, int *rebuild, int *record)
{
    const int limit = stream_form ? (1 << 11) : (1 << 20);
    const bool below = launches >= 0 && launches < limit;
    if (rebuild) *rebuild = (below && launches > 0 && (launches & (launches - 1)) == 0) ? 1 : 0;
    if (record) *record = (below && launches + 1 < limit && ((launches + 1) & launches) == 0) ? 1 : 0;
    return below ? launches + 1 : limit;
}

// Launches with one (camera, scene, shape, limit, algorithm) record what every quad of tiles costs; later launches with the same key
// dispatch the most expensive quads first (sorted on the device).  Everything is enqueued on the stream; results do not depend on it.
// (The stream form orders its start-hit list the same way, as algorithm 2 of the key; its items record their costs.)
int DispatchOrder::before_launches(ptmi_ctx *c, const ptmi_camera &camera, uint64_t scene_version, const RenderTarget &target, int bounce_limit, int algorithm,
                                   bool stream_form, RenderArgs &a)
{
    const unsigned int n_quads = quad_positions(target.width, target.rows_local);
    const size_t quad_bytes = n_quads * sizeof(unsigned int);
    DeviceBlock *quads[3] = {&d_quad_cost, &d_quad_order, &d_quad_class};
    if (std::any_of(quads, quads + 3, [&](const DeviceBlock *q) { return q->bytes < quad_bytes; })) {
        launches = 0; ++generation_;
        for (DeviceBlock *q : quads)
            if (int rc = grow(c, *q, quad_bytes, "the dispatch order")) return rc;
    }
    Key now{};
    now.cam = camera; now.scene_version = scene_version;
    const int dims[8] = {target.width, target.height, target.rows_local, target.stripe_rows, target.n_parts, target.part, bounce_limit, stream_form ? 2 : algorithm};
    std::memcpy(now.dims, dims, sizeof dims);
    if (std::memcmp(&now, &key, sizeof now) != 0) { key = now; launches = 0; ++generation_; }
    // `launches` counts the launches made with this key.  The launches before a rebuild add their costs (a 1-spp launch says little
    // on its own: the compat entry renders one sample per call); the order is rebuilt before launch 1, 2, 4, 8, ...
    int rebuild = 0, record = 0;
    launches_after = ptmi_order_schedule(launches, stream_form ? 1 : 0, &rebuild, &record);       // (every launch counts, whether or not it records)
    if (int rc = grow(c, d_tail_start, 64, "the tail's start")) return rc;
    if (launches == 0) {
        PTMI_HIP(c, hipMemsetAsync(d_quad_cost.p, 0, quad_bytes, c->stream));
        PTMI_HIP(c, hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(d_tail_start.p), (int)n_quads, 1, c->stream));   // no tail yet
    } else if (rebuild) {
        // (the stream form: the order kernel also says where the order's cheap end begins -- render_streams_wavefront.  How much of the
        // recorded cost that end may hold: 15 % where a lane sees four pixels or more, 40 % where it sees fewer -- 1280x720 / 64 spp: 2.34 ms
        // with 15 %, 2.16 with 40 %, chain kernel 1.96; 1080p: 4.24 / 4.21.)
        const unsigned long long lanes_full = 64ull * (unsigned long long)(c->cus > 0 ? c->cus : 256) * 4ull * (unsigned long long)streams_pixels_waves();
        const unsigned int permille = tail_permille >= 0 ? (unsigned int)tail_permille
                                    : ((unsigned long long)target.width * (unsigned long long)target.rows_local < 4ull * lanes_full ? 400u : 150u);
        PTMI_HIP(c, launch_quad_order(d_quad_cost.as<unsigned int>(), d_quad_order.as<unsigned int>(), d_quad_class.as<unsigned int>(), n_quads,
                                      stream_form ? d_tail_start.as<unsigned int>() : nullptr, permille, c->stream));
        ++generation_;
    }
    if (launches > 0) a.quad_order = d_quad_order.as<unsigned int>();
    if (record) a.quad_cost = d_quad_cost.as<unsigned int>();
    return PTMI_OK;
}
