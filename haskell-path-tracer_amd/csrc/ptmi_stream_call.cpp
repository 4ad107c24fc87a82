// ptmi_stream_call.cpp -- the host side of `render Streams` in its stream ("wavefront") form: the pass schedules, one call's steps (StreamCall) and what the form
// keeps between calls (StreamFormState, ptmi_ctx.h).  launch_render (ptmi_api.cpp) decides whether a call takes this form and whether in a dispatch order (DispatchOrder,
// ptmi_order.cpp: its generation keys the start-hit list, its tail word is where the per-pixel tail begins); the kernels are ptmi_stream_*.hip.
#include "ptmi_ctx.h"

#include <algorithm>

using namespace ptmi;

namespace {

constexpr int kGlassBatchDefault = 1;      // PTMI_OPT_GLASS_BATCH = 0 (automatic): parking off -- see the measurements in DESIGN.md 5.5

RayQueue carve_queue(void *block, size_t capacity, int which)
{
    RayQueue q;
    q.base = static_cast<uint32_t *>(block) + (size_t)which * kRayQueueWords * capacity;
    q.capacity = (unsigned int)capacity;
    return q;
}

// The passes of the stream form's split kernel: which samples of its pixels pass p renders (first[p] .. first[p + 1]).
// A pass is one item per start hit, taken by whatever lane is free, and the launch ends as its LAST items do: with uniform
// passes of 16 samples the waves of a 1080p / 64-spp glass launch ended anywhere between 75 % and 98 % of it (a wave holds 64
// items of very different weight when the tickets run out) -- an eighth of the chip's wave-time idle.  So the passes are GRADED
// (guided self-scheduling): at most `per_item` samples -- the size that gives a lane its ~16 items -- and never more than a
// fraction of what is still to come, chosen so that an item five times the mean weight, taken when its pass begins, is over
// before the remaining passes are: the last passes are a few samples (not fewer than a floor: below), and the end of the launch is as long as their trees.
// Which sample belongs to which pass changes no seed (snapshots) and no ray; only the order of a pixel's float additions,
// which the stream form with GLASS does not define anyway.  Returns the number of passes (<= kMaxStreamPasses).
constexpr int kMaxStreamPasses = 64;
constexpr int kMaxStreamRaysPerPixel = 64;   // PTMI_OPT_STREAM_CAPACITY's upper end, and how far a call grows its overflow streams before it counts drops
int stream_schedule(int n_spp, unsigned long long n_px, unsigned long long lanes, int batch, bool graded, int first[kMaxStreamPasses + 1])
{
    first[0] = 0;
    if (n_spp <= 0 || n_px == 0 || lanes == 0) { first[1] = n_spp > 0 ? n_spp : 0; return 1; }
    int per_item = batch;
    if (per_item <= 0) {                                      // a lane should see ~16 items
        const double items_wanted = 16.0 * (double)lanes;
        int passes = (int)(items_wanted / (double)n_px + 0.999);
        if (passes < 1) passes = 1;
        if (passes > kMaxStreamPasses) passes = kMaxStreamPasses;
        per_item = (n_spp + passes - 1) / passes;
        if (per_item < 8) per_item = n_spp < 8 ? n_spp : 8;
    }
    if (per_item > n_spp) per_item = n_spp;
    if ((n_spp + per_item - 1) / per_item > kMaxStreamPasses) per_item = (n_spp + kMaxStreamPasses - 1) / kMaxStreamPasses;
    int passes = 0, done = 0;
    if (!graded) {
        while (done < n_spp) { done = done + per_item < n_spp ? done + per_item : n_spp; first[++passes] = done; }
        return passes;
    }
    const double f = ((double)n_px / (double)lanes) / 5.0;     // items per lane and pass / the weight of a heavy item
    double frac = f / (1.0 + f);
    frac = frac < 0.2 ? 0.2 : (frac > 0.5 ? 0.5 : frac);
    // ... and never BELOW a floor: a pass costs every start hit a ticket's share, a refill (record + snapshot into the lane's LDS column) and an
    // item end (three float atomics), which a single sample does not repay -- glass 1080p / 64 spp with the passes ending 4, 2, 1, 1: 7.70-7.77 ms;
    // ending 6, 6, 4: 7.60-7.61 (C5's 512 spp: no difference either way).  What the floor leaves over joins the pass before it where the item
    // cap allows; the sizes are handed out longest first.
    const int floor_size = per_item >= 16 ? 4 : (per_item >= 8 ? 2 : 1);
    int sizes[kMaxStreamPasses];
    while (done < n_spp) {
        const int left = n_spp - done;
        int size = (int)((double)left * frac + 0.999999);
        if (size > per_item) size = per_item;
        if (size < floor_size) size = floor_size;
        const int passes_left = kMaxStreamPasses - passes;     // never more than kMaxStreamPasses passes: a pass takes at least its share of what is left
        const int share = (left + passes_left - 1) / passes_left;
        if (size < share) size = share;
        if (size > left) size = left;
        if (left - size < floor_size && (left <= per_item || passes_left == 1)) size = left;      // (no pass below the floor at the very end)
        done += size; sizes[passes++] = size;
    }
    std::sort(sizes, sizes + passes, [](int x, int y) { return x > y; });
    for (int k = 0, at = 0; k < passes; ++k) { at += sizes[k]; first[k + 1] = at; }
    return passes;
}

// In which order the split kernel hands out its tickets (ItemArgs.group_first; PTMI_OPT_STREAM_PASS_GROUPS).  Pass by pass -- every region of the
// start-hit list in pass 0, then every region in pass 1 ... -- a region's 64-byte records, its snapshots' lines and the colour lines of its pixels
// come from HBM once per PASS: 1 482 MB of fetches per 1080p / 64-spp call of the glass scene (six passes), against 190 MB of records.  In GROUPS
// of consecutive passes, each group region by region, the items of a start hit that belong to one group are taken within microseconds of each
// other from one ticket queue by waves behind one L2, and only the first reads HBM (tools/traffic_terms.py, profiles/r05_traffic_terms.json:
// 1 482 -> 959 MB in pairs, 757 in threes, 546 as one group, the launch's time within +- 0.5 %).  What a group must not do is undo the GRADING:
// as ONE group the launch ends with the cheapest regions' items of EVERY pass, the long ones included -- with few regions per wave (a C5 part:
// 2.6 per pass) that is + 2 % and a quarter more spilled children.  Hence, automatically: a group is a run of passes of EQUAL size (16, 16, 16 | 8 |
// 4, 4 at 1080p / 64 spp; 74 x 5 | 50 | 32 | 21 | 14 | 9 | 6, 6 | 4 on a C5 part) -- within it every item is as long as every other, so the order
// of its tickets cannot lengthen the end of the launch.
// option 0 = automatic, 1 = every pass on its own, k in [2, 64] = the last k passes as one group, 100 + g = groups of g passes all the way (what
// does not divide goes first, pass by pass).  Returns the number of groups; table[0 .. groups] = the first pass of every group, and `passes`.
int pass_group_table(int option, const int *first, int passes, int table[kMaxStreamPasses + 1])
{
    int groups = 0;
    table[0] = 0;
    auto close = [&](int next_first) { table[++groups] = next_first; };
    if (passes < 2 || option == 1) {
        for (int p = 1; p <= passes; ++p) close(p);
    } else if (option == 0) {
        for (int p = 1; p <= passes; ++p)
            if (p == passes || first[p + 1] - first[p] != first[p] - first[p - 1]) close(p);
    } else if (option >= 100) {
        int g = option - 100 < passes ? option - 100 : passes;
        if (g < 1) g = 1;
        for (int p = 1; p <= passes % g; ++p) close(p);
        for (int p = passes % g + g; p <= passes; p += g) close(p);
    } else {
        const int g = option < passes ? option : passes;
        for (int p = 1; p <= passes - g; ++p) close(p);
        close(passes);
    }
    return groups;
}

// `render Streams` as a stream ("wavefront" form, ptmi_stream_*.hip).  Every sample of a pixel shoots the same primary ray: its
// hit is evaluated once per call into the start-hit list (regions in dispatch order), then ONE persistent launch renders all
// samples of the call:
//   * scenes whose rays never split (default batch): streams_pixels_kernel -- a lane owns a pixel for the launch, no atomics,
//     bit-identical to the per-pixel kernel under both seed rules; nothing is read back, the call is asynchronous;
//   * GLASS (or PTMI_OPT_STREAM_BATCH > 0): streams_split_kernel -- items of (start hit, sample range), children through the
//     waves' LDS rings.  The predicate `null state` (Trace.hs:166-170) is the overflow stream's length: read back ONCE, after
//     the launch; only if children really travelled through HBM does the host play `awhile`, one launch per overflow level.
// One call: its steps, and what they share.
struct StreamCall {
    ptmi_ctx *c;
    StreamFormState &f;               // c->stream_form
    RenderArgs &a;
    int n_spp;
    size_t n;                         // pixels of the part
    unsigned int n_regions, region_slots;
    size_t hit_slots;
    int cus;
    bool fresh_list = false;          // the start-hit list was built by this call
    HitList hits{};
    ItemArgs it{};
    // the split kernel
    unsigned int grid = 0, first_block = 0, level_grid_max = 0;
    size_t floor_slots = 0;           // the overflow streams hold at least every wave's static block
    int cap_rays = 0;                 // rays per pixel the overflow streams are sized for ...
    size_t capacity = 0;              // ... and the rays each of the two holds
    RayQueue q[2]{};
    std::vector<unsigned int> base{}, raw{};   // per level (mod kLvMaxLevels): where its reserved blocks start; the counters read back
    size_t plane_bytes = 0, cost_bytes = 0;
    bool can_redo = false;

    int start_hit_list(const ptmi_camera &camera);
    int ordered_passes();
    int split_setup();
    int copy_colour(bool restore);
    int read_counters(int levels);
    int overflow_levels(unsigned long long &overflowed);
    int redo_longer(bool *again);
    int fold_counters(unsigned long long overflowed);

    unsigned int *qcount() const { return f.d_qcount.as<unsigned int>(); }
    static size_t cursor_of(int level) { return (size_t)(kLvCursor + kLvPerLevel * (level % kLvMaxLevels)) * kCounterStride; }
    unsigned long long emitted_of(int level) const {         // children the level stored: the sum of its shards (read back into `raw`)
        unsigned long long total = 0;
        for (int k = 0; k < kLvEmitShards; ++k) total += raw[cursor_of(level) + (size_t)(2 + k) * kCounterStride];
        return total;
    }
    size_t slots_for(int rays_per_pixel) const { return n * (size_t)rays_per_pixel < floor_slots ? floor_slots : n * (size_t)rays_per_pixel; }
    void carve_streams() { capacity = f.queue_capacity(); q[0] = carve_queue(f.queue_block.p, capacity, 0); q[1] = carve_queue(f.queue_block.p, capacity, 1); }
};

// The start-hit list: sized, keyed, and launched unless the list of an earlier call stands.  It is a function of (camera, scene, shape,
// partition, dispatch order) only -- every sample of a pixel shoots the same primary ray, in every call.
int StreamCall::start_hit_list(const ptmi_camera &camera)
{
    if (hit_slots > f.hit_capacity || n_regions > f.hit_regions) {
        f.hit_list_valid = false;
        f.hit_capacity = 0; f.hit_regions = 0;
        // the records, and behind them one key word per slot
        if (int rc = grow(c, f.hit_block, (size_t)(kHitListWords + 1) * hit_slots * 4, "the start-hit list")) return rc;
        if (int rc = grow(c, f.d_hit_counts, (size_t)n_regions * sizeof(unsigned int), "the start-hit list's counts")) return rc;
        if (int rc = grow(c, f.d_hit_missed, (size_t)n_regions * sizeof(unsigned long long), "the start-hit list's misses")) return rc;
        f.hit_capacity = hit_slots; f.hit_regions = n_regions;
    }
    if (int rc = grow(c, f.d_qcount, (size_t)kLvWords * sizeof(unsigned int), "the stream form's counters")) return rc;
    hits.base = f.hit_block.as<uint32_t>();
    hits.slot_key = hits.base + (size_t)kHitListWords * f.hit_capacity;
    hits.counts = f.d_hit_counts.as<unsigned int>();
    hits.missed = f.d_hit_missed.as<unsigned long long>();
    hits.region_slots = region_slots;
    hits.n_regions = n_regions;
    // the statistics accumulate on the device over the whole call; cursors start from zero
    PTMI_HIP(c, hipMemsetAsync(qcount(), 0, (size_t)kLvWords * sizeof(unsigned int), c->stream));
    StreamFormState::HitKey key{};
    key.cam = camera; key.scene_version = c->scene.version; key.order_generation = a.quad_order ? c->order.generation() : 0;
    const int key_dims[8] = {a.width, a.height, a.rows_local, a.stripe_rows, a.n_parts, a.part, a.quad_order ? 1 : 0, 0};
    std::memcpy(key.dims, key_dims, sizeof key_dims);
    key.region_slots = region_slots; key.cap_allows_split = a.stream_step_cap >= 3 ? 1 : 0; key.planes_r = nullptr;
    fresh_list = !(f.hit_list_valid && std::memcmp(&key, &f.hit_key, sizeof key) == 0);
    if (fresh_list) {
        f.hit_list_valid = false;
        PTMI_HIP(c, launch_streams_primary(a, hits, qcount(), c->stream));
        f.hit_key = key; f.hit_list_valid = true;
    }
    return PTMI_OK;
}

// One lane renders a pixel's samples in order, so an item is a serial chain and the end of a launch is as long as its last
// items: with three items per lane (1080p) a quarter of the wave-time of the launch lay after the first wave had ended.
// The samples are therefore cut into ordered passes INSIDE the one launch (streams_pixels_kernel): a pixel's next pass is
// handed out once its previous one has been published.
int StreamCall::ordered_passes()
{
    const unsigned int grid_full = (unsigned int)(cus * 4 * streams_pixels_waves());
    const unsigned long long lanes = 64ull * grid_full;
    int passes = 1;
    if (c->opt_ordered_passes > 0) passes = c->opt_ordered_passes;    // (1 = off: one pass, no hand-off between waves inside the launch)
    else if (c->opt_batch > 0) passes = (n_spp + c->opt_batch - 1) / c->opt_batch;     // PTMI_OPT_STREAM_BATCH: samples per item
    else if (c->opt_pass_handoff == 0 && n < 3ull * lanes && n_spp >= 256) passes = n_spp / 64 < 8 ? n_spp / 64 : 8;
    // (automatic only with the FENCED hand-off -- release / acquire at agent scope once per region and pass, what the memory model
    // promises; the fence-free hand-off of rounds 3-5, PTMI_OPT_PASS_HANDOFF = 1, is measured valid, not promised, and never chosen
    // without the caller's explicit PTMI_OPT_ORDERED_PASSES)
    // (few, LONG items per lane: items of >= 64 samples, at most 8 passes.  The kernel of the ordered passes is 3 % slower per trip
    // than the one-pass kernel, and an item costs its refill and its seven stores.  1080p, S16, ms with 1 / 2 / 4 / 8 / 16 / 32 passes:
    // 64 spp 4.46 / 4.62 / 4.63 / 4.84 / 4.83 / 4.86; 256 spp 17.49 / 17.24 / 16.99 / 17.11 / 17.70 / 18.96; 1024 spp 69.7 / 68.1 / 66.0 /
    // 64.9 / 65.3 / 66.8.  With the per-pixel tail below, which only a one-pass launch has, the whole 1080p image -- 4.5 pixels per lane --
    // is better off in one pass: 256 spp 16.60 against 17.19 ms with four passes, 512 spp 32.86 against 33.48, 1024 spp equal; one of 8
    // parts of a 4K image -- 2.3 pixels per lane -- is not: 1024 spp 38.98 against 36.10 with eight passes.  Hence 3 pixels per lane.)
    if (passes > 64) passes = 64;
    const int most = n_spp / streams_min_pass_samples();   // a pass holds at least that many samples
    if (passes > most) passes = most;
    if (passes < 1) passes = 1;
    it.passes = passes;                                // (ordered passes wait for each other: every pass on its own, no group table)
    it.fenced = c->opt_pass_handoff == 0 ? 1 : 0;
    if (passes > 1 && n_regions >= (1u << 26)) return fail(c, PTMI_ELIMIT, "image too large for ordered passes (2^26 regions)");
    // THE TAIL.  A lane renders a pixel's whole sample chain, so the persistent launch ends as its last items do: its waves end between
    // 70 and 100 % of it.  The cheapest quads of the dispatch order -- the order kernel marks where they begin, on the device -- are
    // therefore left to the per-pixel chain kernel, launched beside the persistent kernel on a low-priority stream: its waves (one
    // tile each) take the slots the persistent waves leave as they end.  Every pixel is rendered by exactly one of the two kernels,
    // by the same arithmetic: no result depends on where the boundary lies.
    // (Only while a pixel's samples are ONE item: where they are cut into ordered passes the end of the launch is short already, and a
    // tail wave would render its tile's many samples in one piece -- 1080p / 256 spp: 16.99 ms with four passes, 17.86 with a tail beside them.)
    const unsigned int *tail = (passes == 1 && a.quad_order && quad_positions(a.width, a.rows_local) > 0) ? c->order.tail_start() : nullptr;
    if (tail && !f.tail_stream) {
        int least = 0, greatest = 0;
        PTMI_HIP(c, hipDeviceGetStreamPriorityRange(&least, &greatest));
        PTMI_HIP(c, hipStreamCreateWithPriority(&f.tail_stream, hipStreamNonBlocking, least));
        PTMI_HIP(c, hipEventCreateWithFlags(&f.ev_fork, hipEventDisableTiming));
        PTMI_HIP(c, hipEventCreateWithFlags(&f.ev_join, hipEventDisableTiming));
    }
    it.tail_start = tail;
    PTMI_HIP(c, launch_streams_advance_missed(a, hits, n_spp, tail, c->stream));
    PTMI_HIP(c, hipMemsetAsync(a.stream_iterations, 0, kItersBytes, c->stream));
    if (tail) {
        PTMI_HIP(c, hipEventRecord(f.ev_fork, c->stream));
        PTMI_HIP(c, hipStreamWaitEvent(f.tail_stream, f.ev_fork, 0));
    }

    if (passes > 1) {
        const size_t done_bytes = (size_t)n_regions * sizeof(unsigned int);
        if (int rc = grow(c, f.d_region_done, done_bytes, "the ordered passes' region counts")) return rc;
        PTMI_HIP(c, hipMemsetAsync(f.d_region_done.p, 0, done_bytes, c->stream));
        it.region_done = f.d_region_done.as<unsigned int>();
    }
    unsigned int grid = grid_full;
    const unsigned long long tickets = (unsigned long long)n_regions * (unsigned long long)passes;
    if (grid > tickets) grid = (unsigned int)(tickets < 1 ? 1 : tickets);
    PTMI_HIP(c, launch_streams_pixels(a, it, grid, c->stream));
    if (tail) {
        PTMI_HIP(c, launch_render_streams_tail(a, tail, f.tail_stream));
        PTMI_HIP(c, hipEventRecord(f.ev_join, f.tail_stream));
        PTMI_HIP(c, hipStreamWaitEvent(c->stream, f.ev_join, 0));
    }
    return PTMI_OK;
}

// ---- rays may split, or the samples of a pixel run as unordered items: everything the split kernel's launch needs but for what the
// overflow levels and a redo change -- passes, snapshots, streams, spill queues, tables, seeds, and the colour backup
int StreamCall::split_setup()
{
    if (quad_positions(a.width, a.rows_local) > (1u << 21)) a.quad_cost = nullptr;      // (the item record keeps the quad in 21 bits: no costs beyond 2^29 pixels)
    grid = (unsigned int)(cus * 4 * streams_split_waves());
    // the passes: graded items, long first and short ones last (stream_schedule above); PTMI_OPT_STREAM_BATCH caps an item's samples
    int first[kMaxStreamPasses + 1];
    int passes = stream_schedule(n_spp, n, 64ull * grid, c->opt_batch, c->opt_graded != 0, first);
    {   // the seed snapshots are passes x record slots x 16 bytes: within an eighth of the device's memory, merging the LAST passes if need be
        const size_t budget = c->opt_snapshot_mb > 0 ? (size_t)c->opt_snapshot_mb << 20 : c->device_memory / 8;
        while (passes > 1 && (size_t)passes * hit_slots * sizeof(uint4) > budget) { --passes; first[passes] = n_spp; }
        if ((size_t)passes * hit_slots * sizeof(uint4) > budget) return fail(c, PTMI_ELIMIT, "seed snapshots of the stream form would exceed their budget (PTMI_OPT_SNAPSHOT_BUDGET_MB; default: an eighth of the device's memory)");
    }
    const unsigned long long n_tickets = (unsigned long long)n_regions * (unsigned long long)passes;      // a ticket = a region of the start-hit list in one pass
    if (n_tickets > 0x7fffffffull) return fail(c, PTMI_ELIMIT, "too many items for the stream form of Streams");
    if (grid > n_tickets) grid = (unsigned int)n_tickets;
    if (int rc = grow(c, f.d_snapshots, (size_t)passes * hit_slots * sizeof(uint4), "the seed snapshots")) return rc;
    // the overflow streams: rays per pixel (PTMI_OPT_STREAM_CAPACITY, or what an earlier call grew them to) x pixels, at least every wave's static block
    first_block = streams_first_block();
    level_grid_max = (unsigned int)(cus * 4 * 6);
    floor_slots = (size_t)(grid > level_grid_max ? grid : level_grid_max) * first_block + 256;
    cap_rays = f.rays_per_pixel(c->opt_capacity);
    const size_t need = slots_for(cap_rays);
    if (need > 0xfffffff0ull) return fail(c, PTMI_ELIMIT, "image too large for the stream form of Streams");
    if (int rc = grow(c, f.queue_block, 2 * (size_t)kRayQueueWords * need * 4, "the overflow streams")) return rc;
    carve_streams();
    const size_t spill_records = (size_t)grid * streams_spill_records();
    if (int rc = grow(c, f.spill_block, (size_t)kRayQueueWords * spill_records * 4, "the spill queues")) return rc;
    base.assign((size_t)kLvMaxLevels, 0u);

    int group_table[kMaxStreamPasses + 1];
    const int groups = pass_group_table(c->opt_pass_groups, first, passes, group_table);
    {   // the pass table and the group table on the device (one block: kMaxStreamPasses + 1 entries each): rewritten only when they change
        std::vector<int> table(first, first + passes + 1);
        table.resize((size_t)kMaxStreamPasses + 1, 0);
        table.insert(table.end(), group_table, group_table + groups + 1);
        if (int rc = grow(c, f.d_pass_first, 2 * (size_t)(kMaxStreamPasses + 1) * sizeof(int), "the pass tables")) return rc;
        if (table != f.pass_first_host) {
            PTMI_HIP(c, hipStreamSynchronize(c->stream));      // (an earlier launch may still be reading the old tables)
            PTMI_HIP(c, hipMemcpy(f.d_pass_first.p, table.data(), table.size() * sizeof(int), hipMemcpyHostToDevice));
            f.pass_first_host = table;
        }
    }
    const int *pass_first = f.d_pass_first.as<int>();
    PTMI_HIP(c, launch_streams_seeds(a.planes, hits, f.d_snapshots.as<uint4>(), (long long)n, passes, pass_first, n_spp, c->stream));
    it.passes = passes; it.pass_first = pass_first;
    it.group_first = groups < passes ? pass_first + (kMaxStreamPasses + 1) : nullptr;     // (every pass on its own needs no table)
    it.groups = groups;
    // GLASS hits wait in their lanes until that many are pending in the wave (measured: DESIGN.md 5.5); nothing to wait for without GLASS
    it.glass_batch = !c->scene.has_glass ? 0 : (c->opt_glass_batch > 0 ? c->opt_glass_batch : kGlassBatchDefault);
    it.seed_snapshots = f.d_snapshots.as<const uint4>();
    it.spill = carve_queue(f.spill_block.p, f.spill_block.bytes / ((size_t)kRayQueueWords * 4), 0);
    it.out_count = qcount() + cursor_of(0);
    it.out_base = grid * first_block;
    it.emitted = it.out_count + 2 * kCounterStride;
    it.may_emit = c->scene.has_glass ? 1 : 0;

    // `expand` (Trace.hs:284-293) makes its vectors as long as the step needs; the overflow streams here have a capacity.  A call that WOULD drop
    // children is therefore redone with longer streams: the three colour planes -- all a launch changes that the next attempt reads; the seeds moved
    // before the launch, the snapshots stand -- are copied aside first (25 MB at 1080p: ~ 10 us in stream order), and when the counters say that
    // children found no room the planes are put back, the streams doubled (up to kMaxStreamRaysPerPixel rays per pixel, or to what the device
    // still has) and the launch and its levels run again.  The capacity a call reached is kept for later calls.  Only with GLASS: nothing else emits.
    plane_bytes = n * sizeof(float);
    // (only while a redo is possible: with the streams at kMaxStreamRaysPerPixel already the drops would stand, and nothing is copied aside.
    // The recorded quad costs of the launch are part of what a redo must take back: the failed attempt's items added theirs.)
    cost_bytes = a.quad_cost ? (size_t)quad_positions(a.width, a.rows_local) * sizeof(unsigned int) : 0;
    can_redo = c->scene.has_glass && cap_rays < kMaxStreamRaysPerPixel;
    if (can_redo) {
        if (int rc = grow(c, f.colour_backup, 3 * plane_bytes + cost_bytes, "the colour backup")) return rc;
        return copy_colour(false);
    }
    if (f.colour_backup.p && !c->scene.has_glass) {             // the scene lost its GLASS: the three planes' worth of memory goes back
        PTMI_HIP(c, hipStreamSynchronize(c->stream));
        release(f.colour_backup);
    }
    return PTMI_OK;
}

// the three colour planes and the launch's recorded quad costs into the colour backup, or back from it
int StreamCall::copy_colour(bool restore)
{
    void *dev[4] = {a.planes.r, a.planes.g, a.planes.b, a.quad_cost};
    for (int i = 0; i < 4; ++i) {
        const size_t bytes = i < 3 ? plane_bytes : cost_bytes;
        char *kept = f.colour_backup.as<char>() + (size_t)i * plane_bytes;
        if (bytes) PTMI_HIP(c, hipMemcpyAsync(restore ? dev[i] : kept, restore ? kept : dev[i], bytes, hipMemcpyDeviceToDevice, c->stream));
    }
    return PTMI_OK;
}

int StreamCall::read_counters(int levels)                // the statistics and the lines of the first `levels` levels
{
    int lines = kLvCursor + kLvPerLevel * levels;
    if (lines > kLvTickets) lines = kLvTickets;
    PTMI_HIP(c, hipMemcpyAsync(raw.data(), qcount(), (size_t)lines * kCounterStride * sizeof(unsigned int), hipMemcpyDeviceToHost, c->stream));
    PTMI_HIP(c, hipStreamSynchronize(c->stream));
    return PTMI_OK;
}

// `null state` (Trace.hs:166-170): the loop goes on while the last level left children in its overflow stream (a level
// cuts the rays the step cap forbids as it reads them, and counts them)
int StreamCall::overflow_levels(unsigned long long &overflowed)
{
    overflowed = 0;
    for (int level = 0; c->scene.has_glass && emitted_of(level) > 0u;) {
        overflowed += emitted_of(level);
        const size_t cursor = (size_t)raw[cursor_of(level)] + base[(size_t)(level % kLvMaxLevels)];
        const size_t items = cursor < capacity ? cursor : capacity;
        ++level;
        LevelArgs lv{};
        lv.in = q[(level + 1) & 1]; lv.out = q[level & 1];
        lv.stats = qcount();
        lv.in_count = qcount() + cursor_of(level - 1);
        lv.in_base = base[(size_t)((level - 1) % kLvMaxLevels)];
        lv.out_count = qcount() + cursor_of(level);
        lv.emitted = lv.out_count + 2 * kCounterStride;
        lv.may_emit = 1;
        const size_t chunks = (items + 63) / 64;
        const unsigned int lgrid = (unsigned int)(chunks < 1 ? 1 : (chunks > level_grid_max ? level_grid_max : chunks));
        lv.out_base = lgrid * first_block;
        base[(size_t)(level % kLvMaxLevels)] = lv.out_base;
        // the counter words of this level: long idle when they come round again
        PTMI_HIP(c, hipMemsetAsync(lv.out_count, 0, (size_t)kLvPerLevel * kCounterStride * sizeof(unsigned int), c->stream));
        PTMI_HIP(c, launch_streams_level(a, lv, lgrid, c->stream));
        if (int rc = read_counters(level + 1)) return rc;
    }
    return PTMI_OK;
}

// ---- children were dropped: longer streams, the planes put back, once more.  "Longer" must be true: the block may be larger than
// rays-per-pixel x pixels says (the floor of the waves' static blocks, a block left over from a larger image, a lowered
// PTMI_OPT_STREAM_CAPACITY), and a redo into streams of the same length drops the same children again -- so the capacity doubles until
// it asks for more than is there; if even kMaxStreamRaysPerPixel does not, the drops stand, counted.  *again: the launch runs once more.
int StreamCall::redo_longer(bool *again)
{
    *again = false;
    int grown = cap_rays;
    size_t need = 0;
    do {
        grown = grown * 2 < kMaxStreamRaysPerPixel ? grown * 2 : kMaxStreamRaysPerPixel;
        need = slots_for(grown);
    } while (need <= capacity && grown < kMaxStreamRaysPerPixel);
    if (need <= capacity) { f.grown_capacity = grown; return PTMI_OK; }
    if (need > 0xfffffff0ull) return PTMI_OK;
    DeviceBlock bigger;                                    // (first: if the device has no more, the old streams stay and the drops stand, counted)
    if (allocate(bigger, 2 * (size_t)kRayQueueWords * need * 4) != hipSuccess) return PTMI_OK;
    release(f.queue_block);                                // (the stream is idle: read_counters synchronised it)
    f.queue_block = bigger;
    cap_rays = grown; f.grown_capacity = grown;
    carve_streams();
    if (int rc = copy_colour(true)) return rc;
    // every counter of the call starts over -- but for the split pixels' count, which the primary kernel wrote and which is not run again
    const unsigned int split_pixels = raw[(size_t)kLvSplitPixels * kCounterStride];
    PTMI_HIP(c, hipMemsetAsync(qcount(), 0, (size_t)kLvWords * sizeof(unsigned int), c->stream));
    PTMI_HIP(c, hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(qcount() + (size_t)kLvSplitPixels * kCounterStride), (int)split_pixels, 1, c->stream));
    std::fill(base.begin(), base.end(), 0u);
    *again = true;
    return PTMI_OK;
}

// the counters read back after the last level, folded into the context's statistics
int StreamCall::fold_counters(unsigned long long overflowed)
{
    f.totals.rays_overflowed += overflowed;
    for (int k = 0; k < kLvLiveShards; ++k) f.totals.live_host += raw[(size_t)(kLvLive + k) * kCounterStride];
    // the two children of every glass primary hit whose split is cached in the start list: counted here, per sample
    if (fresh_list) f.hit_split_pixels = raw[(size_t)kLvSplitPixels * kCounterStride];
    f.totals.live_host += 2ull * f.hit_split_pixels * (uint64_t)n_spp;
    f.totals.rays_dropped += raw[(size_t)kLvDropped * kCounterStride];
    f.totals.rays_truncated += raw[(size_t)kLvCut * kCounterStride];
    f.totals.rays_spilled += raw[(size_t)kLvSpilled * kCounterStride];
    unsigned int longest = raw[(size_t)kLvDeepest * kCounterStride];            // stream_iterations: the deepest step of this call
    if (f.hit_split_pixels && longest < 2) longest = 2;                         // the children of the cached glass primary hits: traceStep 2
    if (longest == 0) longest = 1;                                              // every primary ray missed: one traceStep all the same
    PTMI_HIP(c, hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(a.stream_iterations), (int)longest, 1, c->stream));
    return PTMI_OK;
}

int split_passes(StreamCall &s)
{
    if (int rc = s.split_setup()) return rc;
    s.raw.assign((size_t)kLvWords, 0u);
    unsigned long long overflowed = 0;
    for (int attempt = 0;; ++attempt) {
        s.it.out = s.q[0];
        s.base[0] = s.it.out_base;
        PTMI_HIP(s.c, launch_streams_split(s.a, s.it, s.grid, s.c->stream));
        // stream_iterations lives in the per-pixel kernels' sharded counter: shard 0 carries this form's figure, copied on the device
        if (attempt == 0) PTMI_HIP(s.c, hipMemsetAsync(s.a.stream_iterations, 0, kItersBytes, s.c->stream));
        if (int rc = s.read_counters(1)) return rc;
        if (int rc = s.overflow_levels(overflowed)) return rc;
        const unsigned int dropped = s.raw[(size_t)kLvDropped * kCounterStride];
        if (!s.can_redo || dropped == 0u || s.cap_rays >= kMaxStreamRaysPerPixel) break;
        bool again = false;
        if (int rc = s.redo_longer(&again)) return rc;
        if (!again) break;
    }
    return s.fold_counters(overflowed);
}

}  // namespace

int ptmi::render_streams_wavefront(ptmi_ctx *c, RenderArgs &a, int n_spp, const ptmi_camera &camera)
{
    const size_t n = (size_t)a.rows_local * a.width;
    if (n == 0 || n_spp <= 0) return PTMI_OK;
    if (n > 0x3ffffff0ull) return fail(c, PTMI_ELIMIT, "image too large for the stream form of Streams");   // 32-bit byte offsets into the planes
    const bool ordered = !c->scene.has_glass && (c->opt_batch == 0 || a.seed_from_result);
    const unsigned int n_regions = streams_regions(a.width, a.rows_local);
    const unsigned int region_slots = ordered ? 64u : 128u;    // a glass primary hit contributes up to two start hits
    const size_t hit_slots = (size_t)n_regions * region_slots;
    if (hit_slots > 0xfffffff0ull) return fail(c, PTMI_ELIMIT, "image too large for the stream form of Streams");
    StreamCall s{c, c->stream_form, a, n_spp, n, n_regions, region_slots, hit_slots, c->cus > 0 ? c->cus : 256};
    int rc = s.start_hit_list(camera);
    if (rc == PTMI_OK) {
        ItemArgs &it = s.it;
        it.hits = s.hits;
        it.n_positions = n_regions / 4u;
        it.passes = 1; it.group_first = nullptr; it.groups = 0;
        it.n_slots = (unsigned int)hit_slots;
        it.stats = s.qcount();
        it.chunk_cursor = s.qcount() + (size_t)kLvTickets * kCounterStride;
        rc = ordered ? s.ordered_passes() : split_passes(s);
    }
    // A list built by THIS call counts as kept by later ones only if this call gets to its end: what the host keeps beside it (the split pixels'
    // count, read back by the split kernel's steps) is only then the list's.  Any error return on the way leaves the list invalid.
    if (rc != PTMI_OK && s.fresh_list) c->stream_form.hit_list_valid = false;
    return rc;
}

int StreamFormState::forget_streams(ptmi_ctx *c)
{
    grown_capacity = 0;
    if (!queue_block.p) return PTMI_OK;
    PTMI_HIP(c, hipSetDevice(c->device));                // "starts over from the value given": the streams are carved anew by the next call
    PTMI_HIP(c, hipStreamSynchronize(c->stream));
    release(queue_block);
    return PTMI_OK;
}
void StreamFormState::image_resized() { release(colour_backup); }
void StreamFormState::destroy_handles()
{
    if (ev_fork) (void)hipEventDestroy(ev_fork);
    if (ev_join) (void)hipEventDestroy(ev_join);
    if (tail_stream) { (void)hipStreamSynchronize(tail_stream); (void)hipStreamDestroy(tail_stream); }
}

extern "C" {

int ptmi_stream_schedule(int n_spp, uint64_t n_pixels, uint64_t lanes, int batch, int graded, int32_t *first, int capacity)
{
    if (n_spp < 0 || !first || capacity < 2) return PTMI_EINVAL;
    int table[kMaxStreamPasses + 1];
    const int passes = stream_schedule(n_spp, n_pixels, lanes, batch, graded != 0, table);
    if (passes + 1 > capacity) return PTMI_ELIMIT;
    for (int k = 0; k <= passes; ++k) first[k] = table[k];
    return passes;
}

int ptmi_stream_tickets(int option, const int32_t *first, int passes, int queue_regions, int32_t *pass_out, int32_t *region_out, int capacity)
{
    if (passes < 1 || passes > kMaxStreamPasses || queue_regions < 1 || !first || !pass_out || !region_out) return PTMI_EINVAL;
    if (option < 0 || option > 164 || (option > 64 && option < 102)) return PTMI_EINVAL;
    for (int p = 0; p < passes; ++p)
        if (first[p + 1] <= first[p]) return PTMI_EINVAL;
    int table[kMaxStreamPasses + 1], sizes[kMaxStreamPasses + 1];
    for (int p = 0; p <= passes; ++p) sizes[p] = first[p];
    const int groups = pass_group_table(option, sizes, passes, table);
    const long long tickets = (long long)passes * queue_regions;
    if (tickets > capacity) return PTMI_ELIMIT;
    for (long long j = 0; j < tickets; ++j) {
        unsigned int pass = 0, k = 0;
        decode_ticket((unsigned int)j, (unsigned int)queue_regions, groups < passes ? table : nullptr, groups, pass, k);
        pass_out[j] = (int32_t)pass; region_out[j] = (int32_t)k;
    }
    return (int)tickets;
}

}  // extern "C"
