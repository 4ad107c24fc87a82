// ptmi_ctx.h -- what the host units of the C ABI share: the context, its device blocks, and the owners of its state -- the scene's device
// state, the chained closure's states, what the stream form keeps between calls, the dispatch order and the statistics (internal;
// ptmi_api.cpp renders, counts and holds the options, ptmi_scene.cpp sets, moves and replaces geometry, ptmi_chain.cpp holds states under
// tokens, ptmi_stream_call.cpp is the stream form of Streams, ptmi_order.cpp the cost-ordered dispatch).
#pragma once

#include "../../include/ptmi.h"

#include <hip/hip_runtime.h>

#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <utility>
#include <vector>

#include "ptmi_kernels.h"
#include "ptmi_stage.h"

// A device block of the context: null <=> 0 bytes.  grow() and release() below keep that, and that nothing the stream may still read is freed.
struct DeviceBlock {
    void *p = nullptr;
    size_t bytes = 0;
    template <class T> T *as() const { return static_cast<T *>(p); }
};

namespace ptmi {

// ---- the layouts of the scene's blocks: each a function of its counts, used by whoever fills a block and whoever points into it ----
// The packed scene, in float4 rows: spheres | planes (two rows each) | materials of spheres, planes and -- a mesh scene -- triangles (two rows each)
struct PackedRows {
    size_t ns = 0, np = 0, nt = 0;
    size_t planes_at() const { return ns; }
    size_t materials_at() const { return ns + 2 * np; }
    size_t kept_materials_at() const { return materials_at() + 2 * ns; }            // planes', then triangles': what new spheres keep
    size_t triangle_materials_at() const { return materials_at() + 2 * (ns + np); }
    size_t rows() const { return triangle_materials_at() + 2 * nt; }
    size_t bytes() const { return rows() * sizeof(float4); }
};
// The sphere hierarchy, in float4: nodes (four each) | spheres in leaf order | their original indices
struct SphereLayout {
    size_t n_nodes = 0, ns = 0;
    size_t geom_at() const { return 4 * n_nodes; }
    size_t index_at() const { return geom_at() + ns; }
    size_t bytes() const { return (index_at() + (ns + 3) / 4) * sizeof(float4); }
};
// The triangle hierarchy, in float4: nodes | kept records in leaf order (three each) | their original indices | every record by index
struct MeshLayout {
    size_t n_nodes = 0, kept = 0, nt = 0;
    size_t geom_at() const { return 4 * n_nodes; }
    size_t index_at() const { return geom_at() + 3 * kept; }
    size_t by_index_at() const { return index_at() + (kept + 3) / 4; }
    size_t bytes() const { return (by_index_at() + 3 * nt) * sizeof(float4); }
};
// A hierarchy's plan block, in bytes: a check kernel's result words | the primitives' leaf positions (the triangles' only) | the nodes level by level
struct PlanLayout {
    size_t n_leaf_pos = 0, n_nodes = 0;
    static constexpr size_t leaf_pos_at() { return 256; }
    size_t levels_at() const { return leaf_pos_at() + ((n_leaf_pos * sizeof(int32_t) + 255) / 256) * 256; }
    size_t bytes() const { return levels_at() + n_nodes * sizeof(int32_t); }
};

// One hierarchy of the scene: `block` is rendered from; a refit writes `shadow` (a block of the same layout) and swaps the two; `plan` holds what
// the device calls need of the topology; `staging` the staged input of the host-pointer entries.
template <class Layout> struct Hierarchy {
    DeviceBlock block, shadow, plan, staging;
    Layout layout;
    PlanLayout plan_layout;
    std::vector<int32_t> level_first;                      // launches + 1 offsets into the plan's nodes, the deepest level first
    float lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0};
    void set_box(const float *l, const float *h) { std::memcpy(lo, l, sizeof lo); std::memcpy(hi, h, sizeof hi); }
    unsigned int *result() const { return plan.as<unsigned int>(); }
    int32_t *leaf_pos() const { return reinterpret_cast<int32_t *>(plan.as<char>() + PlanLayout::leaf_pos_at()); }
    int32_t *level_nodes() const { return reinterpret_cast<int32_t *>(plan.as<char>() + plan_layout.levels_at()); }
};

enum class SceneKind { Linear, Bvh, Mesh };

// The scene's device state.  Only commit() (ptmi_scene.cpp) installs into it; everybody else reads.
struct SceneState {
    SceneKind kind = SceneKind::Linear;
    DeviceBlock packed, packed_shadow;                     // PackedRows; the second block is the sphere refit's, beside spheres.shadow
    PackedRows rows;
    uint64_t share_xy = 0;                                 // a linear scene's spheres that repeat their predecessor's (cx, cy) bits (ptmi_share.h); else 0
    float sphere_reach = 0.0f;                             // a linear scene's largest |sphere centre component| or r^2, +inf when one is not finite: what the any-hit walk may assume (ptmi_query_device.h)
    Hierarchy<SphereLayout> spheres;                       // a BVH or mesh scene
    Hierarchy<MeshLayout> triangles;                       // a mesh scene
    bool glass_spheres = false, glass_planes = false, glass_triangles = false;
    bool has_glass = false;                                // any of the three (commit)
    BvhView bvh{};                                         // into spheres.block
    MeshView mesh{};                                       // into triangles.block (and a copy of bvh)
    uint64_t version = 0;                                  // bumped by every commit: the order's and the start-hit list's key
    bool hierarchical() const { return kind != SceneKind::Linear; }
    template <class F> void each_block(F &&f)
    {
        for (DeviceBlock *b : {&packed, &packed_shadow, &spheres.block, &spheres.shadow, &spheres.plan, &spheres.staging,
                               &triangles.block, &triangles.shadow, &triangles.plan, &triangles.staging})
            f(*b);
    }
};

// The chained closure (ptmi_chain.cpp): the RenderResults the caller holds tokens for.  A state's seven planes are one device block
// (carve), or -- once it had to make room -- one host block of the same layout.  Blocks of released states wait in free_blocks.
struct ChainState {
    uint64_t token = 0;
    int width = 0, height = 0;
    DeviceBlock block;                     // planes_bytes(width * height) bytes; empty: the state is on the host
    std::unique_ptr<char[]> host;          // evicted: as many bytes, carve's layout
};
struct ChainStore {
    std::vector<ChainState> states;        // in token order (oldest first)
    std::vector<DeviceBlock> free_blocks;
    uint64_t serial = 0;                   // this context's number in the process: the upper bits of its tokens
    uint64_t counter = 0;
    ptmi_chain_stats stats{};
    template <class F> void each_block(F &&f) { for (ChainState &st : states) f(st.block); for (DeviceBlock &b : free_blocks) f(b); }
};

// What the stream form of `render Streams` keeps between calls (ptmi_stream_call.cpp).  Everybody else reads `totals` and calls the functions at the end.
struct StreamFormState {
    // The tail (ordered_passes): the end of the dispatch order is rendered by the per-pixel kernel on a stream of its own, beside the persistent launch.
    hipStream_t tail_stream = nullptr;
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    // wavefront Streams (scenes with the GLASS extension): two ray streams + {next length, dropped}
    DeviceBlock queue_block;
    size_t queue_capacity() const { return queue_block.bytes / (2 * (size_t)kRayQueueWords * 4); }   // ... rays per stream
    DeviceBlock hit_block;           // the start hits of the pixels, in regions (HitList)
    // hit_capacity and hit_regions are what the list was LAID OUT for, not what the blocks hold: the block may be larger than
    // (kHitListWords + 1) * 4 * hit_capacity -- a split-kernel call of R regions at 128 slots each, then an ordered call of 1.5 R regions at
    // 64 -- and slot_key lies kHitListWords * hit_capacity words into it.
    size_t hit_capacity = 0;         // ... slots
    DeviceBlock d_hit_counts;        // ... records per region (unsigned int)
    DeviceBlock d_hit_missed;        // ... and the pixels of every region that have none (unsigned long long)
    unsigned int hit_regions = 0;
    // The start-hit list is a function of (camera, scene, shape, partition, dispatch order) only -- every sample of a pixel
    // shoots the same primary ray, in every call -- so it is kept until one of them changes.
    struct HitKey { ptmi_camera cam; uint64_t scene_version, order_generation; int dims[8]; unsigned int region_slots; int cap_allows_split; const void *planes_r; } hit_key{};
    bool hit_list_valid = false;
    uint64_t hit_split_pixels = 0;          // pixels whose glass primary hit the list replaced by its children's hits
    DeviceBlock d_snapshots;         // split kernel: the seed every item starts from
    DeviceBlock d_region_done;       // ordered passes: items published per region (unsigned int)
    DeviceBlock d_pass_first;        // split kernel: the samples of every pass (ItemArgs.pass_first), kMaxStreamPasses + 1 entries
    std::vector<int> pass_first_host;   // ... what the device block holds
    DeviceBlock d_qcount;            // kLvWords counter words (unsigned int)
    DeviceBlock spill_block;         // the waves' spill queues
    int grown_capacity = 0;          // with GLASS: rays per pixel the overflow streams have been GROWN to after a call would have dropped children (0: never)
    DeviceBlock colour_backup;       // ... the three colour planes as they were before the call's launch (the call is redone if children were dropped)
    struct Totals {
        uint64_t rays_dropped = 0;
        uint64_t rays_truncated = 0;
        uint64_t rays_spilled = 0;       // children that found the wave's ring full and went through HBM
        uint64_t rays_overflowed = 0;    // ... and its spill queue too: traced by an overflow level
        uint64_t live_host = 0;          // live rays counted on the host
    } totals;
    template <class F> void each_block(F &&f) { for (DeviceBlock *b : {&queue_block, &hit_block, &d_hit_counts, &d_hit_missed, &d_snapshots, &d_region_done, &d_pass_first, &d_qcount, &spill_block, &colour_backup}) f(*b); }
    int rays_per_pixel(int opt_capacity) const { return grown_capacity > opt_capacity ? grown_capacity : opt_capacity; }   // the capacity in force
    int forget_streams(ptmi_ctx *c);                 // PTMI_OPT_STREAM_CAPACITY was set: the streams are carved anew, from the value given, by the next call
    void image_resized();                            // the colour backup was sized by the old image (the caller has drained the stream)
    void reset_totals() { totals = Totals{}; }
    void destroy_handles();                          // the tail's events, then its stream (synchronised first)
};

struct RenderTarget;

// The cost-ordered dispatch of the tiled kernels (ptmi_order.cpp; ptmi_device.h: lane_pixel): what every quad of tiles cost in the launches
// made with one key -- (camera, scene, shape, limit, algorithm) -- and the order, most expensive first, later launches with that key use.
// launch_render says which calls are ordered and brackets their launches with the first two functions; the stream form reads the next two.
// Behind them: a rebuild of the order, or any change of its use, bumps the generation; another key, or blocks too small, start the count of
// launches over; the count moves only once the launches went out; the tail's start word holds the number of quads -- no tail -- until the first rebuild.
struct DispatchOrder {
    // the blocks hold the target's quads, the costs are cleared or the order rebuilt, a.quad_order / a.quad_cost are set; a code as grow's
    int before_launches(ptmi_ctx *c, const ptmi_camera &camera, uint64_t scene_version, const RenderTarget &target, int bounce_limit, int algorithm,
                        bool stream_form, RenderArgs &a);
    void launches_went_out() { launches = launches_after; }     // ... and after them: a call that failed in between repeats its step of the schedule
    uint64_t generation() const { return generation_; }         // what a start-hit list made in this order is keyed by (StreamFormState::HitKey)
    const unsigned int *tail_start() const { return tail_permille ? d_tail_start.as<unsigned int>() : nullptr; }   // the device word where the stream form's tail begins in the order; null: there is no tail
    int &tail_option() { return tail_permille; }                // PTMI_OPT_STREAM_TAIL
    template <class F> void each_block(F &&f) { for (DeviceBlock *b : {&d_quad_cost, &d_quad_order, &d_quad_class, &d_tail_start}) f(*b); }
private:
    DeviceBlock d_quad_cost, d_quad_order, d_quad_class, d_tail_start;   // unsigned int per quad; one word, written by the order kernel
    struct Key { ptmi_camera cam; uint64_t scene_version; int dims[8]; } key{};
    int launches = 0, launches_after = 0;                  // launches made with this key; ... once this call's went out
    uint64_t generation_ = 0;
    int tail_permille = -1;                                // thousandths of the recorded cost the tail may hold (0 = no tail; -1 = automatic)
};

// The statistics of the render launches (ptmi_api.cpp): the kernels' counter blocks, what the host counts beside them, and the timing events.
struct RenderStats {
    enum { Live, Work, Iters, StreamCounters };            // RenderArgs.live_counter, work_counter, stream_iterations, stream_counters
    DeviceBlock block[4];
    static constexpr size_t kBytes[4] = {(size_t)kStatShards * kStatStride * sizeof(unsigned long long), kWorkWords * sizeof(unsigned int),       // (the first and the
                                         (size_t)kStatShards * 2 * kStatStride * sizeof(unsigned int), kScWords * sizeof(unsigned long long)};   // third are sharded, ptmi_kernels.h)
    uint64_t nominal = 0, samples = 0;
    bool timing = false, ev_valid = false;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    hipError_t create(hipStream_t stream, const char **failed_call);      // the events, the blocks, then stream-ordered zero fills
    int reset(ptmi_ctx *c);
    int read(ptmi_ctx *c, ptmi_stats *out);                               // the shard sums and maximum, the stream form's totals, the elapsed time
    int launches_begin(ptmi_ctx *c, RenderArgs &a);                       // a call's launches: their counters, the two events around them ...
    int launches_end(ptmi_ctx *c, uint64_t samples_made, uint64_t bounces_nominal);       // ... and what the call adds to the host's counts
    template <class F> void each_block(F &&f) { for (DeviceBlock &b : block) f(b); }
};
constexpr size_t kItersBytes = RenderStats::kBytes[RenderStats::Iters];      // (the stream form clears RenderArgs.stream_iterations itself)

}  // namespace ptmi

struct ptmi_ctx {
    std::mutex mu;
    int device = 0;
    std::string err;

    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;

    int width = 0, height = 0;
    int stripe_rows = 0, n_parts = 1, part = 0;   // stripe_rows == 0: one part holds everything
    int rows_local = 0;

    ptmi::Planes owned{};          // seven planes carved from owned_block
    DeviceBlock owned_block;
    ptmi::Planes bound{};
    bool use_bound = false;

    ptmi::SceneState scene;  // what is rendered (ptmi_scene.cpp)
    int opt_bvh_build = PTMI_BVH_BUILD_EQUAL_COUNT;   // PTMI_OPT_BVH_DEVICE_BUILD: which tree ptmi_set_bvh_spheres builds

    ptmi::RenderStats stats;       // what the render launches count (ptmi_api.cpp)
    hipEvent_t ev_snap = nullptr;  // ptmi_snapshot_color: orders a copy on another stream behind the renders
    int variant = ptmi::kVariantAuto;
    ptmi::Stager stager;                          // pinned ring + worker threads for host-buffer entry points (ptmi_stage.h)

    ptmi::DispatchOrder order;     // the cost-ordered dispatch of the tiled kernels (ptmi_order.cpp)
    DeviceBlock d_chunk_done;                  // sample chunks of the tiled Inline kernel: one word per tile workgroup, then the ticket counter's line
    unsigned int chunk_capacity() const { return d_chunk_done.bytes ? (unsigned int)(d_chunk_done.bytes / sizeof(unsigned int)) - 32u : 0u; }   // ... that many

    // scratch for ptmi_render1 / point queries
    DeviceBlock scratch;

    int cus = 0;                     // compute units of the device (persistent grids)
    size_t device_memory = (size_t)64 << 30;   // bytes of the device (budget of the stream form's seed snapshots)
    DeviceBlock tree_stack;          // tree walk: the lanes' first waiting children (RenderArgs.tree_stack)
    ptmi::StreamFormState stream_form;   // the stream form's host side (ptmi_stream_call.cpp)

    // options of render Streams (ptmi_set_option: one row of its table each; PTMI_OPT_STREAM_TAIL is the order's)
    int opt_seed_rule = PTMI_SEED_AUTO;              // resolved per scene: effective_seed_rule()
    int opt_step_cap = ptmi::kStreamStepCapDefault;
    int opt_capacity = 4;
    int opt_form = PTMI_FORM_AUTO;
    int opt_batch = 0;
    int opt_spp_chunks = 0;                    // 0 = automatic
    int opt_arithmetic = PTMI_ARITH_EXACT;
    int opt_ordered_passes = 0;      // PTMI_OPT_ORDERED_PASSES: 0 = automatic, 1 = off, k = k passes
    int opt_pass_handoff = 0;        // PTMI_OPT_PASS_HANDOFF: 0 = release / acquire once per (region, pass); 1 = the fence-free write-through hand-off
    int opt_glass_batch = 0;                   // PTMI_OPT_GLASS_BATCH: 0 = automatic, 1 = off, k = GLASS hits wait until k are pending in their wave
    int opt_graded = 1;                        // PTMI_OPT_STREAM_GRADED: the split kernel's passes shrink towards the end of the launch
    int opt_snapshot_mb = 0;                   // PTMI_OPT_SNAPSHOT_BUDGET_MB: 0 = an eighth of the device's memory
    int opt_pass_groups = 0;                  // PTMI_OPT_STREAM_PASS_GROUPS: 0 = automatic, 1 = off, k = the last k passes are handed out region by region
    int opt_chain_slots = 0;                   // PTMI_OPT_CHAIN_SLOTS: 0 = automatic

    ptmi::ChainStore chain;          // the chained closure's states (ptmi_chain.cpp)

    // Every DeviceBlock above: ptmi_destroy releases them all.  A new block is one more name here, or in its owner's each_block.
    template <class F> void each_block(F &&f)
    {
        for (DeviceBlock *b : {&owned_block, &d_chunk_done, &scratch, &tree_stack}) f(*b);
        stats.each_block(f);
        order.each_block(f);
        scene.each_block(f);
        stream_form.each_block(f);
        chain.each_block(f);
    }
};

namespace ptmi {

// The message of a failed call, and its code (the context's mutex is held by every caller with a context).
int fail(ptmi_ctx *c, int code, const std::string &msg);

// A runtime error leaves through this library's return code -- and not, a second time, through the runtime's sticky slot (hipGetLastError
// keeps the last failure of the thread until somebody asks: the caller's next launch check, or another library's, would find it there).
int fail_hip(ptmi_ctx *c, hipError_t e, const char *call);
#define PTMI_HIP(c, call)                                                                  \
    do {                                                                                   \
        hipError_t e_ = (call);                                                            \
        if (e_ != hipSuccess) return ptmi::fail_hip((c), e_, #call);                       \
    } while (0)

// The one allocation of a DeviceBlock (which must be empty).  On failure it stays empty and the runtime's sticky slot is cleared.
hipError_t allocate(DeviceBlock &b, size_t bytes);
void release(DeviceBlock &b);
// `b` holds at least `bytes` (its contents are not kept).  A block that is replaced goes only once the stream is drained; with none
// held nothing on the stream can read it (the tail stream has joined c->stream before any call returns).  If the allocation fails the
// block is empty.
int grow(ptmi_ctx *c, DeviceBlock &b, size_t bytes, const char *what);

// Host-buffer transfers of the boundary (stream-ordered on c->stream).  Transfers of a megabyte or more go through
// the context's Stager (ptmi_stage.h: parallel page copies into a pinned ring, one DMA per 8-MB chunk -- the driver
// never pins the caller's pages); small ones, or all of them when the engine is off (PTMI_STAGE_THREADS=0), are
// plain async copies.  copy_to_host leaves the stream drained in both cases.
hipError_t copy_to_device(ptmi_ctx *c, const CopySpan *spans, int n);
hipError_t copy_to_host(ptmi_ctx *c, const CopySpan *spans, int n);

// ---- the render path (ptmi_api.cpp), as far as the chain and the stream form use it: seven planes of n pixels in one block, and its size
Planes carve(void *block, size_t n);
size_t planes_bytes(size_t n);
bool too_many_pixels(int width, int height);
// The planes of n pixels against seven host pointers, as copy spans; a null pointer's plane is skipped (what that means is the caller's to say).  Returns their number.
int plane_spans(const Planes &p, const void *const host[7], size_t n, CopySpan spans[7]);
struct RenderTarget {                                      // what a launch renders into: planes, and which rows of which image they are
    Planes planes;
    int width, height, rows_local, stripe_rows, n_parts, part;
    const int64_t *sx, *sy;                                // an explicit screen (ptmi_render1), or null
    static RenderTarget whole(const Planes &p, int w, int h, const int64_t *sx = nullptr, const int64_t *sy = nullptr) { return {p, w, h, h, h, 1, 0, sx, sy}; }
};
int check_render_args(ptmi_ctx *c, const ptmi_camera *camera, int algorithm, int bounce_limit, int n_spp);
int effective_seed_rule(const ptmi_ctx *c);               // PTMI_OPT_STREAMS_SEED_RULE resolved for the context's scene
// What the launcher of a caller-ray kernel takes of the context's scene (the ray queries, the paths, the stepped paths, the ray streams):
// the packed rows, and the hierarchy of a BVH scene or of a mesh scene -- null otherwise
struct RayCallScene { SceneView scene; const BvhView *bvh; const MeshView *mesh; };
SceneView scene_view(const SceneState &s);
RayCallScene ray_call_scene(const ptmi_ctx *c);
int launch_render(ptmi_ctx *c, const RenderTarget &target, const ptmi_camera *camera, int algorithm, int bounce_limit, int n_spp);
// `render Streams` in its stream form (ptmi_stream_call.cpp): launch_render's branch for it
int render_streams_wavefront(ptmi_ctx *c, RenderArgs &a, int n_spp, const ptmi_camera &camera);

}  // namespace ptmi
