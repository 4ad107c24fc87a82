// ptmi_kernels.h -- launch interface between the C ABI (ptmi_api.cpp, ptmi_stream_call.cpp, ptmi_chain.cpp, ptmi_scene.cpp) and the gfx950 kernels (ptmi_*.hip, one unit per kernel family).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <tuple>
#include <type_traits>
#include <utility>

#include "ptmi_core.h"

struct ptmi_ctx;

namespace ptmi {

// (between the C ABI's two units: the image size a context stands at, 0 x 0 while it is unsized -- ptmi_group.cpp checks its members with it)
void context_size(const ptmi_ctx *ctx, int *width, int *height);

// Scene as staged into LDS, one float4 stream (see pack_scene in ptmi_scene.cpp):
//   [0, ns)                 sphere geometry   (cx, cy, cz, r*r)
//   [ns, ns + 2 np)         plane geometry    (px, py, pz, 0) (nx, ny, nz, 0)
//   [geom, geom + 2 (ns+np)) material         (cr, cg, cb, illuminance) (tag bits, p, p/pi, (1-p)/2)
struct SceneView {
    const float4 *packed;      // device memory
    int n_spheres, n_planes;
    unsigned long long share_xy;   // bit i: sphere i has sphere i - 1's cx and cy bits (a linear scene's, ptmi_share.h; 0 otherwise)
    __host__ __device__ int geom_f4() const { return n_spheres + 2 * n_planes; }
    __host__ __device__ int total_f4() const { return geom_f4() + 2 * (n_spheres + n_planes); }
};

// The sphere hierarchy of a BVH scene (ptmi_set_scene_bvh; ptmi_bvh_device.h walks it).  The packed scene above stays as it is (the
// materials, the planes, hit_record by original index); the spheres are tested through `geom`.
struct BvhView {
    const float4 *nodes;      // ptmi_bvh_node, four float4 each: (c0 xyz, c1 x) (c1 yz, h0 xy) (h0 z, h1 xyz) (ref0, ref1, inv_2r0, inv_2r1)
    const float4 *geom;       // the spheres in leaf order: (cx, cy, cz, r*r), as pack_scene makes them
    const int *index;         // ... and their original indices
    float lo[3], hi[3];       // box of the sphere centres
};

// A mesh scene (ptmi_set_scene_mesh; ptmi_mesh_device.h walks it): a BVH scene's spheres and planes, and the triangles in a second
// hierarchy.  The packed scene holds the materials of spheres, planes AND triangles (triangle k is primitive ns + np + k).
struct MeshView {
    BvhView spheres;          // the sphere hierarchy, as for a BVH scene
    const float4 *nodes;      // the triangle hierarchy, ptmi_bvh_node as above (inv_2r unused)
    const float4 *geom;       // the triangles in leaf order, three float4 each: (v0, nx) (v1, ny) (v2, nz), n the unit normal
    const int *index;         // ... and their original indices
    const float4 *by_index;   // the same records by original index (zero area: a NaN normal, never hit)
    int n_triangles, n_kept;  // all of them / those in the hierarchy (non-zero area)
    float lo[3], hi[3];       // box of the kept triangles' vertices
};

struct Planes {
    float *r, *g, *b;
    uint32_t *sa, *sb, *sc, *sctr;
};

struct RenderArgs {
    PrimaryUniforms cam;
    SceneView scene;
    Planes planes;
    const int64_t *screen_x, *screen_y;   // optional explicit Matrix (V2 Int); NULL = implicit
    int width, height;                    // whole image (screenWidth/Height)
    int rows_local;                       // rows held by this context
    int stripe_rows, n_parts, part;       // row-stripe partition
    int bounce_limit, n_spp;
    // device statistics, SHARDED: kStatShards words kStatStride words apart, a wave adds to shard (workgroup & (kStatShards - 1)).
    // One word serves ~90 atomics per microsecond: 7 500 waves of a 1-spp launch ending together took 83 us to count themselves.
    unsigned long long *live_counter;     // += live bounces (the host sums the shards)
    unsigned int *work_counter;           // device counter for dynamic pixel hand-out (variants)
    unsigned int *stream_iterations;      // Streams: steps taken by the last sample (max over waves)
    // Cost-ordered dispatch of the tiled kernels (see lane_pixel in ptmi_device.h).  A "quad" is a run of four
    // x-adjacent 8x8 tiles.  quad_order: the quad each dispatch position works on (NULL = image order).
    // quad_cost: where each wave adds the loop trips it paid (NULL = do not record).
    const unsigned int *quad_order;
    unsigned int *quad_cost;
    // Sample chunks of the tiled render Inline kernel (see render_inline_kernel): spp_chunks = 0 lets the launcher choose,
    // 1 switches them off, k >= 2 forces k copies; chunk_done: one word per tile workgroup (capacity words) and, behind them,
    // the ticket counter of the launch (chunk_done[chunk_capacity]), device memory.
    int cus;                              // compute units of the context's device
    int spp_chunks;
    unsigned int *chunk_done;
    unsigned int chunk_capacity;
    // render Streams only
    int stream_step_cap;                  // traceSteps per ray lineage before the safety cap cuts it (the reference has none)
    int seed_from_result;                 // PTMI_SEED_FROM_RESULT: a hit's ray seed replaces the pixel's (assumption A5)
    unsigned long long *stream_counters;  // device: [kScTruncated] rays cut by the cap, [kScDropped] children that found no room
    // tree walk: the first kTreeFastLevels waiting children of every lane, [tile workgroup][level][lane] records of four float4
    // (tree_stack_tiles workgroups); required by render_streams_tree_kernel
    float4 *tree_stack;
    // render_streams_kernel as the TAIL of the stream form (streams_pixels_kernel's launch): the workgroups start at dispatch position
    // *first_position (a device word: where the stream form's part of the dispatch order ends) and those past the grid do nothing;
    // costs are recorded in the stream form's unit (shaded hits per quad).  NULL = the whole grid, as ever.
    const unsigned int *first_position;
};
enum { kScTruncated = 0, kScDropped = 1, kScWords = 4 };
constexpr int kWorkWords = 256;            // RenderArgs.work_counter: the hand-out counter in [0], the diagnostic builds' counters behind it (ptmi_diag.h; ptmi_debug_counters)
constexpr int kTreeStackDepth = 16;        // per-pixel tree walk: pending children a lane can hold (render_streams_tree_kernel)
#ifndef PTMI_TREE_FAST_LEVELS
#define PTMI_TREE_FAST_LEVELS 4
#endif
constexpr int kTreeFastLevels = PTMI_TREE_FAST_LEVELS;   // ... of which the first few are 64-byte records in global memory (RenderArgs.tree_stack), the rest scratch

// Ray stream of the stream form of Streams: `capacity` records (type RayState, Trace.hs:46) of 16 words = one 64-byte line:
//   [origin xyz, direction x] [direction yz, throughput xy] [throughput z, local pixel index, seed a, seed b]
//   [seed c, seed counter, step index (traceSteps taken by the ray's ancestors = the awhile iteration it belongs to), -]
// A record is written and read as four 16-byte accesses with one address computation (as fifteen word planes every emitted
// child cost fifteen stores with an address each).  One base pointer + the capacity: kernel arguments live in scalar registers.
constexpr int kStatShards = 256, kStatStride = 16;    // 128 B apart (u64) -- u32 shards use the same byte distance (stride 32)

struct RayQueue {
    uint32_t *base;
    unsigned int capacity;  // records
    PTMI_HD float4 *record(unsigned int i) const { return reinterpret_cast<float4 *>(base) + (size_t)i * 4; }
    PTMI_HD uint32_t *pixel_word(unsigned int i) const { return base + (size_t)i * 16 + 9; }     // kHole marks an unused slot
};
constexpr int kRayQueueWords = 16;
constexpr int kCounterStride = 32;          // device counters sit 128 B apart (one per cache line)
constexpr int kStreamStepCapDefault = 1 << 16;   // traceSteps per ray lineage; the reference has no bound (Trace.hs:166-170) -- this only guarantees termination
// Counters of the stream form, each kCounterStride words (one cache line) apart; sums are sharded by workgroup, because one
// word serves only ~90 atomics per microsecond and the 6 144 waves of a level end together:
//   [kLvLive, +kLvLiveShards) children emitted | kLvCut rays cut by the step cap | kLvDropped children that found the output
//   stream full | kLvDeepest deepest step + 1 | kLvSpilled children that went through HBM (spill queues, overflow stream) | kLvSplitPixels pixels whose (glass) primary hit
//   was replaced by its children's hits | per level l, kLvPerLevel lines from kLvCursor + kLvPerLevel l:
//     + 0: the reservation cursor of the stream level l WRITES, counted from the end of its waves' static blocks (grid * first
//          block: LevelArgs.out_base / in_base; that sum = the item count, holes included, of the stream level l + 1 reads)
//     + 1: level l's chunk hand-out | + 2 .. + 2 + kLvEmitShards: the children level l stored (shards)
constexpr int kLvLiveShards = 64, kLvEmitShards = 8, kLvPerLevel = 2 + kLvEmitShards;
constexpr int kLvLive = 0, kLvCut = kLvLiveShards, kLvDropped = kLvCut + 1, kLvDeepest = kLvCut + 2, kLvSpilled = kLvCut + 3, kLvSplitPixels = kLvCut + 4,
              kLvCursor = kLvCut + 5, kLvMaxLevels = 64;
// ... and, behind the per-level lines, the ticket counters of the item kernels: eight (one per XCD queue) per launch of a call
constexpr int kLvTickets = kLvCursor + kLvPerLevel * kLvMaxLevels, kLvMaxLaunches = 32;
constexpr int kLvWords = (kLvTickets + 8 * kLvMaxLaunches) * kCounterStride;
// The hits the samples of the held pixels START from, written once per render call (streams_primary_kernel), in REGIONS: one
// region per 64-pixel tile of the image (a wave of the primary kernel: an 8x8 pixel tile, or 64 consecutive pixels of a row
// for images too small for tiles), in the order the tiles are dispatched (most expensive quad of tiles first once costs
// are known) -- no atomics, the order is deterministic.  A region holds its tile's records compacted to the front (ballot +
// popcount prefix in the wave) and `counts[region]` says how many: usually one per pixel whose primary ray hits, none for
// a pixel whose ray misses.  For a GLASS primary hit -- whose two children are the same two rays in every sample, a glass
// hit draws nothing that changes a direction -- the first hit of each child instead (0, 1 or 2 records), with the
// throughput, the step index and the number of raw draws its ray's seed is ahead of the sample's: regions then have 128 slots.
struct HitList {             // records of 16 words: [position xyz, normal x] [normal yz, direction xy] [direction z, throughput xyz] [primitive, local pixel index, meta, quad]
    uint32_t *base;
    uint32_t *slot_key;      // per record slot: the record's pixel (30 bits) | the code of its raw draws (0, 3, 4 -> 0, 1, 2) << 30 -- all that
                             // streams_slot_seeds_kernel needs of a record: 4 bytes per slot and call instead of the record's 64-byte line
    unsigned int *counts;    // records per region
    unsigned long long *missed;   // per region: the lanes (pixels of the tile) that have no start hit
    unsigned int region_slots;   // 64, or 128 when a primary hit can split
    unsigned int n_regions;
    PTMI_HD float4 *record(unsigned int i) const { return reinterpret_cast<float4 *>(base) + (size_t)i * 4; }
};
constexpr int kHitListWords = 16;
// Overflow levels of the stream form (streams_level_kernel): children that found the wave's ring full travel through HBM.
struct LevelArgs {
    RayQueue in, out;
    const unsigned int *in_count;   // device: the producer's reservation cursor
    unsigned int in_base;           // ... which counts from here (the producer's out_base)
    unsigned int *out_count;        // device: this level's reservation cursor, zero at launch
    unsigned int out_base;          // grid * (first block size): where reserved blocks start
    unsigned int *emitted;          // device: children this level stored in `out`: kLvEmitShards words, kCounterStride apart
    unsigned int *stats;            // device: base of the counter block
    int may_emit;                   // 0: the scene has no ray-splitting material -- nothing is ever written to `out`
};
// The item kernels of the stream form (streams_pixels_kernel, streams_split_kernel): persistent waves take the regions of the
// start-hit list as chunks, by ticket, from eight queues (one per XCD; ChunkCursor in ptmi_stream_form.h).
struct ItemArgs {
    HitList hits;
    unsigned int n_positions;       // groups of four regions (dispatch positions): hits.n_regions / 4
    const unsigned int *tail_start; // streams_pixels_kernel: a device word -- the positions from there on are left to the per-pixel kernel (NULL: none)
    int passes;                     // tickets run over the chunks this many times: a pixel's samples in that many items
    const int *group_first;         // device, groups + 1 entries (NULL: every pass on its own): the passes are handed out in GROUPS of consecutive passes
    int groups;                     // [group_first[g], group_first[g + 1]), a group region by region -- region r in every pass of the group, then region r + 1: a
                                    // region's items of one group follow each other through one ticket queue, and all but the first find its records and
                                    // colour lines in that XCD's L2 (decode_ticket).  A group of one pass is that pass, pass by pass as ever
    unsigned int *region_done;      // streams_pixels_kernel, passes > 1: per region, the items published so far (zero at launch)
    int fenced;                     // ... 1: release / acquire at agent scope, once per (region, pass); 0: the fence-free write-through hand-off (PTMI_OPT_PASS_HANDOFF)
    unsigned int *chunk_cursor;     // device: the launch's eight ticket counters, kCounterStride words apart, zero at launch
    // streams_split_kernel only
    const int *pass_first;          // device, passes + 1 entries: pass p renders samples [pass_first[p], pass_first[p + 1]) of its pixels -- long items first, short ones
                                    // at the end of the launch, which is as long as its last items (stream_schedule in ptmi_stream_call.cpp)
    const uint4 *seed_snapshots;    // [passes][n_slots]: the seed the item (record slot, pass) starts from (streams_slot_seeds_kernel)
    int glass_batch;                // > 1: GLASS hits wait in their lanes until that many are pending in the wave (PTMI_OPT_GLASS_BATCH)
    unsigned int n_slots;           // slots of the start-hit list: hits.n_regions * hits.region_slots
    RayQueue spill;                 // the waves' own spill queues: streams_spill_records() records each, gridDim of them
    RayQueue out;                   // overflow stream: children that found ring and spill queue full
    unsigned int *out_count;        // device: reservation cursor of `out`, zero at launch
    unsigned int out_base;
    unsigned int *emitted;
    unsigned int *stats;
    int may_emit;
};

// Ticket j of a queue of n regions -> (pass, the region's index k in the queue), j < n * passes.  Without a group table: pass by pass.  With one:
// group g owns tickets [n group_first[g], n group_first[g + 1]) and hands them out region by region.  Host and device: the kernels' next_chunk and
// ptmi_stream_tickets (the order as a pure function, tested without a GPU).  (The scan is wave-uniform scalar work, once per ticket -- an item is
// hundreds to thousands of loop trips; a graded schedule has a handful of groups.)
PTMI_HD void decode_ticket(unsigned int j, unsigned int n, const int *group_first, int groups, unsigned int &pass, unsigned int &k)
{
    if (!group_first) {
        pass = j / n;
        k = j - pass * n;
        return;
    }
    int g = 0;
    while (g + 1 < groups && j >= n * (unsigned int)group_first[g + 1]) ++g;
    const unsigned int first = (unsigned int)group_first[g], size = (unsigned int)group_first[g + 1] - first, rem = j - n * first;
    k = rem / size;
    pass = first + (rem - k * size);
}

hipError_t launch_streams_pixels(const RenderArgs &a, const ItemArgs &it, unsigned int grid, hipStream_t stream);
hipError_t launch_streams_split(const RenderArgs &a, const ItemArgs &it, unsigned int grid, hipStream_t stream);
int streams_pixels_waves();           // waves per SIMD the item kernels are built for (persistent grids)
int streams_split_waves();
int streams_min_pass_samples();       // ordered passes: a pass must hold at least this many samples
unsigned int streams_spill_records();   // records of a wave's spill queue in HBM
unsigned int streams_regions(int width, int rows_local);    // regions of the start-hit list
hipError_t launch_streams_seeds(Planes p, HitList hits, uint4 *snapshots, long long n, int passes, const int *pass_first, int draws, hipStream_t stream);   // pass_first: device, passes + 1 entries
hipError_t launch_streams_level(const RenderArgs &a, const LevelArgs &lv, unsigned int grid, hipStream_t stream);
hipError_t launch_streams_primary(const RenderArgs &a, HitList hits, unsigned int *counters, hipStream_t stream);
// updateSeeds for the pixels without start hits (the ordered item kernel advances the others itself)
hipError_t launch_streams_advance_missed(const RenderArgs &a, HitList hits, int draws, const unsigned int *tail_start, hipStream_t stream);
hipError_t launch_render_streams_tail(const RenderArgs &a, const unsigned int *first_position, hipStream_t stream);
unsigned int streams_first_block();   // output slots every wave of a level owns from the start

// The kernel variants (ptmi_set_variant takes them as an int).  Inline's kernel for each; the ablations exist only in builds with
// -DPTMI_ABLATIONS (ptmi_set_variant refuses them otherwise).  A scene too big for LDS takes the scalar-load form of an
// LDS variant (1 -> 6, 4 / 7 / 8 -> 5, 13-16 -> 17).  Streams and the tree walk read 4 / 5 as rows of 64 and 5 / 17 (Streams: 6 too) as
// scalar loads; 9 is the stream form of Streams (the contracted object renders Inline's automatic choice for it).
enum Variant : int {
    kVariantAuto = 0,               // rows or 8x8 tiles, LDS or scalar loads, as the image and the scene make pay
    kVariantPersistent = 1,         // ablation: persistent hand-out, LDS scene
    kVariantLockstep = 2,           // ablation: lock step
    kVariantRegenerate = 3,         // ablation: regenerate only
    kVariantRows = 4,               // cached, a wave = 64 consecutive pixels of a row, LDS scene
    kVariantRowsScalar = 5,         // 4 with the scene through scalar loads
    kVariantPersistentScalar = 6,   // ablation: 1 with the scene through scalar loads
    kVariantCapped4 = 7,            // ablation: 4 capped at 4 waves per SIMD through dynamic LDS
    kVariantCapped3 = 8,            // ablation: ... at 3 waves
    kVariantStreamForm = 9,         // Streams in its stream form
    kVariantPooled2 = 10,           // ablation: pooled second shade round, 2 / 4 / 8 waves per workgroup
    kVariantPooled4 = 11,
    kVariantPooled8 = 12,
    kVariantTiles = 13,             // 4 with 8x8 pixel tiles per wave
    kVariantTiles16x4 = 14,         // ablation: other pixel tiles per wave
    kVariantTiles4x16 = 15,
    kVariantTiles32x2 = 16,
    kVariantTilesScalar = 17,       // 5 with 8x8 tiles
    kVariantRound1 = 18,            // ablation: round 1's loop (no frozen-shade shortcut), 8x8 tiles, LDS scene
    kVariantCount
};
bool variant_available(int variant);
// The per-pixel kernels of each family; bvh: a BVH scene (ptmi_set_scene_bvh, variant 0 only), null for a linear one
hipError_t launch_render_inline(const RenderArgs &a, const BvhView *bvh, int variant, hipStream_t stream);
hipError_t launch_render_inline_ablation(const RenderArgs &a, int variant, bool big_scene, hipStream_t stream);   // ptmi_inline_ablations.hip (-DPTMI_ABLATIONS)
hipError_t launch_render_streams(const RenderArgs &a, const BvhView *bvh, int variant, hipStream_t stream);
hipError_t launch_render_streams_tree(const RenderArgs &a, const BvhView *bvh, int variant, hipStream_t stream);   // scenes with GLASS: per-pixel tree walk
hipError_t launch_eval_check_hit(SceneView scene, const BvhView *bvh, const float *rays, int n, float *t, int32_t *idx, int32_t *just, hipStream_t stream);
// ... their mesh-scene instantiations (ptmi_set_scene_mesh: variant 0, per-pixel forms only)
hipError_t launch_render_inline_mesh(const RenderArgs &a, const MeshView &mesh, hipStream_t stream);
hipError_t launch_render_streams_mesh(const RenderArgs &a, const MeshView &mesh, hipStream_t stream);
hipError_t launch_render_streams_tree_mesh(const RenderArgs &a, const MeshView &mesh, hipStream_t stream);
hipError_t launch_eval_check_hit_mesh(SceneView scene, const MeshView &mesh, const float *rays, int n, float *t, int32_t *idx, int32_t *just, hipStream_t stream);
// The ray queries on device-resident arrays (ptmi_trace_rays_device, ptmi_occluded_device; ptmi_query.hip): one lane per ray against a linear
// scene (bvh and mesh null; its shared-xy walk when scene.share_xy is not 0), a BVH scene (bvh) or a mesh scene (mesh).  hit: n x 6 words or
// null.  reach: a linear scene's largest |sphere centre component| or r^2, +inf when one is not finite (SceneState.sphere_reach).  Every
// array needs 4-byte alignment; 8-byte aligned rays and hit records are moved two words at a time.
hipError_t launch_trace_rays(SceneView scene, const BvhView *bvh, const MeshView *mesh, const float *rays, int n, float *t, int32_t *idx, float *hit,
                             hipStream_t stream);
hipError_t launch_occluded(SceneView scene, const BvhView *bvh, const MeshView *mesh, float reach, const float *rays, const float *t_max, int n,
                           int32_t *occluded, hipStream_t stream);
// ... and through an index (ptmi_trace_rays_indexed_device, ptmi_occluded_indexed_device; ptmi_query_indexed.hip): entry k < m names ray
// index[k], answered into position index[k] of the n-sized outputs; an entry outside [0, n) is skipped.
hipError_t launch_trace_rays_indexed(SceneView scene, const BvhView *bvh, const MeshView *mesh, const float *rays, int n, const int32_t *index, int m,
                                     float *t, int32_t *idx, float *hit, hipStream_t stream);
hipError_t launch_occluded_indexed(SceneView scene, const BvhView *bvh, const MeshView *mesh, float reach, const float *rays, const float *t_max, int n,
                                   const int32_t *index, int m, int32_t *occluded, hipStream_t stream);
// The k nearest hits along a caller's rays (ptmi_trace_rays_multi_device, ptmi_trace_rays_multi_indexed_device; ptmi_multi_hit.hip): one lane per
// ray -- per entry of `index` when that is not null, an entry outside [0, n) skipped -- writes row i of t and idx (n x k words) and count[i].
// t_max: n words, or null for +inf.  Rows are stored in 16-byte pieces when k % 4 == 0 and t and idx are 16-byte aligned.  Nothing is
// launched for n or m <= 0 or a k outside [1, PTMI_MULTI_HIT_MAX].
hipError_t launch_trace_rays_multi(SceneView scene, const BvhView *bvh, const MeshView *mesh, const float *rays, const float *t_max, int n,
                                   const int32_t *index, int m, int k, float *t, int32_t *idx, int32_t *count, hipStream_t stream);
// The nearest-primitive query over a caller's points (ptmi_nearest_device, ptmi_nearest_indexed_device; ptmi_nearest.hip): one lane per point --
// per entry of `index` when that is not null, an entry outside [0, n) skipped -- writes dist[i], idx[i] and, unless `point` is null, the
// nearest location into point[3 i ..].  r_max: n words, or null for +inf.  Nothing is launched for n or m <= 0.
hipError_t launch_nearest(SceneView scene, const BvhView *bvh, const MeshView *mesh, const float *points, const float *r_max, int n, const int32_t *index, int m,
                          float *dist, int32_t *idx, float *point, hipStream_t stream);
// Render Inline along a caller's rays (ptmi_trace_paths_device, ptmi_trace_paths_indexed_device; ptmi_paths.hip): one lane per ray -- per entry
// of `index` when that is not null, an entry outside [0, n) skipped -- adds n_spp samples of traceInline to color[i] (n x 3 words) and
// advances seed[i] (n x 4 words: a, b, c, counter).  Nothing is launched for n, m or n_spp <= 0.  path_seeds: seed[i] = genSeeds' state of
// index first_index + i (ptmi_path_seeds_device).
hipError_t launch_trace_paths(SceneView scene, const BvhView *bvh, const MeshView *mesh, const float *rays, int n, const int32_t *index, int m,
                              int bounce_limit, int n_spp, float *color, uint32_t *seed, hipStream_t stream);
hipError_t launch_path_seeds(uint64_t seed0, uint64_t first_index, int n, uint32_t *seed, hipStream_t stream);
// One bounce of a caller's paths (ptmi_bounce_rays_device, ptmi_bounce_rays_indexed_device; ptmi_bounce.hip): one lane per ray -- per entry of
// `index` when that is not null, an entry outside [0, n) skipped -- does one prepareRay on (rays[i], radiance[i], throughput[i], seed[i]) in
// place and writes the incoming ray's hit words to those of t, idx, hit that are not null.  Nothing is launched for n or m <= 0.
hipError_t launch_bounce_rays(SceneView scene, const BvhView *bvh, const MeshView *mesh, float *rays, int n, const int32_t *index, int m, float *throughput,
                              float *radiance, uint32_t *seed, float *t, int32_t *idx, float *hit, hipStream_t stream);
// Render Streams along a caller's rays (ptmi_trace_streams_device, ptmi_trace_streams_indexed_device; ptmi_trace_streams.hip): one lane per
// ray -- per entry of `index` when that is not null, an entry outside [0, n) skipped -- walks n_spp samples' ray trees depth first, adds every
// hit to color[i] and advances seed[i].  lost: two words (truncated, dropped), added to, or null.  work: trace_streams_bytes(lanes) bytes,
// 16-byte aligned; read and written only at a GLASS hit, so it may be null for a scene without GLASS.  Nothing is launched for n, m or n_spp <= 0.
size_t trace_streams_bytes(int count);
hipError_t launch_trace_streams(SceneView scene, const BvhView *bvh, const MeshView *mesh, const float *rays, int n, const int32_t *index, int m, int n_spp,
                                int step_cap, bool seed_from_result, float *color, uint32_t *seed, unsigned long long *lost, void *work, hipStream_t stream);
// The live list (ptmi_live_rays_device; ptmi_bounce.hip): live[0 .. *n_live) = the candidates -- index[0 .. count), or 0 .. count - 1 when index
// is null -- inside [0, n) whose throughput is not nearZero, in candidate order; -1 behind them up to count.  n_live may be null; live may be
// index.  work: live_rays_bytes(count) bytes, 8-byte aligned.
size_t live_rays_bytes(int count);
hipError_t launch_live_rays(const float *throughput, int n, const int32_t *index, int count, int32_t *live, int32_t *n_live, void *work, hipStream_t stream);
// A coherent order for n rays (ptmi_ray_order_device; ptmi_ray_order.hip): order[position] = ray, ascending by (ptmi_ray_order.h's key,
// index).  work: ray_order_bytes(n) bytes, 8-byte aligned -- the sort's scratch and the box words behind it.
size_t ray_order_bytes(int n);
hipError_t launch_ray_order(const float *rays, int n, void *work, int32_t *order, hipStream_t stream);
// Moving a mesh scene's vertices (ptmi_update_mesh_vertices; ptmi_mesh_refit.hip).  vertices: 9 floats per triangle by original index, device
// memory; leaf_pos: per triangle its position in the leaf order or -1; result: kRefitWords words (ptmi_mesh_box.h), all ones in
// [0, kRefitHi), zero behind, at launch.  check writes `result` only; records writes both copies of the records; level the boxes of
// `count` nodes whose children are complete (one launch per level of MeshRefitPlan, the deepest first).
hipError_t launch_mesh_refit_check(const float *vertices, int n, const int32_t *leaf_pos, unsigned int *result, hipStream_t stream);
hipError_t launch_mesh_refit_records(const float *vertices, int n, const int32_t *leaf_pos, float4 *by_index, float4 *geom, hipStream_t stream);
hipError_t launch_mesh_refit_level(float4 *nodes, const float4 *geom, const int32_t *level_nodes, int count, hipStream_t stream);
// New triangles for a mesh scene (ptmi_set_mesh_triangles; ptmi_mesh_build.hip).  triangles: n ptmi_triangle records (15 words each), device memory.  check
// writes `result` only (kBuildWords words, ptmi_mesh_morton.h: all ones in [0, kBuildHi), zero behind, at launch).  order: keys, the radix
// sort (scratch: mesh_build_sort_bytes(n) bytes, free once the launches are through), then leaf_pos (n) and order (n_kept) from the
// sorted indices; lo / hi: the box check found.  scatter: the records by index and in leaf order, and 2 n material float4.
hipError_t launch_mesh_build_check(const float *triangles, int n, unsigned int *result, hipStream_t stream);
size_t mesh_build_sort_bytes(int n);
hipError_t launch_mesh_build_order(const float *triangles, int n, int n_kept, const float lo[3], const float hi[3], void *scratch, int32_t *leaf_pos,
                                   int32_t *order, hipStream_t stream);
hipError_t launch_mesh_build_scatter(const float *triangles, int n, int n_kept, const int32_t *leaf_pos, float4 *by_index, float4 *geom, float4 *materials,
                                     hipStream_t stream);
// The builds' radix sort (ptmi_mesh_build.hip; the mesh build and the sphere build call it): n (key, index) pairs in `scratch`
// (mesh_build_sort_bytes(n) bytes: two key arrays, two index arrays, the tiles' digit counts; the pairs to sort in the first of each),
// ascending by key -- bits 0 .. 47 -- equal keys in their order.  *sorted: where the sorted indices lie afterwards (within scratch).
inline uint64_t *sort_keys(void *scratch, int) { return static_cast<uint64_t *>(scratch); }
inline uint32_t *sort_indices(void *scratch, int n) { return reinterpret_cast<uint32_t *>(static_cast<uint64_t *>(scratch) + 2 * (size_t)n); }
hipError_t launch_sort_pairs(void *scratch, int n, const uint32_t **sorted, hipStream_t stream);
// Moving or replacing the spheres of a BVH or mesh scene (ptmi_update_spheres, ptmi_set_bvh_spheres; ptmi_bvh_refit.hip).  spheres: n records
// of `words` floats by original index, device memory: 4 -- (x, y, z, radius) -- or 10 -- a ptmi_sphere.  check writes `result` only
// (kSphWords words, ptmi_bvh_box.h: all ones in [0, kSphHi), zero behind, at launch).  records: (c, r * r) into `geom` in leaf order and
// into the scene block's sphere rows, and with 10 words the material pairs (`materials`: the pair of sphere 0).  level: the boxes and
// inv_2r of `count` nodes whose children are complete (one launch per level of BvhLevelPlan, the deepest first).
hipError_t launch_bvh_check(const float *spheres, int words, int n, unsigned int *result, hipStream_t stream);
hipError_t launch_bvh_records(const float *spheres, int words, int n, const int32_t *order, float4 *geom, float4 *scene, float4 *materials, hipStream_t stream);
hipError_t launch_bvh_level(float4 *nodes, const float *spheres, int words, int n, const int32_t *order, const int32_t *level_nodes, int count, hipStream_t stream);
// The leaf order of ptmi_set_bvh_spheres (ptmi_bvh_build.hip): the Morton keys of the centres within lo / hi (the box check found), the
// sort above (scratch: mesh_build_sort_bytes(n) bytes), then order[position] = original index.
hipError_t launch_bvh_build_order(const float *spheres, int n, const float lo[3], const float hi[3], void *scratch, int32_t *order, hipStream_t stream);
// The spatial build of ptmi_set_bvh_spheres (PTMI_BVH_BUILD_SPATIAL; ptmi_bvh_lbvh.hip, ptmi_bvh_spatial.h).  tree: the keys in cubic cells, the
// sort above (scratch: mesh_build_sort_bytes(n) bytes; *sorted: the leaf order, within scratch), then two launches per level into `work`
// (bvh_spatial_work_bytes(n) bytes), whose report -- kSpatialWords ints at bvh_spatial_report: the levels' node counts, the equal-count
// splits taken -- the host reads.  finish: with those counts (`levels` of them, every one positive), the references into `nodes` and the
// nodes by level, the deepest first, into level_nodes.
size_t bvh_spatial_work_bytes(int n);
const int *bvh_spatial_report(void *work, int n);
hipError_t launch_bvh_spatial_tree(const float *spheres, int n, const float lo[3], const float hi[3], void *scratch, void *work, const uint32_t **sorted,
                                   hipStream_t stream);
hipError_t launch_bvh_spatial_finish(void *work, int n, const int *level_count, int levels, float4 *nodes, int32_t *level_nodes, hipStream_t stream);
unsigned int tree_workgroups(int width, int rows_local);   // workgroups per copy of its grid (RenderArgs.tree_stack holds kTreeFastLevels x 64 records of 64 B for each)
// 8x8 tiles leave lanes idle on the right and bottom edges; rows of 64 leave them idle at the end only
inline bool tiles_pay_dims(int width, int rows_local) { return width >= 64 && rows_local >= 16; }
inline bool tiles_pay(const RenderArgs &a) { return tiles_pay_dims(a.width, a.rows_local); }
// entries of quad_order / quad_cost (0 = tiles not used): the tile grid padded to a multiple of 32 (lane_pixel), four tiles to a quad
inline unsigned int quad_positions(int width, int rows_local)
{
    if (!tiles_pay_dims(width, rows_local)) return 0;
    const unsigned int tiles = (unsigned int)(((width + 7) / 8) * ((rows_local + 7) / 8));
    return ((tiles + 31u) & ~31u) / 4u;
}
hipError_t launch_quad_order(const unsigned int *cost, unsigned int *order, unsigned int *cls, unsigned int n, unsigned int *tail_start,
                             unsigned int tail_permille, hipStream_t stream);
bool uses_quad_order(const RenderArgs &a, int algorithm_inline, int variant);
hipError_t launch_seed(Planes p, int width, int rows_local, int stripe_rows, int n_parts, int part,
                       uint64_t seed0, bool clear_color, hipStream_t stream);
hipError_t launch_create_with(Planes p, const uint32_t *w0, const uint32_t *w1, const uint32_t *w2,
                              int64_t n, hipStream_t stream);
hipError_t launch_eval_sphere(const float *spheres10, const float *rays, int n,
                              int32_t *is_just, float *t, float *normalp, hipStream_t stream);
hipError_t launch_eval_plane(const float *planes12, const float *rays, int n,
                             int32_t *is_just, float *t, float *normalp, hipStream_t stream);
// group read-out: member `part`'s snapshot [3][rows][W] (stripes contiguous) into the whole image's planes [H][W]
hipError_t launch_stitch(const float *src, int rows, int width, int stripe_rows, int n_parts, int part,
                         float *r, float *g, float *b, hipStream_t stream);
hipError_t launch_present(Planes p, long long n, int iterations, float *rgb, uint32_t *rgba, hipStream_t stream);
hipError_t launch_eval_sincos(const float *x, int n, float *s, float *c, hipStream_t stream);
hipError_t launch_eval_quaternion(const float *half_angles, int n, float *q_out, hipStream_t stream);

// A launch that reports ITS OWN status.  `kernel<<<...>>>(...)` drops hipLaunchKernel's result, and hipGetLastError() afterwards hands out the
// thread's STICKY error -- the last failure of any runtime call, this library's or another's (an allocation the caller recovered from, an error
// ptmi_destroy ignored), kept until somebody asks: a launch that went out would be reported as failed.  Arguments are converted to the
// kernel's parameter types as a call would convert them.
template <typename Tuple, size_t... I>
inline hipError_t launch_packed(const void *kernel, dim3 grid, dim3 block, size_t lds_bytes, hipStream_t stream, Tuple &values, std::index_sequence<I...>)
{
    void *pointers[] = {static_cast<void *>(&std::get<I>(values))..., nullptr};
    return hipLaunchKernel(kernel, grid, block, pointers, lds_bytes, stream);
}
template <typename... P, typename... A>
inline hipError_t launch(void (*kernel)(P...), dim3 grid, dim3 block, size_t lds_bytes, hipStream_t stream, const A &...args)
{
    static_assert(sizeof...(P) == sizeof...(A), "one argument per kernel parameter");
    std::tuple<std::remove_cv_t<P>...> values(static_cast<P>(args)...);
    return launch_packed(reinterpret_cast<const void *>(kernel), grid, block, lds_bytes, stream, values, std::index_sequence_for<P...>{});
}

}  // namespace ptmi
