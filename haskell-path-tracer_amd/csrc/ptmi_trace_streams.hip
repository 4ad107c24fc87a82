// ptmi_trace_streams.hip -- render Streams along a caller's own device-resident rays (ptmi_trace_streams_device,
// ptmi_trace_streams_indexed_device).  For ray i, n_spp times: the sample's ray TREE is walked depth first from (ray_i, throughput 1, the
// ray's seed), every hit adds emittance * throughput to color_i, and the seed advances one draw -- what render_streams_tree_kernel does
// for a pixel (ptmi_streams_tree_body.inc) and, on a scene without GLASS, what render_streams_kernel does (ptmi_streams_chain_body.inc),
// with the ray read from memory where those kernels compute a camera's.  One lane per ray, one wave per workgroup; nothing here
// synchronises or allocates.
//   * the arithmetic is the render kernels' own: check_hit / check_hit_bvh / check_hit_mesh, hit_record / mesh_hit_record, normal_at,
//     gen_component, quaternion_from_half_angles, rotate, glass_children, glass_refraction_child -- every one general in the direction's
//     length;
//   * the loop is the tree walk's, written a second time (the two *_body.inc files are left alone: their kernels stay instruction for
//     instruction what they were): [dead ray][fetch next work][shade with GLASS as an arm][trace], the START RECORD in a lane-private LDS
//     column -- the ray's first hit, or, for a glass first hit whose children the cap cannot cut, the first hits of both children with the
//     lead seed --, the waiting children's first kTreeFastLevels levels as 64-byte records in the caller's workspace, [workgroup][level][lane],
//     and the deeper ones in scratch memory;
//   * the seed rule: under PTMI_SEED_FROM_RESULT every hit leaves the seed its ray carried in the ray's seed (only ever without GLASS:
//     the entry points refuse the pair, so the lead seed and this rule never meet);
//   * one kernel per scene kind (RayScene, ptmi_ray_lane_device.h, whose frame this lane stands in; kSharedXyLds is not instantiated): a
//     linear scene staged in LDS, a linear scene too big for LDS through scalar loads, a BVH scene and a mesh scene on check_hit_bvh's LDS
//     stack;
//   * the index is lane_ray's wave-uniform null test: lane k < m takes i = index[k] and skips an entry outside [0, n);
//   * what the step cap cut and what a full stack dropped go to lost[0] and lost[1], summed per wave, only when there was something.
// Memory: rays, colour and seeds as in ptmi_paths.hip (load_ray, load_seed and store_seed of ptmi_ray_lane_device.h).
#define PTMI_MESH_EXACT_INLINE __forceinline__
#include "ptmi_ray_lane_device.h"

namespace ptmi {

namespace {

#ifndef PTMI_TREE_WAVES
#define PTMI_TREE_WAVES 6        // the tree walk's occupancy budget (ptmi_streams_tree.hip)
#endif

constexpr int kSeedFromResult = 4;     // StreamRayArgs.flags, beside kWideRays

struct StreamRayArgs {
    SceneView scene;
    const float *rays;           // [n][6]
    const int32_t *index;        // [m], or null: lane k takes ray k
    int n, m;
    int n_spp, step_cap;
    int flags;                   // kWideRays, kSeedFromResult
    float *color;                // [n][3]
    uint32_t *seed;              // [n][4]: a, b, c, counter
    unsigned long long *lost;    // [2]: truncated, dropped; or null
    float4 *work;                // the lanes' first waiting children; null only when the scene holds no GLASS (nothing is ever pushed then)
};

template <RayScene KIND>
__device__ __forceinline__ void trace_streams_lane(const StreamRayArgs &a, const MeshView &uniform_mesh)
{
    constexpr bool LDS_SCENE = staged_in_lds(KIND);
    constexpr int kEntry = 10;                               // words per start hit: position, incoming direction, throughput, primitive | steps | draws
    __shared__ uint32_t start_rec[2 * kEntry][kRenderBlock];
    const int ns = a.scene.n_spheres, np = a.scene.n_planes;
    const float4 *S = stage_scene<KIND>(a.scene);
    if (LDS_SCENE) {
        stage_glass_constants(const_cast<float4 *>(S), a.scene);      // (S is the workgroup's own copy)
        __syncthreads();
    }
    // (a hierarchy kernel's counts and caps are held per lane, as its boxes and here its leaves' index arrays: per_lane)
    const float4 *M = S + (is_hierarchy(KIND) ? per_lane(a.scene.geom_f4()) : a.scene.geom_f4());
    const MeshView mesh = per_lane_view<KIND>(uniform_mesh, std::true_type{});
    auto record = [&](int idx, V3 o, V3 d, float t, V3 &p, V3 &n) { record_hit<KIND>(mesh, S, ns, np, idx, o, d, t, p, n); };
    auto normal_of = [&](int idx, V3 p) -> V3 {
        if constexpr (is_mesh(KIND)) return mesh_normal_at(mesh, S, ns, np, idx, p);
        else return normal_at(S, ns, idx, p);
    };
    // 24 bits of primitive (PTMI_MAX_BVH_SPHERES + PTMI_MAX_BVH_PLANES + PTMI_MAX_MESH_TRIANGLES <= 2^24), steps (0 or 1) at bit 24, draws (0 or 1) at bit 25
    static_assert(PTMI_MAX_BVH_SPHERES + PTMI_MAX_BVH_PLANES + PTMI_MAX_MESH_TRIANGLES <= (1 << 24), "the start record holds 24 bits of primitive");

    int ray;
    if (!lane_ray(a.index, a.n, a.m, ray)) return;          // (nothing below needs the whole wave)
    const int i = ray;
    unsigned int cut = 0, dropped = 0;
    {
        V3 origin, primary;
        load_ray(a.rays, i, a.flags & kWideRays, origin, primary);
        // (the lane keeps its ray's number, not the two addresses, across the walk: four registers less)
        V3 acc;
        Sfc32 pixel_seed;
        {
            const float *c = a.color + 3 * (size_t)i;
            const uint32_t *seed_p = a.seed + 4 * (size_t)i;
            acc = mk(c[0], c[1], c[2]);
            load_seed(seed_p, seed_is_wide(seed_p), pixel_seed);
        }
        const int n_spp = is_hierarchy(KIND) ? per_lane(a.n_spp) : a.n_spp;
        const unsigned int step_cap = (unsigned int)(is_hierarchy(KIND) ? per_lane(a.step_cap) : a.step_cap);
        const int from_result = is_hierarchy(KIND) ? per_lane(a.flags & kSeedFromResult) : a.flags & kSeedFromResult;
        // the seed rule as a mask of all ones (PTMI_SEED_FROM_RESULT) or none: the seed a hit's ray carried is taken by bit selection, so that
        // no comparison's lane mask lives in scalar registers across the loop
        const uint32_t take = 0u - ((uint32_t)from_result / (uint32_t)kSeedFromResult);
        auto note_hit_seed = [&](const Sfc32 &sd) {                 // combine new old: the seed this hit's ray carried
            pixel_seed.a = (sd.a & take) | (pixel_seed.a & ~take); pixel_seed.b = (sd.b & take) | (pixel_seed.b & ~take);
            pixel_seed.c = (sd.c & take) | (pixel_seed.c & ~take); pixel_seed.counter = (sd.counter & take) | (pixel_seed.counter & ~take);
        };

        {
            uint32_t *rec = &start_rec[0][threadIdx.x];
            auto put_entry = [&](int e, V3 p, V3 dir, V3 t, uint32_t word) {
                uint32_t *q = rec + (size_t)e * kEntry * kRenderBlock;
                q[0] = f2u(p.x); q[kRenderBlock] = f2u(p.y); q[2 * kRenderBlock] = f2u(p.z);
                q[3 * kRenderBlock] = f2u(dir.x); q[4 * kRenderBlock] = f2u(dir.y); q[5 * kRenderBlock] = f2u(dir.z);
                q[6 * kRenderBlock] = f2u(t.x); q[7 * kRenderBlock] = f2u(t.y); q[8 * kRenderBlock] = f2u(t.z);
                q[9 * kRenderBlock] = word;
            };
            V3 pos = origin, normal = mk(0.0f, 0.0f, 0.0f);       // pos: the hit to shade, then the next ray's origin
            // what is known of the start record, in one word: the first hit's primitive (24 bits), the number of start hits (kEntries, 2 bits),
            // kPrefix: the first hit is glass and its children's first hits are the start hits, kReflectionFirst: start hit 0 is the
            // reflection child's.  (A word, not flags: see `state` below.)
            enum : uint32_t { kEntriesShift = 24, kPrefix = 1u << 26, kReflectionFirst = 1u << 27 };
            uint32_t info = 0;
            // The lane's waiting children, a stack: origin, direction, throughput, seed, step index.  Its first kTreeFastLevels entries are
            // 64-byte records in the workspace -- a push is four 16-byte stores to one line --, the deeper ones live in scratch memory.
            uint32_t stack_w[kTreeStackDepth - kTreeFastLevels][14];
            float4 *const fast = a.work + ((size_t)blockIdx.x * kTreeFastLevels * kRenderBlock + threadIdx.x) * 4;
            // (the lane's state is one word, not three flags: a flag that lives across trips is a lane mask in two scalar registers)
            // kFirst: the ray's own trace, the same for every sample; kChild0 / kChild1: those of a glass first hit's children.  They are the
            // loop's first traces, so that the hit search is expanded once in the kernel.
            enum : int { kDone = 0, kPending = 1, kEnded = 2, kHasRay = 3, kFirst = 4, kChild0 = 5, kChild1 = 6 };
            int state = kFirst;
            int sp = 0, entry_i = 0;
            int s = -1, idx = 0;                                  // s: the sample being walked; -1 until the start record stands
            unsigned int steps = 0;
            V3 d = primary;
            V3 throughput = mk(1.0f, 1.0f, 1.0f);
            Sfc32 seed = pixel_seed;
            auto begin_sample = [&]() {                           // what every sample of this ray has already behind it
                if (info & kPrefix) {                             // computeResult of the glass first hit, the same in every sample
                    const float4 ma0 = M[2 * (info & 0xffffffu)];
                    acc = acc + (scale_r(mk(ma0.x, ma0.y, ma0.z), ma0.w) * mk(1.0f, 1.0f, 1.0f));
                }
                entry_i = 0;
            };
            // the next hit this sample starts from -- or, when it has none left, the end of the sample and the next one
            auto next_start = [&]() {
                for (;;) {
                    if (entry_i < (int)((info >> kEntriesShift) & 3u)) {
                        const uint32_t *q = rec + (size_t)entry_i * kEntry * kRenderBlock;
                        pos = mk(u2f(q[0]), u2f(q[kRenderBlock]), u2f(q[2 * kRenderBlock]));
                        d = mk(u2f(q[3 * kRenderBlock]), u2f(q[4 * kRenderBlock]), u2f(q[5 * kRenderBlock]));
                        throughput = mk(u2f(q[6 * kRenderBlock]), u2f(q[7 * kRenderBlock]), u2f(q[8 * kRenderBlock]));
                        const uint32_t word = q[9 * kRenderBlock];
                        idx = (int)(word & 0xffffffu);
                        ++entry_i;
                        steps = (word >> 24) & 1u;
                        normal = normal_of(idx, pos);
                        seed = pixel_seed;                        // (with a prefix: the lead seed)
                        if (word >> 25) (void)sfc32_next(seed);   // the refraction child: one more
                        state = kPending;
                        return;
                    }
                    if (s >= 0) (void)random_float(pixel_seed);   // updateSeed: the sample's tree is done
                    ++s;
                    if (s >= n_spp) { state = kDone; return; }
                    begin_sample();
                }
            };
            auto lineage_ended = [&]() {
                if (sp > 0) {                                     // the most recent waiting child
                    --sp;
                    uint32_t e[14];
                    if (sp < kTreeFastLevels) {
                        const float4 *r = fast + (size_t)sp * kRenderBlock * 4;
                        const float4 r0 = r[0], r1 = r[1], r2 = r[2], r3 = r[3];
                        e[0] = f2u(r0.x); e[1] = f2u(r0.y); e[2] = f2u(r0.z); e[3] = f2u(r0.w); e[4] = f2u(r1.x); e[5] = f2u(r1.y); e[6] = f2u(r1.z);
                        e[7] = f2u(r1.w); e[8] = f2u(r2.x); e[9] = f2u(r2.y); e[10] = f2u(r2.z); e[11] = f2u(r2.w); e[12] = f2u(r3.x); e[13] = f2u(r3.y);
                    } else {
                        const int q0 = sp - kTreeFastLevels;
                        for (int q = 0; q < 14; ++q) e[q] = stack_w[q0 < kTreeStackDepth - kTreeFastLevels ? q0 : 0][q];
                    }
                    pos = mk(u2f(e[0]), u2f(e[1]), u2f(e[2]));
                    d = mk(u2f(e[3]), u2f(e[4]), u2f(e[5]));
                    throughput = mk(u2f(e[6]), u2f(e[7]), u2f(e[8]));
                    seed.a = e[9]; seed.b = e[10]; seed.c = e[11]; seed.counter = e[12];
                    steps = e[13];
                    state = kHasRay;
                } else {
                    next_start();
                }
            };
            while (state != kDone) {
                // A ray whose throughput is already near zero dies at this hit (numNewRays): the hit adds its emittance and nothing else
                // of it survives.  Such a lane, and one whose lineage ended in the previous trip (miss, cap), fetches its next piece of
                // work -- its most recent waiting child, its sample's next start hit or the ray's next sample -- in ONE block.
                if (state == kPending && near_zero(throughput)) {
                    const float4 ma = M[2 * idx];
                    acc = acc + (scale_r(mk(ma.x, ma.y, ma.z), ma.w) * throughput);   // computeResult
                    note_hit_seed(seed);
                    ++steps;
                    state = kEnded;
                }
                if (state == kEnded) lineage_ended();
                // (A start hit that the block above has just loaded can itself belong to a dead ray: it waits for the next trip.)
                if (state == kPending && !near_zero(throughput)) {     // alive
                    // GLASS is an arm of the one shade, operation for operation the oracle's glass_children (glass_refraction_child)
                    const float4 ma = M[2 * idx], mb = M[2 * idx + 1];
                    const bool capped = steps + 1u >= step_cap;
                    const bool glass = f2u(mb.x) == 2u, matte = f2u(mb.x) == 0u;
                    const V3 color = mk(ma.x, ma.y, ma.z);
                    note_hit_seed(seed);
                    V3 rv;
                    rv.x = gen_component(seed); rv.y = gen_component(seed); rv.z = gen_component(seed);
                    const float ia = dot(d, normal);
                    const V3 reflection = d - scale_l(2.0f * ia, normal);
                    ++steps;
                    float glass_R = 0.0f;
                    if (glass) {                                  // the refraction child
                        V3 ko, kd, kt; Sfc32 ks;
                        glass_R = glass_refraction_child(color, glass_constants_of<LDS_SCENE>(mb), pos, normal, d, ia, reflection, throughput, seed, ko, kd, kt, ks);
                        // while the cached reflection's subtree is walked, the cached refraction "waits": one slot less
                        if (capped) {
                        } else if (sp < kTreeStackDepth - ((entry_i == 1 && (info & (kPrefix | kReflectionFirst)) == (kPrefix | kReflectionFirst)) ? 1 : 0)) {
                            if (sp < kTreeFastLevels) {
                                float4 *r = fast + (size_t)sp * kRenderBlock * 4;
                                r[0] = float4{ko.x, ko.y, ko.z, kd.x};
                                r[1] = float4{kd.y, kd.z, kt.x, kt.y};
                                r[2] = float4{kt.z, u2f(ks.a), u2f(ks.b), u2f(ks.c)};
                                r[3] = float4{u2f(ks.counter), u2f(steps), 0.0f, 0.0f};
                            } else {
                                const uint32_t e[14] = {f2u(ko.x), f2u(ko.y), f2u(ko.z), f2u(kd.x), f2u(kd.y), f2u(kd.z),
                                                        f2u(kt.x), f2u(kt.y), f2u(kt.z), ks.a, ks.b, ks.c, ks.counter, steps};
                                const int q0 = sp - kTreeFastLevels;
                                for (int q = 0; q < 14; ++q) stack_w[q0 < kTreeStackDepth - kTreeFastLevels ? q0 : 0][q] = e[q];
                            }
                            ++sp;
                        } else {
                            ++dropped;
                        }
                    }
                    // Matte: rotate (anglesToQuaternion $ pi *^ rv) iNormal | Glossy: rotate (anglesToQuaternion $ (1 - p) *^ rv) reflection
                    const V3 axis = matte ? normal : reflection;
                    const float hk = matte ? 0.5f * kPi : mb.w;
                    const V3 rotated = rotate(quaternion_from_half_angles(hk * rv.x, hk * rv.y, hk * rv.z), axis);
                    const float nd = dot(rotated, axis);
                    const float brdf = matte ? mb.z * nd : __builtin_fmaxf(0.0f, nd);
                    constexpr float next_ray_prob = 1.0f / (kPi * 2.0f);
                    const float factor = glass ? glass_R : brdf * next_ray_prob;
                    const V3 next = mk(glass ? reflection.x : rotated.x, glass ? reflection.y : rotated.y, glass ? reflection.z : rotated.z);
                    // results: colour += emittance * throughput for EVERY hit; then the new ray
                    acc = acc + (scale_r(color, ma.w) * throughput);
                    pos = pos + scale_r(next, kEpsilon);
                    d = next;
                    throughput = throughput * scale_r(color, factor);
                    if (capped) { cut += glass ? 2u : 1u; state = kEnded; }
                    else state = kHasRay;
                }
                if (state >= kHasRay) {
                    // the hit search: the render tree kernels'
                    const HitSel h = closest_hit<KIND, kStagedWalk, SphereFold::kStash, SphereShare::kNone>(mesh, S, ns, np, 0ull, pos, d);
                    V3 hp = pos, hn = normal;
                    if (h.just) record(h.idx, pos, d, h.t, hp, hn);
                    if (state == kHasRay) {
                        state = kEnded;
                        if (h.just) { pos = hp; normal = hn; idx = h.idx; state = kPending; }
                    } else if (state == kFirst) {
                        if (!h.just) {
                            int left = n_spp;                      // updateSeed only (the launcher sends n_spp > 0 only)
                            do (void)random_float(pixel_seed); while (--left > 0);
                            state = kDone;
                        } else {
                            // THE START RECORD: what every sample of this ray starts from
                            const float4 ma0 = M[2 * h.idx], mb0 = M[2 * h.idx + 1];
                            info = (uint32_t)h.idx;
                            // a glass first hit whose children cannot be cut: GLASS and a step cap of 3 or more (at most 2^30, so the
                            // difference's sign bit says it), in ONE comparison of a value the loop cannot hoist as a lane mask
                            if (((f2u(mb0.x) ^ 2u) | ((step_cap - 3u) >> 31)) == 0u) {
                                info |= kPrefix;
                                V3 ko[2], kd[2], kt[2]; Sfc32 ks[2];
                                glass_children(mk(ma0.x, ma0.y, ma0.z), glass_constants_of<LDS_SCENE>(mb0), hp, hn, d, mk(1.0f, 1.0f, 1.0f), pixel_seed, ko, kd, kt, ks);
                                put_entry(0, ko[0], kd[0], kt[0], 0u);         // the children's rays wait where their first hits will stand
                                put_entry(1, ko[1], kd[1], kt[1], 0u);
                                // THE LEAD SEED (ptmi_streams_tree_body.inc): from here to the end of the ray `pixel_seed` holds the ray's seed
                                // advanced by 3 raw draws -- the reflection child's seed as it stands, the refraction child's one step further
                                // -- and is stepped back three times before it is stored.
                                (void)sfc32_next(pixel_seed); (void)sfc32_next(pixel_seed); (void)sfc32_next(pixel_seed);
                                pos = ko[0]; d = kd[0];
                                state = kChild0;
                            } else {
                                put_entry(0, hp, d, mk(1.0f, 1.0f, 1.0f), (uint32_t)h.idx);
                                info |= 1u << kEntriesShift; entry_i = 1;
                                state = kEnded;                    // the next trip starts sample 0 from the record
                            }
                        }
                    } else {                                       // a glass first hit's child: its first hit, if any, is a start hit
                        const int e = state - kChild0;
                        if (h.just) {
                            const uint32_t *q = rec + (size_t)e * kEntry * kRenderBlock;
                            const V3 rt = mk(u2f(q[6 * kRenderBlock]), u2f(q[7 * kRenderBlock]), u2f(q[8 * kRenderBlock]));
                            const int n_entries = (int)((info >> kEntriesShift) & 3u);
                            if (n_entries == 0 && e == 0) info |= kReflectionFirst;
                            put_entry(n_entries, hp, d, rt, (uint32_t)h.idx | (1u << 24) | ((uint32_t)e << 25));
                            info += 1u << kEntriesShift;
                        }
                        if (e == 0) {
                            const uint32_t *q = rec + (size_t)kEntry * kRenderBlock;
                            pos = mk(u2f(q[0]), u2f(q[kRenderBlock]), u2f(q[2 * kRenderBlock]));
                            d = mk(u2f(q[3 * kRenderBlock]), u2f(q[4 * kRenderBlock]), u2f(q[5 * kRenderBlock]));
                            state = kChild1;
                        } else {
                            entry_i = (int)((info >> kEntriesShift) & 3u);
                            state = kEnded;                        // the next trip starts sample 0 from the record
                        }
                    }
                }
            }
            if (info & kPrefix) { sfc32_prev(pixel_seed); sfc32_prev(pixel_seed); sfc32_prev(pixel_seed); }     // the lead seed back to the ray's
        }
        float *c = a.color + 3 * (size_t)i;
        uint32_t *seed_p = a.seed + 4 * (size_t)i;
        c[0] = acc.x; c[1] = acc.y; c[2] = acc.z;
        store_seed(seed_p, seed_is_wide(seed_p), pixel_seed);
    }
    if (__any((cut | dropped) != 0u)) {                               // rare: one add per word and wave, summed over the lanes that lost something
        unsigned long long n_cut = 0, n_dropped = 0;
        for (unsigned long long lanes = __ballot((cut | dropped) != 0u); lanes; lanes &= lanes - 1) {
            const int lane = (int)__builtin_ctzll(lanes);
            n_cut += (unsigned int)__builtin_amdgcn_readlane((int)cut, lane); n_dropped += (unsigned int)__builtin_amdgcn_readlane((int)dropped, lane);
        }
        if (a.lost && (int)(threadIdx.x & 63) == (int)__builtin_ctzll(__ballot(1))) {
            if (n_cut) atomicAdd(a.lost, n_cut);
            if (n_dropped) atomicAdd(a.lost + 1, n_dropped);
        }
    }
}

// One kernel per scene kind, under a name that says which (a BVH scene's view travels in the mesh view's sphere part)
#define PTMI_STREAM_RAYS_KERNEL(NAME, KIND, WAVES)                                                                                   \
    __global__ void __launch_bounds__(kRenderBlock, WAVES) trace_streams_##NAME##_kernel(const StreamRayArgs a, const MeshView mesh) \
    {                                                                                                                                \
        trace_streams_lane<KIND>(a, mesh);                                                                                           \
    }
PTMI_STREAM_RAYS_KERNEL(linear_lds, RayScene::kLinearLds, PTMI_TREE_WAVES)
PTMI_STREAM_RAYS_KERNEL(linear_scalar, RayScene::kLinearScalar, PTMI_TREE_WAVES)
PTMI_STREAM_RAYS_KERNEL(bvh, RayScene::kBvh, PTMI_BVH_WAVES)
PTMI_STREAM_RAYS_KERNEL(mesh, RayScene::kMesh, PTMI_BVH_WAVES)
#undef PTMI_STREAM_RAYS_KERNEL

}  // namespace

// the first kTreeFastLevels waiting children of every lane: 64-byte records, [workgroup][level][lane]
size_t trace_streams_bytes(int count)
{
    if (count <= 0) return 0;
    const size_t workgroups = ((size_t)count + kRenderBlock - 1) / kRenderBlock;
    return workgroups * kTreeFastLevels * kRenderBlock * 64;
}

hipError_t launch_trace_streams(SceneView scene, const BvhView *bvh, const MeshView *mesh, const float *rays, int n, const int32_t *index, int m, int n_spp,
                                int step_cap, bool seed_from_result, float *color, uint32_t *seed, unsigned long long *lost, void *work, hipStream_t stream)
{
    const int lanes = index ? m : n;
    if (n <= 0 || lanes <= 0 || n_spp <= 0) return hipSuccess;
    StreamRayArgs a;
    a.scene = scene; a.rays = rays; a.index = index; a.n = n; a.m = m;
    a.n_spp = n_spp; a.step_cap = step_cap;
    a.flags = (aligned8(rays) ? kWideRays : 0) | (seed_from_result ? kSeedFromResult : 0);
    a.color = color; a.seed = seed; a.lost = lost; a.work = static_cast<float4 *>(work);
    // (no kernel of its own for shared-xy runs: the tree walk's check_hit does not follow them)
    return launch_by_scene(scene, bvh, mesh, trace_streams_mesh_kernel, trace_streams_bvh_kernel, trace_streams_linear_scalar_kernel, trace_streams_linear_lds_kernel,
                           trace_streams_linear_lds_kernel, lanes, stream, a);
}

}  // namespace ptmi
