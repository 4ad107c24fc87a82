// ptmi_paths.hip -- render Inline along a caller's own device-resident rays (ptmi_trace_paths_device, ptmi_trace_paths_indexed_device) and
// the seeds such a caller starts from (ptmi_path_seeds_device).  For ray i, n_spp times: (new, seed') = traceInline limit scene ray_i seed_i;
// color_i = new + color_i; seed_i = seed' -- what render_inline_kernel does for a pixel (ptmi_inline_body.inc), with the ray read from
// memory where that kernel computes a camera's.  One lane per ray, one wave per workgroup; nothing here synchronises, allocates or stages.
//   * the arithmetic is the render kernels' own: check_hit / check_hit_bvh / check_hit_mesh, hit_record / mesh_hit_record, bounce_axis,
//     next_about_axis, apply_bounce, surely_frozen_after, finish_frozen -- every one general in the direction's length;
//   * the loop is render Inline's, written a second time (ptmi_inline_body.inc is left alone: its kernels stay instruction for instruction
//     what they were): the ray's first hit once -- as the loop's first trace, so that the hit search is expanded once per kernel --, the
//     restart record -- hit position, axis, half-angle scale, accumulator -- in a lane-private LDS column of 10 words, and
//     [finish frozen][restart][shade][trace] with regeneration across the n_spp samples;
//   * one kernel per scene kind: a linear scene staged in LDS, without and with shared-xy runs (as launch_linear chooses), a linear scene
//     too big for LDS through scalar loads, a BVH scene and a mesh scene on check_hit_bvh's LDS stack;
//   * the index is a wave-uniform null test: lane k < m takes i = index[k] and skips an entry outside [0, n).
// The frame around the loop -- the scene kinds, the staging, the words held per lane, the search by kind, the lane's ray, the seed's load
// and store, the launcher's choice -- is ptmi_ray_lane_device.h's, shared with ptmi_bounce.hip and ptmi_trace_streams.hip.
// Memory: a ray as load_ray loads it (three 8-byte loads when the array is 8-byte aligned, six dwords otherwise); the seed one
// 16-byte load and store when its array is 16-byte aligned (four dwords otherwise); the colour three dwords, 12 bytes apart.
// The mesh scene's literal fold is inlined as in ptmi_query.hip: no kernel of this unit has any scratch.
#define PTMI_MESH_EXACT_INLINE __forceinline__
#include "ptmi_ray_lane_device.h"

namespace ptmi {

namespace {

struct PathArgs {
    SceneView scene;
    const float *rays;           // [n][6]
    const int32_t *index;        // [m], or null: lane k takes ray k
    int n, m;
    int bounce_limit, n_spp;
    int flags;                   // kWideRays
    float *color;                // [n][3]
    uint32_t *seed;              // [n][4]: a, b, c, counter
};

template <RayScene KIND>
__device__ __forceinline__ void trace_path_lane(const PathArgs &a, const MeshView &uniform_mesh)
{
    __shared__ float path_const[10][kRenderBlock];          // per-lane restart record (see below)
    const int ns = a.scene.n_spheres, np = a.scene.n_planes;
    const float4 *S = stage_scene<KIND>(a.scene);
    // (a mesh kernel's counts and limits are held per lane, as its boxes: per_lane)
    const float4 *M = S + (is_mesh(KIND) ? per_lane(a.scene.geom_f4()) : a.scene.geom_f4());
    const MeshView mesh = per_lane_view<KIND>(uniform_mesh, std::false_type{});
    // (the record behind a local name, the search called where it is made: the shapes that keep these kernels' code)
    auto record = [&](int idx, V3 o, V3 d, float t, V3 &p, V3 &n) { record_hit<KIND>(mesh, S, ns, np, idx, o, d, t, p, n); };

    int ray;
    if (!lane_ray(a.index, a.n, a.m, ray)) return;
    const int i = ray;

    V3 origin, primary;
    load_ray(a.rays, i, a.flags & kWideRays, origin, primary);
    float *c = a.color + 3 * (size_t)i;
    uint32_t *sp = a.seed + 4 * (size_t)i;
    V3 acc = mk(c[0], c[1], c[2]);
    Sfc32 seed;
    load_seed(sp, seed_is_wide(sp), seed);
    const int limit = is_mesh(KIND) ? per_lane(a.bounce_limit) : a.bounce_limit;
    const int n_spp = is_mesh(KIND) ? per_lane(a.n_spp) : a.n_spp;

    {
        // iterate 0 (limit <= 0): every sample returns (0, seed); new + old (the launcher sends n_spp > 0 only), and no trip of the loop.
        // Otherwise: every sample of a ray shoots the same ray, so its checkHit + hit are evaluated ONCE and every sample starts from that record.
        // Loop shape, as render Inline's: a lane comes round with a hit to shade (kPending), with its sample over (kOver: the trace
        // missed, or the last shade left a throughput that the next prepareRay freezes) or with a ray to trace (kHasRay).  The shades whose
        // outcome is CERTAIN to be frozen (the iteration limit, or surely_frozen_after) are finished first -- emittance + three draws -- and
        // those lanes are over too; then ONE block restarts every such lane on its ray's next sample, from the cached first hit; then one
        // full shade and one trace for all.  The ray's own trace is the loop's first (s == -2): the hit search is expanded once in the
        // kernel, and what a sample restarts from -- the position of that hit, the axis and half-angle scale of its bounce, the accumulator
        // -- goes into the lane-private LDS column then.  A ray that misses ends there: every sample's result is 0, the seed untouched.
        if (limit <= 0) acc = mk(0.0f, 0.0f, 0.0f) + acc;
        float *mine = &path_const[0][threadIdx.x];
        auto put = [&](int w, float v) { mine[w * kRenderBlock] = v; };
        auto get = [&](int w) { return mine[w * kRenderBlock]; };
        put(7, acc.x); put(8, acc.y); put(9, acc.z);
        // (the lane's state is one word, not three flags: a flag that lives across trips is a lane mask in two scalar registers, and the
        // hierarchies' kernels have none to spare)
        enum : int { kDone = 0, kPending = 1, kOver = 2, kHasRay = 3 };
        int state = limit > 0 ? kHasRay : kDone;
        int s = -2, it = 0, idx = 0, idx0 = 0;                // s: the sample being traced; -2 until the ray's own trace is through (the first restart makes it 0)
        V3 pos = origin, d = primary, normal = mk(0.0f, 0.0f, 0.0f);     // pos: the hit to shade, then the next ray's origin
        V3 throughput = mk(1.0f, 1.0f, 1.0f), result = mk(0.0f, 0.0f, 0.0f);
        while (state != kDone) {
            float4 mb = M[2 * idx + 1];
            V3 axis = mk(0.0f, 0.0f, 0.0f); float hk = 0.0f;
            if (state == kPending) {
                bounce_axis(mb, normal, d, axis, hk);
                const float4 ma = M[2 * idx];
                if (it + 1 >= limit || surely_frozen_after(ma, mb, axis, throughput)) {
                    finish_frozen(ma, throughput, result, seed);
                    state = kOver;
                }
            }
            if (state == kOver) {                              // next sample of this ray
                // \(new, seed') (old, _) -> (new + old, seed') -- once a sample has been traced
                if (s >= 0) { put(7, result.x + get(7)); put(8, result.y + get(8)); put(9, result.z + get(9)); }
                ++s; it = 0;
                throughput = mk(1.0f, 1.0f, 1.0f); result = mk(0.0f, 0.0f, 0.0f);
                pos = mk(get(0), get(1), get(2)); idx = idx0;
                mb = M[2 * idx0 + 1];
                axis = mk(get(3), get(4), get(5)); hk = get(6);
                state = s < n_spp ? kPending : kDone;
            }
            if (state == kPending) {
                V3 next; float brdf;
                next_about_axis(mb, axis, hk, seed, next, brdf);
                apply_bounce(M, idx, pos, next, brdf, pos, d, throughput, result);
                ++it;
                // the next prepareRay would freeze the path (Trace.hs:364-365)
                state = (it >= limit || near_zero(throughput)) ? kOver : kHasRay;
            }
            if (state == kHasRay) {
                const HitSel h = closest_hit<KIND, true, SphereFold::kStashSelect, SphereShare::kXY>(mesh, S, ns, np, a.scene.share_xy, pos, d);
                const bool first = s < -1;
                if (h.just) {
                    record(h.idx, pos, d, h.t, pos, normal);
                    idx = h.idx;
                    state = kPending;
                    if (first) {                               // the restart record; the lane starts sample 0 on the next trip
                        V3 axis0; float hk0;
                        bounce_axis(M[2 * idx + 1], normal, d, axis0, hk0);
                        put(0, pos.x); put(1, pos.y); put(2, pos.z);
                        put(3, axis0.x); put(4, axis0.y); put(5, axis0.z); put(6, hk0);
                        idx0 = idx;
                        s = -1;
                        state = kOver;
                    }
                } else if (first) {
                    put(7, 0.0f + get(7)); put(8, 0.0f + get(8)); put(9, 0.0f + get(9));     // every sample: new = 0; 0 + old
                    state = kDone;
                } else {
                    state = kOver;
                }
            }
        }
        acc = mk(get(7), get(8), get(9));
    }

    c[0] = acc.x; c[1] = acc.y; c[2] = acc.z;
    store_seed(sp, seed_is_wide(sp), seed);
}

// One kernel per scene kind, under a name that says which (a BVH scene's view travels in the mesh view's sphere part)
#define PTMI_PATH_KERNEL(NAME, KIND, WAVES)                                                                                          \
    __global__ void __launch_bounds__(kRenderBlock, WAVES) trace_paths_##NAME##_kernel(const PathArgs a, const MeshView mesh)        \
    {                                                                                                                                \
        trace_path_lane<KIND>(a, mesh);                                                                                              \
    }
PTMI_PATH_KERNEL(linear_lds, RayScene::kLinearLds, PTMI_INLINE_WAVES)
PTMI_PATH_KERNEL(shared_xy_lds, RayScene::kSharedXyLds, PTMI_INLINE_WAVES)
PTMI_PATH_KERNEL(linear_scalar, RayScene::kLinearScalar, PTMI_INLINE_WAVES)
PTMI_PATH_KERNEL(bvh, RayScene::kBvh, PTMI_BVH_WAVES)
PTMI_PATH_KERNEL(mesh, RayScene::kMesh, PTMI_BVH_WAVES)
#undef PTMI_PATH_KERNEL

// genSeeds for a caller's rays: seed i is the state ptmi_init_output(seed0) gives pixel first_index + i of an unpartitioned image (seed_kernel)
__global__ void __launch_bounds__(kBlock) path_seeds_kernel(uint64_t seed0, uint64_t first_index, int n, int wide, uint32_t *seed)
{
    const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const uint64_t index = first_index + (uint64_t)i;
    const Sfc32 s = sfc32_seed3(seed_word(seed0, index, 0), seed_word(seed0, index, 1), seed_word(seed0, index, 2));
    uint32_t *sp = seed + 4 * (size_t)i;
    if (wide) {
        *reinterpret_cast<uint4 *>(sp) = uint4{s.a, s.b, s.c, s.counter};
    } else {
        sp[0] = s.a; sp[1] = s.b; sp[2] = s.c; sp[3] = s.counter;
    }
}

}  // namespace

hipError_t launch_path_seeds(uint64_t seed0, uint64_t first_index, int n, uint32_t *seed, hipStream_t stream)
{
    if (n <= 0) return hipSuccess;
    return launch(path_seeds_kernel, dim3(blocks_for(n)), dim3(kBlock), 0, stream, seed0, first_index, n, aligned16(seed) ? 1 : 0, seed);
}

hipError_t launch_trace_paths(SceneView scene, const BvhView *bvh, const MeshView *mesh, const float *rays, int n, const int32_t *index, int m,
                              int bounce_limit, int n_spp, float *color, uint32_t *seed, hipStream_t stream)
{
    const int lanes = index ? m : n;
    if (n <= 0 || lanes <= 0 || n_spp <= 0) return hipSuccess;
    PathArgs a;
    a.scene = scene; a.rays = rays; a.index = index; a.n = n; a.m = m;
    a.bounce_limit = bounce_limit; a.n_spp = n_spp;
    a.flags = aligned8(rays) ? kWideRays : 0;
    a.color = color; a.seed = seed;
    return launch_by_scene(scene, bvh, mesh, trace_paths_mesh_kernel, trace_paths_bvh_kernel, trace_paths_linear_scalar_kernel, trace_paths_shared_xy_lds_kernel,
                           trace_paths_linear_lds_kernel, lanes, stream, a);
}

}  // namespace ptmi
