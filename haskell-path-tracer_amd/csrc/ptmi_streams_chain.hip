// ptmi_streams_chain.hip -- render Streams (src/Scene/Trace.hs:141-191, 272-331), one chain per pixel: the default of Streams for
// every scene whose rays never split, and the per-pixel TAIL of the stream form (ptmi_stream_pixels.hip).
#include "ptmi_mesh_device.h"

namespace ptmi {

namespace {

// ---------------------------------------------------------------------------------------
// render Streams (Trace.hs:141-191, 272-331).  The reference keeps one ray per pixel in a stream
// that `expand` compacts after every step (numNewRays is 0 or 1, Trace.hs:329-331) and scatters the
// colours back with `permute (+)`; because a pixel never owns more than one ray, the stream is the
// per-pixel chain below and the compaction becomes "a lane whose ray died starts its pixel's next
// sample" -- the wave stays dense without moving ray state through memory.  What differs from
// Inline, and is reproduced literally:
//   * every hit adds emittance * throughput straight into the accumulator, also in the step where the
//     throughput is already near zero (computeResult runs for every intersection, Trace.hs:290-293);
//   * the ray dies when nearZero throughput || miss (Trace.hs:329-331); there is NO bounce limit -- a
//     non-empty stream is never stopped by the iteration count (Trace.hs:166-170).  a.stream_step_cap only
//     guarantees that the kernel terminates (rays it cuts are counted, stream_counters[kScTruncated]);
//   * which seed the pixel carries out of `combine` (Trace.hs:179-184) is Accelerate-backend behaviour
//     (assumption A5).  Default: the pixel keeps its OLD seed while the sample runs;
//     a.seed_from_result: the seed of the ray that made the sample's LAST hit replaces it (kept in the lane's LDS
//     column, not in registers).  Either way updateSeed then advances the pixel's seed by one
//     draw (Trace.hs:151, :190-191).
// ---------------------------------------------------------------------------------------

#ifndef PTMI_STREAMS_WAVES
#define PTMI_STREAMS_WAVES 7     // 72 VGPRs (one pair spilled around the loop, not in it): C2 4.27 -> 4.17 ms
#endif
template <bool LDS_SCENE, int TILE_W = 0>
__global__ void __launch_bounds__(kRenderBlock, PTMI_STREAMS_WAVES) render_streams_kernel(const RenderArgs a)
{
#define PTMI_HIT(STAGED, ...) check_hit<STAGED>(__VA_ARGS__)
#define PTMI_HIT_RECORD hit_record
#define PTMI_NORMAL_AT normal_at
#include "ptmi_streams_chain_body.inc"
#undef PTMI_HIT_RECORD
#undef PTMI_NORMAL_AT
#undef PTMI_HIT
}

// BVH scenes (ptmi_set_scene_bvh): the same body, the spheres searched through the hierarchy (check_hit_bvh); the packed scene
// (materials, planes) is read through scalar loads, as for every scene too big for LDS.
template <int TILE_W>
__global__ void __launch_bounds__(kRenderBlock, PTMI_BVH_WAVES) render_streams_bvh_kernel(const RenderArgs a, const BvhView bvh)
{
    constexpr bool LDS_SCENE = false;
#define PTMI_HIT(STAGED, S, ns, np, o, d, ...) check_hit_bvh(bvh, S, ns, np, o, d)
#define PTMI_HIT_RECORD hit_record
#define PTMI_NORMAL_AT normal_at
#include "ptmi_streams_chain_body.inc"
#undef PTMI_HIT_RECORD
#undef PTMI_NORMAL_AT
#undef PTMI_HIT
}

// mesh scenes (ptmi_set_scene_mesh): the same body, spheres ++ planes ++ triangles searched through the two hierarchies (check_hit_mesh)
template <int TILE_W>
__global__ void __launch_bounds__(kRenderBlock, PTMI_BVH_WAVES) render_streams_mesh_kernel(const RenderArgs a, const MeshView mesh)
{
    constexpr bool LDS_SCENE = false;
#define PTMI_HIT(STAGED, S, ns, np, o, d, ...) check_hit_mesh(mesh, S, ns, np, o, d)
#define PTMI_HIT_RECORD(S, ns, idx, o, d, t, p, n) mesh_hit_record(mesh, S, ns, np, idx, o, d, t, p, n)
#define PTMI_NORMAL_AT(S, ns, idx, p) mesh_normal_at(mesh, S, ns, np, idx, p)
#include "ptmi_streams_chain_body.inc"
#undef PTMI_HIT_RECORD
#undef PTMI_NORMAL_AT
#undef PTMI_HIT
}

// the linear scenes' kernel: the scene staged in LDS or read through scalar loads, waves on tiles or rows as `mapping` says
hipError_t launch_linear(const RenderArgs &a, Mapping mapping, bool lds_scene, hipStream_t stream)
{
    if (lds_scene) return launch_per_pixel(a, mapping, render_streams_kernel<true, 8>, render_streams_kernel<true>, true, PTMI_STREAMS_WAVES, 16, stream);
    return launch_per_pixel(a, mapping, render_streams_kernel<false, 8>, render_streams_kernel<false>, false, PTMI_STREAMS_WAVES, 16, stream);
}

}  // namespace

hipError_t launch_render_streams(const RenderArgs &a, const BvhView *bvh, int variant, hipStream_t stream)
{
    if (hipError_t e = clear_stream_iterations(a, stream)) return e;
    if (bvh) return launch_per_pixel(a, Mapping::kAuto, render_streams_bvh_kernel<8>, render_streams_bvh_kernel<0>, false, PTMI_BVH_WAVES, 16, stream, *bvh);
    const bool rows = variant == kVariantRows || variant == kVariantRowsScalar;          // 4 / 5 keep the row mapping (ablation)
    const bool scalar = variant == kVariantRowsScalar || variant == kVariantPersistentScalar || variant == kVariantTilesScalar;
    return launch_linear(a, rows ? Mapping::kRows : Mapping::kAuto, !scalar && scene_fits_lds(a), stream);
}

hipError_t launch_render_streams_mesh(const RenderArgs &a, const MeshView &mesh, hipStream_t stream)
{
    if (hipError_t e = clear_stream_iterations(a, stream)) return e;
    return launch_per_pixel(a, Mapping::kAuto, render_streams_mesh_kernel<8>, render_streams_mesh_kernel<0>, false, PTMI_BVH_WAVES, 16, stream, mesh);
}

// The per-pixel chain kernel as the TAIL of a stream-form launch: a grid over every dispatch position whose workgroups start at
// *first_position (RenderArgs.first_position); no sample chunks; stream_iterations is the stream form's to clear.
hipError_t launch_render_streams_tail(const RenderArgs &a, const unsigned int *first_position, hipStream_t stream)
{
    if (!tiles_pay(a) || !first_position) return hipSuccess;
    RenderArgs b = a;
    b.spp_chunks = 1; b.first_position = first_position;
    return launch_linear(b, Mapping::kTiles, scene_fits_lds(a), stream);
}

}  // namespace ptmi
