// ptmi_streams_chain.hip -- render Streams (src/Scene/Trace.hs:141-191, 272-331), one chain per pixel: the default of Streams for
// every scene whose rays never split, and the per-pixel TAIL of the stream form (ptmi_stream_pixels.hip).
#include "ptmi_bvh_device.h"

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
#include "ptmi_streams_chain_body.inc"
#undef PTMI_HIT
}

// BVH scenes (ptmi_set_scene_bvh): the same body, the spheres searched through the hierarchy (check_hit_bvh); the packed scene
// (materials, planes) is read through scalar loads, as for every scene too big for LDS.
template <int TILE_W>
__global__ void __launch_bounds__(kRenderBlock, PTMI_BVH_WAVES) render_streams_bvh_kernel(const RenderArgs a, const BvhView bvh)
{
    constexpr bool LDS_SCENE = false;
#define PTMI_HIT(STAGED, S, ns, np, o, d, ...) check_hit_bvh(bvh, S, ns, np, o, d)
#include "ptmi_streams_chain_body.inc"
#undef PTMI_HIT
}

}  // namespace

hipError_t launch_render_streams(const RenderArgs &a, int variant, hipStream_t stream)
{
    const long long n_local = (long long)a.rows_local * a.width;
    if (n_local <= 0) return hipSuccess;
    const dim3 grid(blocks_for(n_local, kRenderBlock)), block(kRenderBlock);
    const size_t lds = (size_t)a.scene.total_f4() * sizeof(float4);
    hipError_t e = hipMemsetAsync(a.stream_iterations, 0, (size_t)kStatShards * 2 * kStatStride * sizeof(unsigned int), stream);   // every shard: the figure is per launch
    if (e != hipSuccess) return e;
    const bool scalar_scene = variant == 5 || variant == 6 || variant == 17 || lds > kMaxSceneLds;
    const bool tiles = variant == 4 || variant == 5 ? false : tiles_pay(a);      // 4 / 5 keep the row mapping (ablation)
    if (tiles) {
        RenderArgs b = a;
        const unsigned int per_copy = tile_grid(a, 8);
        if (hipError_t ce = choose_sample_chunks(b, per_copy, PTMI_STREAMS_WAVES, stream)) return ce;
        const dim3 tgrid(per_copy * (unsigned int)b.spp_chunks);
        if (scalar_scene) return launch(render_streams_kernel<false, 8>, tgrid, block, 0, stream, b);
        else              return launch(render_streams_kernel<true, 8>, tgrid, block, lds, stream, b);
    } else {
        if (scalar_scene) return launch(render_streams_kernel<false>, grid, block, 0, stream, a);
        else              return launch(render_streams_kernel<true>, grid, block, lds, stream, a);
    }
}

// render Streams on a BVH scene: the automatic choice of the linear scenes' launcher (8x8 tiles with sample chunks once the image has whole tiles,
// rows of 64 otherwise); the degenerate counts go through the same kernel.  No variants: ptmi_set_variant refuses them.
hipError_t launch_render_streams_bvh(const RenderArgs &a, const BvhView &bvh, hipStream_t stream)
{
    const long long n_local = (long long)a.rows_local * a.width;
    if (n_local <= 0) return hipSuccess;
    const dim3 block(kRenderBlock);
    hipError_t e = hipMemsetAsync(a.stream_iterations, 0, (size_t)kStatShards * 2 * kStatStride * sizeof(unsigned int), stream);
    if (e != hipSuccess) return e;
    if (tiles_pay(a)) {
        RenderArgs b = a;
        const unsigned int per_copy = tile_grid(a, 8);
        if (hipError_t ce = choose_sample_chunks(b, per_copy, PTMI_BVH_WAVES, stream)) return ce;
        return launch(render_streams_bvh_kernel<8>, dim3(per_copy * (unsigned int)b.spp_chunks), block, 0, stream, b, bvh);
    }
    return launch(render_streams_bvh_kernel<0>, dim3(blocks_for(n_local, kRenderBlock)), block, 0, stream, a, bvh);
}

// The per-pixel chain kernel as the TAIL of a stream-form launch: a grid over every dispatch position whose workgroups start at
// *first_position (RenderArgs.first_position); no sample chunks; stream_iterations is the stream form's to clear.
hipError_t launch_render_streams_tail(const RenderArgs &a, const unsigned int *first_position, hipStream_t stream)
{
    if (!tiles_pay(a) || !first_position) return hipSuccess;
    RenderArgs b = a;
    b.spp_chunks = 1; b.first_position = first_position;
    const size_t lds = (size_t)a.scene.total_f4() * sizeof(float4);
    const dim3 grid(tile_grid(a, 8)), block(kRenderBlock);
    if (lds > kMaxSceneLds) return launch(render_streams_kernel<false, 8>, grid, block, 0, stream, b);
    else                    return launch(render_streams_kernel<true, 8>, grid, block, lds, stream, b);
}

}  // namespace ptmi
