// ptmi_inline.hip -- render Inline (src/Scene/Trace.hs:193-200 + 344-383) for gfx950: the default kernel at every size.
//
//   * one lane per pixel; the seven state planes are read once and written once per launch, coalesced (x fastest), whatever the
//     sample count;
//   * the sample loop AND the bounce loop live in the kernel.  A lane whose path ends starts its pixel's next sample at once
//     ("regeneration"), so the 64 lanes of a wave stay busy although paths end after different numbers of bounces -- the
//     per-pixel order of RNG draws and of floating-point additions is exactly that of n_spp successive `render` calls;
//   * the primitive list is staged into LDS once per workgroup and read as wave-wide broadcasts (every lane walks the same
//     primitive at the same time);
//   * a shade whose outcome the next prepareRay is certain to freeze only adds its emittance and draws (surely_frozen_after);
//   * each LARGE block -- "start the pixel's next sample" -- is expanded once per trip: the sites that end a sample only set a
//     per-lane flag, and one block at the top of the next trip acts on it (three inlined copies cost 3 %);
//   * no MFMA: the work is scalar-per-lane f32/f64 VALU with divergent control flow.
// The ablation loops of DESIGN.md 5.2 (round 1's loop, regenerate-only, lock step, pooled shade round, persistent hand-out) are in
// ptmi_inline_ablations.hip, which only builds with -DPTMI_ABLATIONS.
// This unit is compiled a second time with -DPTMI_CONTRACTED_BUILD -ffp-contract=fast -Dptmi=ptmi_contracted (a * b + c fused: a
// labelled measurement mode, see the end of the file).
#include "ptmi_bvh_device.h"

namespace ptmi {

namespace {

// ---------------------------------------------------------------------------------------
// render Inline.  LDS_SCENE: primitives staged in LDS (default) or read straight from global memory through scalar loads
// (scenes over 3 KB).  TILE_W: the wave's pixels are an 8 x 8 tile (8) or 64 consecutive pixels of a row (0).
// The primary hit is evaluated once per pixel; loop [finish frozen shades + restart][shade][trace].
// ---------------------------------------------------------------------------------------
#ifndef PTMI_INLINE_WAVES
#define PTMI_INLINE_WAVES 7      // 72 VGPRs (three registers spilled around the loop, not in it) and a 10-word LDS column: C2 3.10 -> 3.04 ms
#endif
template <bool LDS_SCENE, int TILE_W = 0>
__global__ void __launch_bounds__(kRenderBlock, PTMI_INLINE_WAVES) render_inline_kernel(const RenderArgs a)
{
#define PTMI_HIT(STAGED, ...) check_hit<STAGED>(__VA_ARGS__)
#include "ptmi_inline_body.inc"
#undef PTMI_HIT
}

#ifndef PTMI_CONTRACTED_BUILD
// BVH scenes (ptmi_set_scene_bvh): the same body, the spheres searched through the hierarchy (check_hit_bvh); the packed scene
// (materials, planes) is read through scalar loads, as for every scene too big for LDS.
template <int TILE_W>
__global__ void __launch_bounds__(kRenderBlock, PTMI_BVH_WAVES) render_inline_bvh_kernel(const RenderArgs a, const BvhView bvh)
{
    constexpr bool LDS_SCENE = false;
#define PTMI_HIT(STAGED, S, ns, np, o, d, ...) check_hit_bvh(bvh, S, ns, np, o, d)
#include "ptmi_inline_body.inc"
#undef PTMI_HIT
}
#endif

}  // namespace

// Which render Inline kernel a variant is (ptmi_set_variant):
//   0 auto | 4 cached, a wave = 64 consecutive pixels of a row (LDS scene) | 5 the same with the scene through scalar loads
//   13 = 4 with 8x8 pixel tiles per wave | 17 = 5 with 8x8 tiles -- these are what auto chooses from.
// Only in builds with -DPTMI_ABLATIONS (ptmi_set_variant refuses them otherwise):
//   1 / 6 persistent hand-out (LDS / scalar-load scene) | 2 lock step | 3 regenerate | 7 / 8 capped occupancy
//   10-12 pooled second shade round | 14-16 other tile shapes | 18 round 1's loop
hipError_t launch_render_inline(const RenderArgs &a, int variant, hipStream_t stream)
{
    const long long n_local = (long long)a.rows_local * a.width;
    if (n_local <= 0) return hipSuccess;
    const dim3 grid(blocks_for(n_local, kRenderBlock)), block(kRenderBlock);
    const size_t lds = (size_t)a.scene.total_f4() * sizeof(float4);
    const bool big_scene = lds > kMaxSceneLds;               // every route reads such a scene through scalar loads, not LDS
    const bool degenerate = a.bounce_limit <= 0 || a.n_spp <= 0;   // the cached kernel handles both (iterate 0; no sample at all)
    if (variant == 0 || degenerate) {
        // static mapping wins at every size measured; a scene so big that staging it per wave would cost more occupancy than scalar loads cost speed is
        // read through scalar loads; 8x8 tiles once the image is big enough for whole tiles to dominate
        const bool tiles = tiles_pay(a);
        variant = !big_scene ? (tiles ? 13 : 4) : (tiles ? 17 : 5);
    }
    if (big_scene) {                                         // the LDS forms would not fit or would cap occupancy
        if (variant == 1) variant = 6;
        else if (variant == 4 || variant == 7 || variant == 8) variant = 5;
        else if (variant >= 13 && variant <= 16) variant = 17;
    }
    if (variant == 17 || variant == 13) {
        RenderArgs b = a;
        const unsigned int per_copy = tile_grid(a, 8);
        if (hipError_t e = choose_sample_chunks(b, per_copy, PTMI_INLINE_WAVES, stream)) return e;
        const dim3 cgrid(per_copy * (unsigned int)b.spp_chunks);
        return variant == 17 ? launch(render_inline_kernel<false, 8>, cgrid, block, 0, stream, b)
                             : launch(render_inline_kernel<true, 8>, cgrid, block, lds, stream, b);
    }
    if (variant == 5) return launch(render_inline_kernel<false>, grid, block, 0, stream, a);
    if (variant == 4) return launch(render_inline_kernel<true>, grid, block, lds, stream, a);
#if defined(PTMI_ABLATIONS) && !defined(PTMI_CONTRACTED_BUILD)
    if (variant >= 14 && variant <= 16) {                     // other pixel tiles per wave: 16x4 / 4x16 / 32x2 (8x8 is handled above)
        const int tw = variant == 14 ? 16 : variant == 15 ? 4 : 32;
        const dim3 tgrid(tile_grid(a, tw));
        if (tw == 16) return launch(render_inline_kernel<true, 16>, tgrid, block, lds, stream, a);
        if (tw == 4)  return launch(render_inline_kernel<true, 4>, tgrid, block, lds, stream, a);
        return launch(render_inline_kernel<true, 32>, tgrid, block, lds, stream, a);
    }
    if (variant == 7 || variant == 8) {                       // capped occupancy through dynamic LDS: 4 / 3 waves per SIMD
        return launch(render_inline_kernel<true>, grid, block, (variant == 7 ? 33 : 41) * 1024, stream, a);
    }
    return launch_render_inline_ablation(a, variant, big_scene, stream);      // ptmi_inline_ablations.hip
#else
    return hipErrorInvalidValue;                             // ptmi_set_variant admits only what the build holds
#endif
}

#ifndef PTMI_CONTRACTED_BUILD
// render Inline on a BVH scene: the automatic choice of the linear scenes' launcher (8x8 tiles with sample chunks once the image has whole tiles,
// rows of 64 otherwise); the degenerate counts go through the same kernel.  No variants: ptmi_set_variant refuses them.
hipError_t launch_render_inline_bvh(const RenderArgs &a, const BvhView &bvh, hipStream_t stream)
{
    const long long n_local = (long long)a.rows_local * a.width;
    if (n_local <= 0) return hipSuccess;
    const dim3 block(kRenderBlock);
    if (tiles_pay(a)) {
        RenderArgs b = a;
        const unsigned int per_copy = tile_grid(a, 8);
        if (hipError_t ce = choose_sample_chunks(b, per_copy, PTMI_BVH_WAVES, stream)) return ce;
        return launch(render_inline_bvh_kernel<8>, dim3(per_copy * (unsigned int)b.spp_chunks), block, 0, stream, b, bvh);
    }
    return launch(render_inline_bvh_kernel<0>, dim3(blocks_for(n_local, kRenderBlock)), block, 0, stream, a, bvh);
}

bool variant_available(int variant)
{
    if (variant == 0 || variant == 4 || variant == 5 || variant == 9 || variant == 13 || variant == 17) return true;
#ifdef PTMI_ABLATIONS
    return variant >= 0 && variant <= 18;
#else
    return false;
#endif
}
#endif

}  // namespace ptmi

#ifdef PTMI_CONTRACTED_BUILD
// THE CONTRACTED-ARITHMETIC OBJECT.  This unit is compiled a second time with -ffp-contract=fast and -Dptmi=ptmi_contracted
// (every name above then lives in namespace ptmi_contracted): the same kernel with a * b + c contracted into fused
// multiply-adds wherever the source writes it -- dot products, cross products, the rotation, the quaternion.  It is NOT the
// reference's arithmetic as this repository reads it (every operation rounded on its own); it exists to
// MEASURE how much of the kernel's time that reading costs (PTMI_OPT_ARITHMETIC, never the default, never the headline).  One C
// entry, because the two objects' RenderArgs are distinct types of identical layout.
extern "C" int ptmi_contracted_launch_inline(const void *args, int variant, void *stream)
{
    return (int)ptmi::launch_render_inline(*static_cast<const ptmi::RenderArgs *>(args), variant, static_cast<hipStream_t>(stream));
}
#endif
