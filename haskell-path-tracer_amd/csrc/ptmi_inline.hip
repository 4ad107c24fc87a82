// ptmi_inline.hip -- render Inline (src/Scene/Trace.hs:193-200 + 344-383) for gfx950: the default kernel at every size.
//
//   * one lane per pixel; the seven state planes are read once and written once per launch, coalesced (x fastest), whatever the
//     sample count;
//   * the sample loop AND the bounce loop live in the kernel.  A lane whose path ends starts its pixel's next sample at once
//     ("regeneration"), so the 64 lanes of a wave stay busy although paths end after different numbers of bounces -- the
//     per-pixel order of RNG draws and of floating-point additions is exactly that of n_spp successive `render` calls;
//   * the primitive list is staged into LDS once per workgroup and read as wave-wide broadcasts (every lane walks the same
//     primitive at the same time);
//   * a trace's sphere candidates keep (tca, x, index) in their lanes and take their square roots in dense passes, 1.4 a trace on C2
//     where the whole wave ran the root 2.7 times (check_hit, ptmi_device.h: SphereFold::kStashSelect, the stash as selects);
//   * a shade whose outcome the next prepareRay is certain to freeze only adds its emittance and draws (surely_frozen_after);
//   * each LARGE block -- "start the pixel's next sample" -- is expanded once per trip: the sites that end a sample only set a
//     per-lane flag, and one block at the top of the next trip acts on it (three inlined copies cost 3 %);
//   * no MFMA: the work is scalar-per-lane f32/f64 VALU with divergent control flow.
// The ablation loops of DESIGN.md 5.2 (round 1's loop, regenerate-only, lock step, pooled shade round, persistent hand-out) are in
// ptmi_inline_ablations.hip, which only builds with -DPTMI_ABLATIONS.
// This unit is compiled a second time with -DPTMI_CONTRACTED_BUILD -ffp-contract=fast -Dptmi=ptmi_contracted (a * b + c fused: a
// labelled measurement mode, see the end of the file).
#include "ptmi_mesh_device.h"

namespace ptmi {

namespace {

// ---------------------------------------------------------------------------------------
// render Inline.  LDS_SCENE: primitives staged in LDS (default) or read straight from global memory through scalar loads
// (scenes over 3 KB).  TILE_W: the wave's pixels are an 8 x 8 tile (8) or 64 consecutive pixels of a row (0).
// The primary hit is evaluated once per pixel; loop [finish frozen shades + restart][shade][trace].
// ---------------------------------------------------------------------------------------
// (the diagnostic counters a trace passes to the hit search, or none: the primary hit's)
__device__ __forceinline__ unsigned int *hit_diag(unsigned int *counters = nullptr) { return counters; }

#ifndef PTMI_INLINE_WAVES
#define PTMI_INLINE_WAVES 7      // 72 VGPRs (three registers spilled around the loop, not in it) and a 10-word LDS column: C2 3.10 -> 3.04 ms
#endif
template <bool LDS_SCENE, int TILE_W = 0>
__global__ void __launch_bounds__(kRenderBlock, PTMI_INLINE_WAVES) render_inline_kernel(const RenderArgs a)
{
#define PTMI_HIT(STAGED, S, ns, np, o, d, ...) check_hit<STAGED, SphereFold::kStashSelect, SphereShare::kXY>(S, ns, np, o, d, hit_diag(__VA_ARGS__), a.scene.share_xy)
#define PTMI_HIT_RECORD hit_record
#define PTMI_NORMAL_AT normal_at
#include "ptmi_inline_body.inc"
#undef PTMI_HIT_RECORD
#undef PTMI_NORMAL_AT
#undef PTMI_HIT
}

// ... for a scene staged in LDS in which no sphere shares its predecessor's cx and cy (SceneView.share_xy == 0: mainScene): the same body, every
// sphere running the whole test -- the kernel as it was before the sharing, instruction for instruction (tools/isa_diff.py), so that such
// a scene pays nothing for the mask: no bit test, no branch.  The choice is the launcher's (launch_linear): the mask is known on the host.
// (Inside one kernel a second, untested walk costs a spill more than the budget allows: experiments/shared_xy/.)
template <int TILE_W = 0>
__global__ void __launch_bounds__(kRenderBlock, PTMI_INLINE_WAVES) render_inline_kernel_plain(const RenderArgs a)
{
    constexpr bool LDS_SCENE = true;
#define PTMI_HIT(STAGED, ...) check_hit<STAGED, SphereFold::kStashSelect>(__VA_ARGS__)
#define PTMI_HIT_RECORD hit_record
#define PTMI_NORMAL_AT normal_at
#include "ptmi_inline_body.inc"
#undef PTMI_HIT_RECORD
#undef PTMI_NORMAL_AT
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
#define PTMI_HIT_RECORD hit_record
#define PTMI_NORMAL_AT normal_at
#include "ptmi_inline_body.inc"
#undef PTMI_HIT_RECORD
#undef PTMI_NORMAL_AT
#undef PTMI_HIT
}

// mesh scenes (ptmi_set_scene_mesh): the same body, spheres ++ planes ++ triangles searched through the two hierarchies (check_hit_mesh),
// a triangle's hit record from its stored normal
template <int TILE_W>
__global__ void __launch_bounds__(kRenderBlock, PTMI_BVH_WAVES) render_inline_mesh_kernel(const RenderArgs a, const MeshView mesh)
{
    constexpr bool LDS_SCENE = false;
#define PTMI_HIT(STAGED, S, ns, np, o, d, ...) check_hit_mesh(mesh, S, ns, np, o, d)
#define PTMI_HIT_RECORD(S, ns, idx, o, d, t, p, n) mesh_hit_record(mesh, S, ns, np, idx, o, d, t, p, n)
#define PTMI_NORMAL_AT(S, ns, idx, p) mesh_normal_at(mesh, S, ns, np, idx, p)
#include "ptmi_inline_body.inc"
#undef PTMI_HIT_RECORD
#undef PTMI_NORMAL_AT
#undef PTMI_HIT
}
#endif

// the linear scenes' kernel: the scene staged in LDS or read through scalar loads, waves on tiles or rows as `mapping` says
hipError_t launch_linear(const RenderArgs &a, Mapping mapping, bool lds_scene, hipStream_t stream)
{
    // (the scalar-load form is one kernel: a scene that big walks a mask of its first 64 spheres only, and pays its tests either way)
    if (lds_scene && a.scene.share_xy == 0ull)
        return launch_per_pixel(a, mapping, render_inline_kernel_plain<8>, render_inline_kernel_plain<0>, true, PTMI_INLINE_WAVES, 16, stream);
    if (lds_scene) return launch_per_pixel(a, mapping, render_inline_kernel<true, 8>, render_inline_kernel<true>, true, PTMI_INLINE_WAVES, 16, stream);
    return launch_per_pixel(a, mapping, render_inline_kernel<false, 8>, render_inline_kernel<false>, false, PTMI_INLINE_WAVES, 16, stream);
}

}  // namespace

hipError_t launch_render_inline(const RenderArgs &a, const BvhView *bvh, int variant, hipStream_t stream)
{
    if (renders_nothing(a)) return hipSuccess;
#ifndef PTMI_CONTRACTED_BUILD
    if (bvh) return launch_per_pixel(a, Mapping::kAuto, render_inline_bvh_kernel<8>, render_inline_bvh_kernel<0>, false, PTMI_BVH_WAVES, 16, stream, *bvh);
#endif
    // static mapping wins at every size measured; a scene so big that staging it per wave would cost more occupancy than
    // scalar loads cost speed is read through scalar loads (every route); the cached kernel handles the degenerate counts (iterate 0; no sample at all)
    const bool lds_scene = scene_fits_lds(a);
    if (variant == kVariantAuto || a.bounce_limit <= 0 || a.n_spp <= 0) return launch_linear(a, Mapping::kAuto, lds_scene, stream);
    if (!lds_scene) {                                         // the LDS forms would not fit or would cap occupancy
        if (variant == kVariantPersistent) variant = kVariantPersistentScalar;
        else if (variant == kVariantRows || variant == kVariantCapped4 || variant == kVariantCapped3) variant = kVariantRowsScalar;
        else if (variant >= kVariantTiles && variant <= kVariantTiles32x2) variant = kVariantTilesScalar;
    }
    switch (variant) {
    case kVariantRows:        return launch_linear(a, Mapping::kRows, true, stream);
    case kVariantRowsScalar:  return launch_linear(a, Mapping::kRows, false, stream);
    case kVariantTiles:       return launch_linear(a, Mapping::kTiles, true, stream);
    case kVariantTilesScalar: return launch_linear(a, Mapping::kTiles, false, stream);
    default: break;
    }
#if defined(PTMI_ABLATIONS) && !defined(PTMI_CONTRACTED_BUILD)
    const dim3 grid(blocks_for((long long)a.rows_local * a.width, kRenderBlock)), block(kRenderBlock);
    const size_t lds = (size_t)a.scene.total_f4() * sizeof(float4);
    if (variant >= kVariantTiles16x4 && variant <= kVariantTiles32x2) {       // other pixel tiles per wave: 16x4 / 4x16 / 32x2 (8x8 is handled above)
        const int tw = variant == kVariantTiles16x4 ? 16 : variant == kVariantTiles4x16 ? 4 : 32;
        const dim3 tgrid(tile_grid(a, tw));
        if (tw == 16) return launch(render_inline_kernel<true, 16>, tgrid, block, lds, stream, a);
        if (tw == 4)  return launch(render_inline_kernel<true, 4>, tgrid, block, lds, stream, a);
        return launch(render_inline_kernel<true, 32>, tgrid, block, lds, stream, a);
    }
    if (variant == kVariantCapped4 || variant == kVariantCapped3)             // capped occupancy through dynamic LDS: 4 / 3 waves per SIMD
        return launch(render_inline_kernel<true>, grid, block, (variant == kVariantCapped4 ? 33 : 41) * 1024, stream, a);
    return launch_render_inline_ablation(a, variant, !lds_scene, stream);      // ptmi_inline_ablations.hip
#else
    return hipErrorInvalidValue;                             // ptmi_set_variant admits only what the build holds
#endif
}

#ifndef PTMI_CONTRACTED_BUILD
hipError_t launch_render_inline_mesh(const RenderArgs &a, const MeshView &mesh, hipStream_t stream)
{
    return launch_per_pixel(a, Mapping::kAuto, render_inline_mesh_kernel<8>, render_inline_mesh_kernel<0>, false, PTMI_BVH_WAVES, 16, stream, mesh);
}

bool variant_available(int variant)
{
    switch (variant) {
    case kVariantAuto: case kVariantRows: case kVariantRowsScalar: case kVariantStreamForm: case kVariantTiles: case kVariantTilesScalar: return true;
    default: break;
    }
#ifdef PTMI_ABLATIONS
    return variant >= 0 && variant < kVariantCount;
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
    return (int)ptmi::launch_render_inline(*static_cast<const ptmi::RenderArgs *>(args), nullptr, variant, static_cast<hipStream_t>(stream));
}
#endif
