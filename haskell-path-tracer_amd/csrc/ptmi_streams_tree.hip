// ptmi_streams_tree.hip -- render Streams for scenes whose rays SPLIT (the build-defined GLASS extension), per-pixel form: the
// tree walk (the default with GLASS).  The stream form of the same algorithm is ptmi_stream_split.hip.
#include "ptmi_mesh_device.h"

namespace ptmi {

namespace {

// ---------------------------------------------------------------------------------------
// render Streams for scenes whose rays SPLIT (the build-defined GLASS extension), per-pixel form: the tree walk.
// A lane owns a pixel and walks each sample's ray TREE depth first: at a GLASS hit the reflection child continues in
// the lane and the refraction child waits on a lane-private stack (scratch memory); when a lineage ends the lane pops
// the most recent waiting child, and only when the stack is empty does it go on with the sample's next start hit or
// the pixel's next sample.  Compared with the stream form below: no ray ever travels through HBM queues, a colour word
// has ONE adder (no atomics, and the order of a pixel's additions is defined: depth first, reflection before
// refraction -- oracle: ora_render_streams_tree, bit-exact), and the waves are dispatched by recorded cost, exactly as in
// render_streams_kernel.  The set of rays traced is the stream algorithm's (same children, same seeds, same step
// indices); a child that finds kTreeStackDepth children waiting in its lane is dropped and counted.
//
// THE START RECORD.  Every sample of a pixel shoots the same primary ray (Trace.hs:244-262), and a GLASS hit involves no
// random draw that changes a direction (glass_children only ADVANCES the seed): if the primary hit is glass, its two
// children are the same two rays in every sample too.  So what is evaluated once per pixel and kept in a lane-private
// LDS column is not only the primary hit but, for a glass primary hit, the first hit of EACH child -- the hits a sample
// starts from (0, 1 or 2 of them; a child that misses contributes nothing).  A sample then adds the glass hit's
// emittance (the same value every time), counts its two children, and works through its start hits in tree order, each
// with the seed its ray would carry: the sample's seed advanced by 3 (reflection) or 4 (refraction) raw draws.  Two
// traces and one glass evaluation per sample disappear for such pixels; everything downstream -- including start hits
// that are glass themselves -- takes the general path.  (With a step cap below 3 the children could be cut: no caching.)
// ---------------------------------------------------------------------------------------
#ifndef PTMI_TREE_WAVES
#define PTMI_TREE_WAVES 6        // 80 VGPRs (three values spilled around the shade) and a start record of 2 x 10 words: 8.39 -> 7.96 ms on the glass scene
#endif
template <bool LDS_SCENE, int TILE_W = 0>
__global__ void __launch_bounds__(kRenderBlock, PTMI_TREE_WAVES) render_streams_tree_kernel(const RenderArgs a)
{
#define PTMI_HIT(STAGED, ...) check_hit<STAGED>(__VA_ARGS__)
#define PTMI_HIT_RECORD hit_record
#define PTMI_NORMAL_AT normal_at
// a linear scene has at most PTMI_MAX_PRIMITIVES = 1024 primitives: 16 bits of primitive, steps at bit 16, draws at bit 24
#define PTMI_TREE_PACK(prim, steps, draws) ((uint32_t)(prim) | ((steps) << 16) | ((draws) << 24))
#define PTMI_TREE_PRIM(w) ((w) & 0xffffu)
#define PTMI_TREE_META(w) ((w) >> 16)
#include "ptmi_streams_tree_body.inc"
#undef PTMI_TREE_PACK
#undef PTMI_TREE_PRIM
#undef PTMI_TREE_META
#undef PTMI_HIT_RECORD
#undef PTMI_NORMAL_AT
#undef PTMI_HIT
}

// BVH scenes (ptmi_set_scene_bvh): the same body, the spheres searched through the hierarchy (check_hit_bvh); the packed scene
// (materials, planes) is read through scalar loads, as for every scene too big for LDS.
template <int TILE_W>
__global__ void __launch_bounds__(kRenderBlock, PTMI_BVH_WAVES) render_streams_tree_bvh_kernel(const RenderArgs a, const BvhView bvh)
{
    constexpr bool LDS_SCENE = false;
#define PTMI_HIT(STAGED, S, ns, np, o, d, ...) check_hit_bvh(bvh, S, ns, np, o, d)
#define PTMI_HIT_RECORD hit_record
#define PTMI_NORMAL_AT normal_at
// a BVH scene has up to PTMI_MAX_BVH_SPHERES + PTMI_MAX_BVH_PLANES primitives: 24 bits of primitive, steps at bit 24, draws at bit 25
static_assert(PTMI_MAX_BVH_SPHERES + PTMI_MAX_BVH_PLANES <= (1 << 24), "the tree walk's start record holds 24 bits of primitive");
#define PTMI_TREE_PACK(prim, steps, draws) ((uint32_t)(prim) | ((steps) << 24) | ((draws) << 25))
#define PTMI_TREE_PRIM(w) ((w) & 0xffffffu)
#define PTMI_TREE_META(w) ((((w) >> 24) & 1u) | (((w) >> 25) << 8))
#include "ptmi_streams_tree_body.inc"
#undef PTMI_TREE_PACK
#undef PTMI_TREE_PRIM
#undef PTMI_TREE_META
#undef PTMI_HIT_RECORD
#undef PTMI_NORMAL_AT
#undef PTMI_HIT
}

// mesh scenes (ptmi_set_scene_mesh): the same body, spheres ++ planes ++ triangles searched through the two hierarchies (check_hit_mesh)
template <int TILE_W>
__global__ void __launch_bounds__(kRenderBlock, PTMI_BVH_WAVES) render_streams_tree_mesh_kernel(const RenderArgs a, const MeshView mesh)
{
    constexpr bool LDS_SCENE = false;
#define PTMI_HIT(STAGED, S, ns, np, o, d, ...) check_hit_mesh(mesh, S, ns, np, o, d)
#define PTMI_HIT_RECORD(S, ns, idx, o, d, t, p, n) mesh_hit_record(mesh, S, ns, np, idx, o, d, t, p, n)
#define PTMI_NORMAL_AT(S, ns, idx, p) mesh_normal_at(mesh, S, ns, np, idx, p)
// up to PTMI_MAX_BVH_SPHERES + PTMI_MAX_BVH_PLANES + PTMI_MAX_MESH_TRIANGLES primitives: the BVH kernel's 24 bits of primitive
static_assert(PTMI_MAX_BVH_SPHERES + PTMI_MAX_BVH_PLANES + PTMI_MAX_MESH_TRIANGLES <= (1 << 24), "the tree walk's start record holds 24 bits of primitive");
#define PTMI_TREE_PACK(prim, steps, draws) ((uint32_t)(prim) | ((steps) << 24) | ((draws) << 25))
#define PTMI_TREE_PRIM(w) ((w) & 0xffffffu)
#define PTMI_TREE_META(w) ((((w) >> 24) & 1u) | (((w) >> 25) << 8))
#include "ptmi_streams_tree_body.inc"
#undef PTMI_TREE_PACK
#undef PTMI_TREE_PRIM
#undef PTMI_TREE_META
#undef PTMI_HIT_RECORD
#undef PTMI_NORMAL_AT
#undef PTMI_HIT
}

}  // namespace

// workgroups (per copy of the grid) of the tree walk = records' worth of RenderArgs.tree_stack: x kTreeFastLevels x 64 lanes x 64 B
unsigned int tree_workgroups(int width, int rows_local)
{
    if (tiles_pay_dims(width, rows_local)) return quad_positions(width, rows_local) * 4u;
    return (unsigned int)(((long long)width * rows_local + kRenderBlock - 1) / kRenderBlock);
}

hipError_t launch_render_streams_tree(const RenderArgs &a, const BvhView *bvh, int variant, hipStream_t stream)
{
    if (hipError_t e = clear_stream_iterations(a, stream)) return e;
    if (bvh)
        return launch_per_pixel(a, Mapping::kAuto, render_streams_tree_bvh_kernel<8>, render_streams_tree_bvh_kernel<0>, false, PTMI_BVH_WAVES, 10, stream, *bvh);
    // 4 / 5 keep the row mapping (ablation); 5 and 17, not 6, read the scene through scalar loads; 10 rounds of waves (choose_sample_chunks)
    const Mapping mapping = variant == kVariantRows || variant == kVariantRowsScalar ? Mapping::kRows : Mapping::kAuto;
    if (variant != kVariantRowsScalar && variant != kVariantTilesScalar && scene_fits_lds(a))
        return launch_per_pixel(a, mapping, render_streams_tree_kernel<true, 8>, render_streams_tree_kernel<true>, true, PTMI_TREE_WAVES, 10, stream);
    return launch_per_pixel(a, mapping, render_streams_tree_kernel<false, 8>, render_streams_tree_kernel<false>, false, PTMI_TREE_WAVES, 10, stream);
}

hipError_t launch_render_streams_tree_mesh(const RenderArgs &a, const MeshView &mesh, hipStream_t stream)
{
    if (hipError_t e = clear_stream_iterations(a, stream)) return e;
    return launch_per_pixel(a, Mapping::kAuto, render_streams_tree_mesh_kernel<8>, render_streams_tree_mesh_kernel<0>, false, PTMI_BVH_WAVES, 10, stream, mesh);
}

}  // namespace ptmi
