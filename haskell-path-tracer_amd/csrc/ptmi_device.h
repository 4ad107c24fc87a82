// ptmi_device.h -- what every render kernel of libptmi shares: the device side of checkHit / hit / calcNextRay
// (src/Scene/Trace.hs:344-456, src/Scene/Intersection.hs:16-64, src/Util.hs:114-118, :156-178), the pixel -> wave mapping,
// the sample chunks, the GLASS extension's children.  Included by one translation unit per kernel family:
//   ptmi_inline.hip          render Inline (Trace.hs:193-200)             [+ ptmi_inline_ablations.hip with -DPTMI_ABLATIONS]
//   ptmi_streams_chain.hip   render Streams, one chain per pixel (Trace.hs:141-191)
//   ptmi_streams_tree.hip    render Streams with ray splitting, one tree per pixel
//   ptmi_stream_primary.hip / ptmi_stream_pixels.hip / ptmi_stream_split.hip   the stream ("wavefront") form (ptmi_stream_form.h)
//   ptmi_small.hip           seeds, createWith, present, stitch, dispatch order, point queries
//   ptmi_query.hip           the ray queries on device-resident rays: closest hit, occlusion (ptmi_query_device.h), and with the other kernels along a
//                            caller's rays -- ptmi_query_indexed.hip, ptmi_paths.hip, ptmi_bounce.hip, ptmi_trace_streams.hip -- ptmi_ray_lane_device.h
// Everything here is in an unnamed namespace: each unit gets its own copy, nothing is linked across units (no -fgpu-rdc).
// Diagnostic builds (-DPTMI_*_STATS) live in ptmi_diag.h; the kernels only call its probes, which are empty otherwise.
#pragma once

#include "ptmi_kernels.h"
#include "ptmi_diag.h"

namespace ptmi {

namespace {

constexpr int kBlock = 256;      // small streaming kernels
constexpr size_t kMaxSceneLds = 3 * 1024;  // bytes of staged scene per one-wave workgroup before LDS would cap occupancy (~60 primitives)
constexpr int kRenderBlock = 64; // render kernels: one wave per workgroup, so a finished wave's slot is refilled at once (+1 % on C2)

struct HitSel { float t; int idx; bool just; };
#ifdef PTMI_NO_STAGED_WALK_OTHERS          // (A/B builds: the Streams kernels read the staged scene as S[i], as they did until round 6)
constexpr bool kStagedWalk = false;
#else
constexpr bool kStagedWalk = true;
#endif

// Whole-wave votes of the render loops as scalar work: __any(c) / __all(c) come out as v_cndmask 0, 1 and v_cmp_ne_u32 on top of c's own
// compare -- two four-cycle issue slots for what s_cmp does on the mask that compare already left in an SGPR pair.
__device__ __forceinline__ bool wave_any(bool c)
{
#ifdef PTMI_NO_SCALAR_VOTES
    return __any(c);
#else
    return __builtin_amdgcn_ballot_w64(c) != 0ull;
#endif
}
__device__ __forceinline__ bool wave_all(bool c)
{
#ifdef PTMI_NO_SCALAR_VOTES
    return __all(c);
#else
    return __builtin_amdgcn_ballot_w64(!c) == 0ull;
#endif
}

// Correctly rounded binary32 square root (== IEEE sqrtf, which is what the reference's `sqrt`
// lowers to) without the compiler's always-on denormal scaling: v_sqrt_f32 is within 1 ulp, two
// exact FMA residuals pick the neighbour.  The residual test needs x == 0 or x >= 2^-96; if ANY
// lane of the wave holds a smaller positive x the whole wave takes the compiler's scaled sequence.
__device__ __forceinline__ float sqrt_rn(float x)
{
    const bool tiny = (f2u(x) - 1u) < (0x0f800000u - 1u);          // 0 < x < 2^-96
    if (__builtin_expect(wave_any(tiny), 0)) return __builtin_sqrtf(x);
    const float s = __builtin_amdgcn_sqrtf(x);
    const float s_dn = u2f(f2u(s) - 1u), s_up = u2f(f2u(s) + 1u);
    const float e_dn = __builtin_fmaf(-s_dn, s, x);
    const float e_up = __builtin_fmaf(-s_up, s, x);
    float r = (e_dn <= 0.0f) ? s_dn : s;
    r = (e_up > 0.0f) ? s_up : r;
    return r;
}

// v ^/ s for the three components of a sphere normal: three IEEE divisions by ONE denominator.  The compiler's division is
// div_scale (both operands), rcp, two refinements of the reciprocal, quotient, two residual corrections, div_fmas, div_fixup;
// when neither operand needs scaling and nothing is special -- the denominator within [2^-20, 2^20], the numerators at least
// 2^-100 in magnitude (so every quotient is a normal number, >= 2^-120) and, being components of the vector whose length the
// denominator is, not above it -- div_scale is the
// identity, div_fmas a plain fma and div_fixup passes the quotient through, so the same operations with the reciprocal and its
// refinements formed ONCE give the same three quotients bit for bit (18 instead of 33 instructions, one v_rcp_f32 instead of
// three).  If any lane of the wave falls outside (a zero component, a huge sphere, a NaN) the wave takes the compiler's form.
__device__ __forceinline__ V3 div3_by_length(V3 v, float s)
{
#ifdef PTMI_PLAIN_DIVISION
    return div_r(v, s);
#else
    const float amin = __builtin_fminf(__builtin_fminf(__builtin_fabsf(v.x), __builtin_fabsf(v.y)), __builtin_fabsf(v.z));
    const bool plain = s >= 0x1p-20f && s <= 0x1p20f && amin >= 0x1p-100f;
    if (__builtin_expect(!wave_all(plain), 0)) return div_r(v, s);
    const float r0 = __builtin_amdgcn_rcpf(s);
    const float r = __builtin_fmaf(__builtin_fmaf(-s, r0, 1.0f), r0, r0);
    auto quotient = [&](float a) {
        float q = a * r;
        q = __builtin_fmaf(__builtin_fmaf(-s, q, a), r, q);
        return __builtin_fmaf(__builtin_fmaf(-s, q, a), r, q);
    };
    return mk(quotient(v.x), quotient(v.y), quotient(v.z));
#endif
}

// checkHit (Trace.hs:443-447): mapScene over spheres ++ planes (Util.hs:156-158), then
// expMinWith (Util.hs:171-178): left fold keeping the accumulated element iff keyA <= keyB.
// The reference builds every hit record and selects; selecting the index first and building
// one record afterwards gives the same value.
//
// check_hit_exact is the fold written out literally (every primitive, every lane, no shortcuts).
template <typename ScenePtr>
__device__ __noinline__ HitSel check_hit_exact(ScenePtr S, int ns, int np, V3 o, V3 d)
{
    HitSel best; best.t = 0.0f; best.idx = 0; best.just = false;
    float best_key = 0.0f;
    for (int i = 0; i < ns + np; ++i) {
        bool just; float t;
        if (i < ns) {                                        // distanceTo @Sphere (Intersection.hs:39-48)
            const float4 g = S[i];
            const V3 l = mk(g.x, g.y, g.z) - o;
            const float tca = dot(l, d);
            const float d2 = dot(l, l) - (tca * tca);
            const float thc = __builtin_sqrtf(g.w - d2);
            t = tca - thc;                                   // min t0 t1 == t0
            just = !(tca < 0.0f || d2 > g.w || t < 0.0f);
        } else {                                             // distanceTo @Plane (Intersection.hs:57-62)
            const float4 gp = S[ns + 2 * (i - ns)], gn = S[ns + 2 * (i - ns) + 1];
            const V3 nor = mk(gn.x, gn.y, gn.z);
            const float denom = dot(d, nor);
            t = dot(mk(gp.x, gp.y, gp.z) - o, nor) / denom;
            just = !(denom > 1e-6f || t < 0.0f);
        }
        const float key = just ? t : kInfinite;              // maybe infinite fst
        if (i == 0 || !(best_key <= key)) { best_key = key; best.t = t; best.idx = i; best.just = just; }
    }
    return best;
}

// distanceTo @Sphere (Intersection.hs:39-48) up to the square root, for g = (cx, cy, cz, r*r): declares tca, x and cand.  t = tca -
// sqrt_rn(x) (min t0 t1 == t0), Just iff cand && !(t < 0).  A macro, so that check_hit and check_hit_bvh (ptmi_bvh_device.h) make
// the SAME operations -- a BVH scene's hits are bit for bit the linear fold's -- and check_hit's code stays what it was.
// PTMI_SPHERE_TERMS is the macro up to d2: check_hit's walk forms the candidates from tca and d2 as a wave mask and x = r2 - d2 only where a
// lane is one (fold_sphere); the hierarchies' walks take every lane's square root at a leaf and keep the macro whole.
#define PTMI_SPHERE_TERMS(g, o, d)                                                                                                  \
    const V3 l = mk(g.x, g.y, g.z) - o;                                                                                             \
    const float tca = dot(l, d);                                                                                                    \
    const float d2 = dot(l, l) - (tca * tca)
#define PTMI_SPHERE_TEST(g, o, d)                                                                                                   \
    PTMI_SPHERE_TERMS(g, o, d);                                                                                                     \
    const float x = g.w - d2;                            /* rad ** 2 - d2 (rad ** 2 squared at upload) */                           \
    /* Nothing iff tca < 0 || d2 > rad**2 || t < 0;  d2 > r2 <=> r2 - d2 < 0 (exact: gradual underflow) */                         \
    const bool cand = !(tca < 0.0f) && !(x < 0.0f)

// distanceTo @Plane (Intersection.hs:57-62) folded into the accumulator after the spheres, for check_hit and the hierarchies' walks
// (ptmi_bvh_device.h, ptmi_mesh_device.h): ONE text, so that all of them make the same operations.  at(k) is element k of the scene's
// plane records, (px, py, pz, 0) at 2j and (nx, ny, nz, 0) at 2j + 1.
//   * the cheap part -- denom = dot(d, n), candidate iff !(denom > 1e-6) -- runs for every lane and every plane, as it did, and
//     only STASHES the plane in the lane: its index and its denom, one select each.  Which lanes hold a stash is a wave mask, so
//     the bookkeeping is scalar;
//   * the division runs in dense passes: when a plane comes up for a lane whose stash is taken, and after the last plane, every
//     lane with a stash reads ITS plane's two records by its own address, divides by the denom it kept (the same bits) and folds.
//     Floor and ceiling are candidates of complementary sets of rays: tested plane by plane the division ran twice per trace on
//     half-empty lanes, now once on full ones (the mirror box's six planes: three passes for six).  A pass runs only at a plane that
//     has a candidate, or at the end for what is left, so there are never more passes than planes with a candidate -- what ran before.
//   * the fold is the same fold: a lane's stash is always its earliest candidate not yet folded, so the lane folds its candidates in
//     ascending index after all its spheres, with the same `<=`: ties keep the earlier primitive (a sphere before a plane at the same
//     t, the first of two coincident planes).  A lane without a stash takes part in a pass with a denom of 1 -- no candidate, a
//     Nothing, which replaces an accumulator that is still NaN and no other (+inf: see check_hit) -- as lanes that were no candidates
//     of a tested plane always did.  A plane a lane is no candidate of is otherwise a Nothing that the lane skips, like every skipped
//     element (see check_hit): it differs from the literal fold only where the final accumulator is a Just whose key is not < FLT_MAX
//     -- which the callers detect and redo literally -- or where the accumulator is never filled (no sphere on the square-root path,
//     no pass): just == false then, as in the literal fold, and every caller reads t and idx of a Just only.
// The per-plane operations of that fold, for it and for the any-hit walks (ptmi_query_device.h); macros for PTMI_SPHERE_TEST's reason.
// PTMI_PLANE_DENOM: the denominator of a plane's normal row; PTMI_PLANE_DISTANCE: for the plane (gp, gn) and the denominator the lane
// kept, declares t and just.
#define PTMI_PLANE_DENOM(gn, d) dot(d, mk(gn.x, gn.y, gn.z))
#define PTMI_PLANE_DISTANCE(gp, gn, o, denom)                                                                                       \
    const float t = dot(mk(gp.x, gp.y, gp.z) - o, mk(gn.x, gn.y, gn.z)) / denom;                                                    \
    const bool just = !(denom > 1e-6f) && !(t < 0.0f)

template <typename At>
__device__ __forceinline__ void fold_planes(At at, int ns, int np, V3 o, V3 d, float &best_key, int &best_idx, bool &best_just,
                                            unsigned int *diag = nullptr)
{
    int stash = 0;
    float stash_denom = 1.0f;
    unsigned long long stashed = 0ull;                       // the lanes that hold a stash
    auto pass = [&]() {
        diag::plane_pass(diag);
        const float4 gp = at(2 * stash), gn = at(2 * stash + 1);
        PTMI_PLANE_DISTANCE(gp, gn, o, stash_denom);         // t, just
        const float key = just ? t : kInfinite;
        if (!(best_key <= key)) { best_key = key; best_idx = ns + stash; best_just = just; }
        stash_denom = 1.0f;
        stashed = 0ull;
    };
    for (int j = 0; j < np; ++j) {
        const float4 gn = at(2 * j + 1);
        const float denom = PTMI_PLANE_DENOM(gn, d);
        const bool cand = !(denom > 1e-6f);
        const unsigned long long cands = __ballot(cand);
        diag::plane_test(diag);
        if (cands & stashed) pass();
        stash = cand ? j : stash;
        stash_denom = cand ? denom : stash_denom;
        stashed |= cands;
    }
    if (stashed) pass();
}

// How check_hit takes the square roots of a trace's sphere candidates (its FOLD parameter; measured per kernel family,
// profiles/sphere_pass_ab.txt and experiments/sphere_pass/):
//   kStash        dense passes, a candidate lane stashing (tca, x, index) in a masked block -- s_and_saveexec, three v_mov, s_or exec.  The
//                 default: the Streams chain, the tree walk, the stream form's per-pixel kernels, the point queries;
//   kStashSelect  dense passes, the stash as three selects (and the index's move).  render Inline: there the selects are the faster
//                 stash (C2 2.63-2.65 ms against 2.64-2.66), in the tree walk they give the passes' gain away;
//   kPerSphere    no stash: square root, t and the fold update at every sphere that has a candidate lane, for the whole wave, as every
//                 kernel did before.  The stream form's split kernels (GLASS): their compacted waves hold a candidate in so many
//                 lanes that nearly every such sphere meets a taken stash, and the stash only adds its moves (+0.4 % measured).
enum class SphereFold { kStash, kStashSelect, kPerSphere };

// Whether check_hit's walk carries the x-y terms of the sphere test from one sphere to the next (its SHARE parameter; chosen per kernel
// family like FOLD, profiles/shared_xy_ab.txt and experiments/shared_xy/):
//   kNone  every sphere runs PTMI_SPHERE_TEST whole.  The default;
//   kXY    a sphere whose bit is set in `share` (SceneView.share_xy: its cx and cy have its predecessor's bits, ptmi_share.h) keeps the
//          predecessor's sxy = lx dx + ly dy and qxy = lx lx + ly ly and forms tca = sxy + lz dz, d2 = (qxy + lz lz) - tca tca: 10 VALU
//          instructions for 18.  render Inline on linear scenes (S16: 6 of 14 spheres) and the point queries, for a scene whose mask is not 0.
//          In a scene without runs the walk would pay a scalar bit test and an untaken branch a sphere for nothing (C0's scene +0.6 %), and a
//          second, untested walk behind a branch on mask == 0 costs render Inline a spill more than its budget allows (experiments/shared_xy/):
//          the LAUNCHERS send a mask of 0 to a kNone kernel (render_inline_kernel_plain, ptmi_inline.hip; ptmi_small.hip).
enum class SphereShare { kNone, kXY };

// A/B builds (tools/ab.py, profiles/four_cycle_ab.txt): -DPTMI_NO_SPHERE_TWO_COMPARES forms check_hit's candidates as it did (x for every
// lane, one compare of min(tca, x)), -DPTMI_NO_SCALAR_VOTES leaves the whole-wave votes to __any / __all,
// -DPTMI_NO_SINCOS_TINY sends a wave that holds an angle below 2^-12 to sincos() (ptmi_core.h).
#ifdef PTMI_NO_SPHERE_TWO_COMPARES
constexpr bool kSphereTwoCompares = false;
#else
constexpr bool kSphereTwoCompares = true;
#endif

// check_hit is the same fold shaped for the SIMD:
//   * the cheap part of every test (16 f32 operations for a sphere) runs for all lanes; the square
//     root / division and the fold update run only when some lane of the wave can still be hit
//     (wave-uniform branch on a ballot) -- the common case to skip once rays are incoherent;
//   * best_key starts as NaN so that the first evaluated element always replaces the accumulator
//     (`NaN <= key` is false), which is expMinWith seeding the fold with its head;
//   * a skipped element is a Nothing (key FLT_MAX).  In the literal fold a Nothing replaces the
//     accumulator only when the accumulated key is NaN or +inf; leaving the accumulator alone instead
//     can change the outcome only if the FINAL accumulator is a Just whose key is not < FLT_MAX, so that
//     one case (a ray or primitive with non-finite numbers) is detected at the end and redone literally.
//   * spheres are walked two per trip with the two register sets swapping roles, so the prefetch of
//     the next primitive costs no moves.
//   * STAGED = true (the caller has staged the scene in LDS and S points there): the geometry is read off ONE vector register
//     that holds its LDS address, four spheres per trip, the offsets as immediates.  The address of a wave-uniform LDS read is a
//     scalar, but ds_read wants it in a VGPR: read as S[i] every ds_read_b128 had a `v_mov_b32 vN, sK` in front of it -- one
//     VALU issue slot in 22 of the sphere test, 56 M of them per C2 launch (round 6, tools/isa_other.py: C2 2.93 -> 2.86 ms).
//   * the sphere candidates' square roots run in DENSE PASSES (FOLD != kPerSphere), as fold_planes takes the planes' divisions.  On
//     C2 a sphere with a candidate has it in 6 of the wave's 55 active lanes, 2.67 such spheres a trace: the whole wave paid for the
//     correctly rounded root each time.  Now a candidate lane only STASHES (tca, x, i); which lanes hold a stash is a wave mask, so
//     the bookkeeping is scalar.  A pass takes the square root, t, Just and key of every stashed lane's OWN sphere and folds it; it
//     runs when a sphere comes up for a lane whose stash is taken, before that lane overwrites it, and once behind the last sphere
//     (before the planes): never more passes than spheres with a candidate, which is what ran the square root before (C2: 1.42 a trace).
//       - the same fold: a lane's stash is always its earliest candidate not yet folded, so the lane folds exactly its own candidates
//         in ascending index with the same `<=` -- ties keep the earlier sphere -- and before any plane.
//       - lanes without a stash sit OUT of a pass.  When the square root ran per sphere such a lane went through the update as a
//         Nothing (key FLT_MAX), which replaces an accumulator that is still NaN (or +inf) and no other: all it could do was turn an
//         unfilled accumulator into a Nothing.  Sitting out leaves best_just false and best_key NaN there instead.  Every later
//         element replaces a NaN accumulator (`NaN <= key` is false); it replaced that Nothing too unless its own key is not <
//         FLT_MAX -- another Nothing, which changes nothing a caller reads, or a Just that the final test below sends to the literal
//         fold either way.  And no caller reads t or idx unless just.
//       - sqrt_rn's whole-wave vote (__any(tiny)) sees the pass's lanes only, and in them only candidates' x: a wave takes the
//         compiler's scaled sequence for fewer x than before, never for fewer than need it, and both sequences are the IEEE root.
//   * SHARE = kXY: dot is (a.x b.x + a.y b.y) + a.z b.z (ptmi_core.h), so lx, ly, sxy = lx dx + ly dy and qxy = lx lx + ly ly are whole
//     subexpressions of the test's literal arithmetic, and functions of (cx, cy) and the ray alone.  A sphere with its predecessor's cx
//     and cy BITS would compute the same four values from the same operands: it takes them as they stand (a wave-uniform branch on the
//     scene's mask, shifted along with the walk) and makes the rest of the test -- lz, tca, d2, then fold_sphere's x and candidates -- by the macro's operations in
//     the macro's order.  Shared or not, the same operations meet the same operands: the hits stay bit for bit PTMI_SPHERE_TEST's, which
//     the hierarchies' walks (and kNone) keep running whole, so a BVH scene's hits stay the linear fold's.  Nothing is reordered (ties
//     keep the earlier index), and the stash, the passes, the planes and the final test below see tca, x and cand as before.
template <bool STAGED = false, SphereFold FOLD = SphereFold::kStash, SphereShare SHARE = SphereShare::kNone, typename ScenePtr>
__device__ __forceinline__ HitSel check_hit(ScenePtr S, int ns, int np, V3 o, V3 d, unsigned int *diag = nullptr, unsigned long long share = 0ull)
{
    float best_key = __builtin_nanf("");
    int best_idx = 0;
    bool best_just = false;

    float stash_tca = 0.0f, stash_x = 0.0f;
    int stash_idx = 0;
    unsigned long long stashed = 0ull;                       // the lanes that hold a stash
    auto pass = [&]() {
        diag::sphere_pass(diag);
        if (__builtin_amdgcn_inverse_ballot_w64(stashed)) {  // (the mask becomes the exec mask: no lane computes its own bit)
            const float t = stash_tca - sqrt_rn(stash_x);    // min t0 t1 == t0 (thc >= 0 or NaN)
            const bool just = !(t < 0.0f);                   // (a lane with a stash is a candidate)
            const float key = just ? t : kInfinite;          // maybe infinite fst
            // (as a masked block -- s_and_saveexec, two v_mov, s_or exec -- not as three selects: the selects cost C2 + 1.6 %, round 6)
            if (!(best_key <= key)) { best_key = key; best_idx = stash_idx; best_just = just; }
        }
        stashed = 0ull;
    };
    // (kXY) lx dx + ly dy and lx lx + ly ly of the last sphere that computed them.  Not initialised: bit 0 of the mask is never set, so the
    // first sphere writes them before any reads them, and two moves a trace are 0.5 % of a small scene's instructions
    float sxy, qxy;
    // (kTwoCompares) the candidates of a sphere as a WAVE MASK from two compares, tca < 0 and d2 > r2, joined by one scalar and: x = r2 - d2
    // is then needed only where a lane is a candidate (a fifth of the tests on C2) and is formed there, by the same subtraction.  d2 > r2 is
    // the predicate x < 0 (see PTMI_SPHERE_TEST; r2 = inf with d2 = inf and every NaN answer false to both), so tca, x and the candidates
    // are the macro's bit for bit, and the stash's selects and `stashed` take the scalar mask as it stands.
    auto fold_sphere = [&](int i, float tca, float d2, float r2) {
        float x = 0.0f;
        bool cand;
        unsigned long long cands;
        if constexpr (kSphereTwoCompares) {
            cands = __builtin_amdgcn_ballot_w64(!(tca < 0.0f)) & __builtin_amdgcn_ballot_w64(!(d2 > r2));
            cand = __builtin_amdgcn_inverse_ballot_w64(cands);
        } else {
            x = r2 - d2;
            cand = !(tca < 0.0f) && !(x < 0.0f);
            cands = __ballot(cand);
        }
        diag::sphere_test(diag, cand);
        if constexpr (FOLD == SphereFold::kPerSphere) {
            if (cands) {
                if constexpr (kSphereTwoCompares) x = r2 - d2;
                const float t = tca - sqrt_rn(x);            // min t0 t1 == t0 (thc >= 0 or NaN)
                const bool just = cand && !(t < 0.0f);
                const float key = just ? t : kInfinite;      // maybe infinite fst
                if (!(best_key <= key)) { best_key = key; best_idx = i; best_just = just; }
            }
        } else if (cands) {
            if (cands & stashed) pass();
            if constexpr (kSphereTwoCompares) x = r2 - d2;
            if constexpr (FOLD == SphereFold::kStashSelect) {
                stash_tca = cand ? tca : stash_tca;
                stash_x = cand ? x : stash_x;
                stash_idx = cand ? i : stash_idx;
            } else {
                if (cand) { stash_tca = tca; stash_x = x; stash_idx = i; asm volatile(""); }    // (the empty statement keeps the block from becoming selects)
            }
            stashed |= cands;
        }
    };
    // `bit`: which bit of `share` is this sphere's (the walks below shift the mask by a trip's spheres, so it is an immediate)
    auto sphere = [&](const float4 g, int i, int bit = 0) {
        if constexpr (SHARE == SphereShare::kXY) {
            const float lz = g.z - o.z;
            if (!((unsigned int)share & (1u << bit))) {      // wave-uniform: the mask is the scene's
                const float lx = g.x - o.x, ly = g.y - o.y;
                sxy = lx * d.x + ly * d.y;
                qxy = lx * lx + ly * ly;
            } else diag::sphere_shared(diag);
            // PTMI_SPHERE_TEST from here on, operation for operation
            const float tca = sxy + lz * d.z;
            const float d2 = (qxy + lz * lz) - (tca * tca);
            fold_sphere(i, tca, d2, g.w);                    // x, cand
        } else {
            (void)bit;
            PTMI_SPHERE_TERMS(g, o, d);                      // tca, d2
            fold_sphere(i, tca, d2, g.w);                    // x, cand
        }
    };

    float4 ga, gb;
    int i = 0;
#if defined(__HIP_DEVICE_COMPILE__)
    typedef __attribute__((address_space(3))) const float4 *Staged;
    Staged P = nullptr;
    if constexpr (STAGED) {
        unsigned int lds_at = (unsigned int)(uintptr_t)&S[0];    // the low half of a generic LDS address is the LDS offset
        asm volatile("" : "+v"(lds_at));                          // ... kept in a VGPR: the loads below take it with immediate offsets
        P = (Staged)(uintptr_t)lds_at;
        ga = P[0];
        for (; i + 3 < ns; i += 4) {
            gb = P[1]; sphere(ga, i, 0);
            ga = P[2]; sphere(gb, i + 1, 1);
            gb = P[3]; sphere(ga, i + 2, 2);
            ga = P[4]; sphere(gb, i + 3, 3);                      // S has readable elements past the geometry
            P += 4;
            share >>= 4;                                          // (nothing is left of it from sphere 64 on)
        }
        for (; i + 1 < ns; i += 2) {
            gb = P[1]; sphere(ga, i, 0);
            ga = P[2]; sphere(gb, i + 1, 1);
            P += 2;
            share >>= 2;
        }
        if (i < ns) {
            sphere(ga, i, 0);
            P += 1;
        }
    } else
#endif
    {
        ga = S[0];
        for (; i + 1 < ns; i += 2) {
            gb = S[i + 1];
            sphere(ga, i, 0);
            ga = S[i + 2];                                       // S has readable elements past the geometry
            sphere(gb, i + 1, 1);
            share >>= 2;
        }
        if (i < ns) sphere(ga, i, 0);
    }
    if (FOLD != SphereFold::kPerSphere && stashed) pass();
    fold_planes([&](int k) -> float4 {
#if defined(__HIP_DEVICE_COMPILE__)
        if constexpr (STAGED) return P[k]; else
#endif
        return S[ns + k];
    }, ns, np, o, d, best_key, best_idx, best_just, diag);
    // (the vote on ONE compare, of the key a Just holds and 0 otherwise: the ballot of a two-term condition goes back through a VGPR)
#ifdef PTMI_NO_SCALAR_VOTES
    if (__builtin_expect(__any(best_just && !(best_key < kInfinite)), 0))
#else
    float just_key = best_just ? best_key : 0.0f;
#if defined(__HIP_DEVICE_COMPILE__)
    asm volatile("" : "+v"(just_key));                       // (... and the compiler folds the select back into that condition)
#endif
    if (__builtin_expect(__builtin_amdgcn_ballot_w64(!(just_key < kInfinite)) != 0ull, 0))
#endif
        return check_hit_exact(S, ns, np, o, d);
    HitSel best; best.t = best_key; best.idx = best_idx; best.just = best_just;
    return best;
}

// hit (Intersection.hs:29-32) + normal (:50 / :64) for the selected primitive
template <typename ScenePtr>
__device__ __forceinline__ void hit_record(ScenePtr S, int ns, int idx, V3 o, V3 d, float t,
                                           V3 &hit_pos, V3 &normal)
{
    hit_pos = o + scale_r(d, t);
    if (idx < ns) {
        const float4 g = S[idx];
        // normalize (linear): v unchanged if |v|^2 is within 1e-6 of 0 or 1, else v / sqrt |v|^2
        const V3 v = hit_pos - mk(g.x, g.y, g.z);
        const float len2 = dot(v, v);
        normal = (near_zero(len2) || near_zero(1.0f - len2)) ? v : div3_by_length(v, sqrt_rn(len2));
    } else {
        const float4 gn = S[ns + 2 * (idx - ns) + 1];
        normal = mk(gn.x, gn.y, gn.z);
    }
}

// normal (Intersection.hs:50 / :64) of primitive idx at a hit position computed earlier: the second half of hit_record
template <typename ScenePtr>
__device__ __forceinline__ V3 normal_at(ScenePtr S, int ns, int idx, V3 hit_pos)
{
    if (idx < ns) {
        const float4 g = S[idx];
        const V3 v = hit_pos - mk(g.x, g.y, g.z);
        const float len2 = dot(v, v);
        return (near_zero(len2) || near_zero(1.0f - len2)) ? v : div3_by_length(v, sqrt_rn(len2));
    }
    const float4 gn = S[ns + 2 * (idx - ns) + 1];
    return mk(gn.x, gn.y, gn.z);
}

// genVec (Util.hs:114-118) for the device: component = (random * 2.0) - 1.0 with
// random = (float(int32 w) * 2^-32 + 0.5) + 2^-33.  Doubling is exact and commutes with rounding
// here (no value leaves the normal range), so the doubled form below is the same binary32 value
// with one multiplication less: ((I * 2^-31 + 1.0) + 2^-32) - 1.0.
__device__ __forceinline__ float gen_component(Sfc32 &seed)
{
    const float i = (float)(int32_t)sfc32_next(seed);
    return ((i * 4.656612873077392578125e-10f + 1.0f) + 2.3283064365386962890625e-10f) - 1.0f;
}

// calcNextRay's direction part (Trace.hs:394-429): the three draws, the rotated direction `next` and the BRDF
// factor `b`.  Both BRDF arms are evaluated through selects so that Matte and Glossy lanes of one wave do not
// serialise.  M points at the material records.
//   Matte:  rotate (anglesToQuaternion $ pi *^ rv) iNormal
//   Glossy: rotate (anglesToQuaternion $ (1 - p) *^ rv) reflection
// anglesToQuaternion halves every angle; (k * rv) * 0.5 == (0.5 k) * rv bit for bit (power-of-two scaling).
__device__ __forceinline__ void bounce_axis(float4 mb, V3 normal, V3 d, V3 &axis, float &hk)
{
    const bool matte = f2u(mb.x) == 0u;
    const float ia = dot(d, normal);
    const V3 reflection = d - scale_l(2.0f * ia, normal);
    axis = matte ? normal : reflection;
    hk = matte ? 0.5f * kPi : mb.w;       // mb.w = 0.5 * (1 - p)  (Trace.hs:424 and Util.hs:62-67), exact halving
}

__device__ __forceinline__ void next_about_axis(float4 mb, V3 axis, float hk, Sfc32 &seed, V3 &next, float &brdf)
{
    const bool matte = f2u(mb.x) == 0u;
    V3 rv;
    rv.x = gen_component(seed); rv.y = gen_component(seed); rv.z = gen_component(seed);
    next = rotate(quaternion_from_half_angles(hk * rv.x, hk * rv.y, hk * rv.z), axis);
    const float nd = dot(next, axis);
    brdf = matte ? mb.z * nd : __builtin_fmaxf(0.0f, nd);      // mb.z = p / pi (Trace.hs:411), divided at upload
}

// -DPTMI_SINCOS_STATS (diagnostic build, tools/sincos_stats.py): called before next_about_axis with a COPY of the seed, it makes the three
// draws again and votes as quaternion_from_half_angles will: [30] shade rounds of a wave, [31] those that leave the three-angle fast form
// (an angle beyond +-T2, inf or NaN in any lane that shades; with -DPTMI_NO_SINCOS_TINY also one below 2^-12 in magnitude), [29] those that
// stay in it and run the fix-up for angles below 2^-12.  Empty and static otherwise, like diag's probes.
#ifdef PTMI_SINCOS_STATS
__device__ __forceinline__ void sincos3_probe(unsigned int *wc, float hk, Sfc32 seed)
{
#if defined(__HIP_DEVICE_COMPILE__)                                  // (the vote exists in the device pass only)
    const float x = gen_component(seed), y = gen_component(seed), z = gen_component(seed);
#ifdef PTMI_NO_SINCOS_TINY
    const bool fast = sincos3_wave_is_fast(hk * x, hk * y, hk * z), tiny = false;
#else
    bool tiny;
    const bool fast = sincos3_wave_in_range(hk * x, hk * y, hk * z, tiny);
#endif
    if (wc && (threadIdx.x & 63) == (int)__builtin_ctzll(__ballot(1))) { atomicAdd(wc + 30, 1u); if (!fast) atomicAdd(wc + 31, 1u); else if (tiny) atomicAdd(wc + 29, 1u); }
#endif
}
#else
__device__ __forceinline__ static void sincos3_probe(unsigned int *, float, const Sfc32 &) {}
#endif

template <typename ScenePtr>
__device__ __forceinline__ void next_direction(ScenePtr M, int idx, V3 normal, V3 d, Sfc32 &seed, V3 &next, float &brdf)
{
    const float4 mb = M[2 * idx + 1];
    V3 axis; float hk;
    bounce_axis(mb, normal, d, axis, hk);
    next_about_axis(mb, axis, hk, seed, next, brdf);
}

// The rest of calcNextRay (Trace.hs:431-435) and computeRay (Trace.hs:374-383) once `next` and `b` are known.
template <typename ScenePtr>
__device__ __forceinline__ void apply_bounce(ScenePtr M, int idx, V3 hit_pos, V3 next, float brdf,
                                             V3 &o, V3 &d, V3 &throughput, V3 &result)
{
    const float4 ma = M[2 * idx];
    const V3 color = mk(ma.x, ma.y, ma.z);
    const float illuminance = ma.w;
    const V3 emittance = scale_r(color, illuminance);
    constexpr float next_ray_prob = 1.0f / (kPi * 2.0f);
    o = hit_pos + scale_r(next, kEpsilon);
    d = next;
    const V3 tmod = scale_r(color, brdf * next_ray_prob);
    result = result + (emittance * throughput);
    throughput = throughput * tmod;
}

// computeRay (Trace.hs:374-383) + calcNextRay (Trace.hs:394-435)
template <typename ScenePtr>
__device__ __forceinline__ void shade(ScenePtr M, int idx, V3 hit_pos, V3 normal,
                                      V3 &o, V3 &d, V3 &throughput, V3 &result, Sfc32 &seed)
{
    V3 next; float brdf;
    next_direction(M, idx, normal, d, seed, next, brdf);
    apply_bounce(M, idx, hit_pos, next, brdf, o, d, throughput, result);
}

// The first shade of a sample that starts from the pixel's cached primary hit: result = 0, throughput = 1 and the
// incoming ray is the primary ray, so the rotation axis, the half angle scale and 0 + emittance * 1 are per-pixel
// constants (evaluated once, by the same operations), and throughput * tmod = 1 * tmod = tmod.
// ACCUMULATE (render Streams): `result` is the pixel's accumulator and first_term = emittance * 1 is added to it;
// otherwise (render Inline) first_term = 0 + emittance * 1 is the sample's result so far.
template <bool ACCUMULATE, typename ScenePtr>
__device__ __forceinline__ void shade_first(ScenePtr M, int idx, V3 hit_pos, V3 axis, float hk, V3 first_term,
                                            V3 &o, V3 &d, V3 &throughput, V3 &result, Sfc32 &seed)
{
    const float4 ma = M[2 * idx], mb = M[2 * idx + 1];
    V3 next; float brdf;
    next_about_axis(mb, axis, hk, seed, next, brdf);
    constexpr float next_ray_prob = 1.0f / (kPi * 2.0f);
    o = hit_pos + scale_r(next, kEpsilon);
    d = next;
    result = ACCUMULATE ? result + first_term : first_term;
    throughput = scale_r(mk(ma.x, ma.y, ma.z), brdf * next_ray_prob);
}

// Is the shade that is about to happen CERTAIN to leave a throughput that the next prepareRay freezes (nearZero,
// Trace.hs:364-365) -- whatever the three random draws turn out to be?  If so its `next` ray and throughput are never
// looked at again: the only things the reference keeps from that iteration are result += emittance * throughput and
// the seed after genVec's three draws (Trace.hs:374-383), and the expensive half of the shade (three sin/cos pairs,
// the quaternion, the rotation) can be skipped without changing any output bit.
// Bound: next = rotate q axis with |q| = 1 up to rounding, so |next . axis| <= |axis|^2 (1 + 2e-5) <= a2 below; hence
// |brdf| <= bmax (Matte: |p/pi| a2, Glossy: max(0, nd) <= a2) by monotonicity of rounding, |tmod_c| <= |color_c| (bmax prob)
// and |throughput'_c| <= |throughput_c| (|color_c| g), formed in the SAME association as the real product so that it
// overflows exactly when the real one can; 1 % of slack covers the four roundings of the real dot product.  Every
// comparison is written so that a NaN or an infinity anywhere answers "not certain".
__device__ __forceinline__ bool surely_frozen_after(float4 ma, float4 mb, V3 axis, V3 throughput)
{
    const bool matte = f2u(mb.x) == 0u;
    const float a2 = dot(axis, axis) * 1.001f + 1e-30f;             // >= |next . axis|, also when the products are denormal
    const float bmax = matte ? __builtin_fabsf(mb.z) * a2 : a2;
    const float g = bmax * (1.0f / (kPi * 2.0f));
    const V3 v = throughput * scale_r(mk(ma.x, ma.y, ma.z), g);
    return dot(v, v) * 1.01f <= 1e-6f;
}

// What the reference keeps of an iteration whose throughput is frozen right afterwards: the contribution and the seed.
__device__ __forceinline__ void finish_frozen(float4 ma, V3 throughput, V3 &result, Sfc32 &seed)
{
    result = result + (scale_r(mk(ma.x, ma.y, ma.z), ma.w) * throughput);
    (void)sfc32_next(seed); (void)sfc32_next(seed); (void)sfc32_next(seed);     // genVec's three draws
}

__device__ __forceinline__ int global_row(int local_row, int stripe_rows, int n_parts, int part)
{
    return ((local_row / stripe_rows) * n_parts + part) * stripe_rows + local_row % stripe_rows;
}

// How many lanes below this one are set in `mask`: v_mbcnt_lo/hi, no per-lane 64-bit mask to keep in registers.
__device__ __forceinline__ unsigned int rank_in(unsigned long long mask)
{
    return __builtin_amdgcn_mbcnt_hi((unsigned int)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned int)mask, 0u));
}
__device__ __forceinline__ unsigned long long wave_sum(unsigned int v)
{
    unsigned long long s = v;
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
    return s;
}

// Which pixel a lane of a one-wave workgroup works on.  TILE_W == 0: 64 consecutive pixels of a row (plane order).
// TILE_W > 0: a TILE_W x (64 / TILE_W) tile of the image -- the 64 primary rays of a wave meet the same few
// primitives and their paths have similar lengths, which is worth 1-2 % (8 x 8 measured best); the
// seven plane accesses of a lane happen once per launch, so their shorter runs do not matter.
template <int TILE_W>
__device__ __forceinline__ bool lane_pixel(const RenderArgs &a, long long &pixel, unsigned int &quad, unsigned int wg = blockIdx.x)
{
    quad = 0;
    if (TILE_W > 0) {
        constexpr int tw = TILE_W > 0 ? TILE_W : 64, th = 64 / tw;
        const int tiles_x = (a.width + tw - 1) / tw;
        // Workgroups are dealt round-robin to the 8 XCDs, each with its own L2.  A tile row segment is only tw * 4
        // bytes of a 128-byte line, so x-adjacent tiles must meet in ONE L2 or the line is fetched from HBM once per
        // tile (measured: 232 MB instead of 58 MB per launch): runs of 4 consecutive tiles ("quads") go to the same
        // XCD, as consecutive workgroups of that XCD.  The grid is padded to a multiple of 32 so that this is a bijection.
        // Which quad a dispatch position gets is the image order, or -- once a launch with the same camera has recorded
        // what every quad costs -- the most expensive first (quad_order), which shortens the end of the kernel where
        // the last waves run with the chip half empty.
        const unsigned int xcd = wg & 7u, k = wg >> 3;
        const unsigned int position = (k >> 2) * 8u + xcd;
        quad = a.quad_order ? a.quad_order[position] : position;
        const unsigned int tile = (quad << 2) + (k & 3u);
        const int tx = (int)(tile % (unsigned)tiles_x), ty = (int)(tile / (unsigned)tiles_x);
        const int x = tx * tw + (int)(threadIdx.x % tw), y = ty * th + (int)(threadIdx.x / tw);
        pixel = (long long)y * a.width + x;
        return x < a.width && y < a.rows_local;              // also false for the padding tiles (ty beyond the image)
    }
    pixel = (long long)wg * kRenderBlock + threadIdx.x;
    return pixel < (long long)a.rows_local * a.width;
}

// what the wave paid: the loop trips of its slowest lane, added to its quad's cost
__device__ __forceinline__ void record_cost(const RenderArgs &a, unsigned int quad, unsigned int trips)
{
    if (!a.quad_cost) return;
    for (int off = 32; off > 0; off >>= 1) { const unsigned int other = __shfl_xor(trips, off, 64); trips = other > trips ? other : trips; }
    if ((threadIdx.x & 63) == 0) atomicAdd(a.quad_cost + quad, trips + 1u);
}

__host__ inline unsigned int tile_grid(const RenderArgs &a, int tw)
{
    const int th = 64 / tw;
    const unsigned int tiles = (unsigned int)(((a.width + tw - 1) / tw) * ((a.rows_local + th - 1) / th));
    return (tiles + 31u) & ~31u;                             // see lane_pixel
}

// Sample chunks (see the comment in render_inline_kernel): which copy of the tile grid this workgroup is, which slice of
// the samples it renders, and the wait for the previous copy of the same tile.
template <int TILE_W>
__device__ __forceinline__ void enter_sample_chunk(const RenderArgs &a, unsigned int &wg, int &chunk, int &n_spp_chunk)
{
    wg = blockIdx.x + (a.first_position ? 4u * *a.first_position : 0u);     // (the tail of the stream form: RenderArgs.first_position)
    chunk = 0; n_spp_chunk = a.n_spp;
    if (TILE_W > 0 && a.spp_chunks > 1) {
        // The workgroup's place in the chain of copies is a TICKET, not blockIdx: HIP promises nothing about the order in which
        // workgroups are dispatched, and a consumer that waited for a producer not yet dispatched -- with every slot held by
        // waiting consumers -- would hang the launch.  The producer of a ticket's tile holds the ticket per_copy lower: it was
        // taken by a workgroup that is running or has finished.
        unsigned int t = 0;
        if ((threadIdx.x & 63) == 0) t = atomicAdd(a.chunk_done + a.chunk_capacity, 1u);
        wg = (unsigned int)__builtin_amdgcn_readfirstlane((int)t);
        const unsigned int per_copy = gridDim.x / (unsigned int)a.spp_chunks;
        chunk = (int)(wg / per_copy);
        wg -= (unsigned int)chunk * per_copy;
        const int per = (a.n_spp + a.spp_chunks - 1) / a.spp_chunks;
        n_spp_chunk = a.n_spp - chunk * per;
        n_spp_chunk = n_spp_chunk < 0 ? 0 : (n_spp_chunk > per ? per : n_spp_chunk);
        if (chunk > 0) {
            // one relaxed poll, then ONE acquire (polling with acquire loads invalidates the L1 every time round)
            while (__hip_atomic_load(a.chunk_done + wg, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < (unsigned int)chunk)
                __builtin_amdgcn_s_sleep(16);
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        }
    }
}

template <int TILE_W>
__device__ __forceinline__ void leave_sample_chunk(const RenderArgs &a, unsigned int wg, int chunk)
{
    if (TILE_W > 0 && a.spp_chunks > 1 && chunk + 1 < a.spp_chunks) {     // publish: the next copy of this tile may start
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                   // the write-back has completed before the flag leaves (the compiler may drop its own wait)
        if ((threadIdx.x & 63) == 0) __hip_atomic_store(a.chunk_done + wg, (unsigned int)(chunk + 1), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// The two constants of a GLASS material that glass_children needs: eta = 1 / ior and Schlick's r0 = ((1 - ior) / (1 + ior))^2 -- two
// divisions per glass hit.  A kernel that keeps the scene in LDS computes them once per workgroup, with the same operations, into the
// two words of the material record that GLASS leaves unused (mb.z, mb.w of the LDS copy); one that reads the scene through scalar
// loads computes them at the hit.
struct GlassConstants { float eta, r0; };
__device__ __forceinline__ GlassConstants glass_constants(float ior)
{
    GlassConstants g;
    g.eta = 1.0f / ior;
    const float q = (1.0f - ior) / (1.0f + ior);
    g.r0 = q * q;
    return g;
}
__device__ __forceinline__ void stage_glass_constants(float4 *lds, const SceneView &scene)
{
    float4 *M = lds + scene.geom_f4();
    const int n = scene.n_spheres + scene.n_planes;
    for (int i = threadIdx.x; i < n; i += kRenderBlock) {
        float4 mb = M[2 * i + 1];
        if (f2u(mb.x) == 2u) { const GlassConstants g = glass_constants(mb.y); mb.z = g.eta; mb.w = g.r0; M[2 * i + 1] = mb; }
    }
}
template <bool LDS_SCENE>
__device__ __forceinline__ GlassConstants glass_constants_of(float4 mb)
{
    if (LDS_SCENE) { GlassConstants g; g.eta = mb.z; g.r0 = mb.w; return g; }
    return glass_constants(mb.y);
}

// GLASS ior (extension): reflection child + refraction child; see the oracle's glass_children for the spec.
__device__ __forceinline__ void glass_children(V3 color, GlassConstants gc, V3 p, V3 n, V3 d, V3 throughput, Sfc32 seed,
                                               V3 o_out[2], V3 d_out[2], V3 t_out[2], Sfc32 s_out[2])
{
    (void)gen_component(seed); (void)gen_component(seed); (void)gen_component(seed);   // genVec is drawn before the match
    const float dn = dot(d, n);
    const float cosi = -dn;
    const float eta = gc.eta;
    const float k = 1.0f - (eta * eta) * (1.0f - cosi * cosi);
    const V3 reflection = d - scale_l(2.0f * dn, n);
    const float r0 = gc.r0;
    const float mm = 1.0f - cosi;
    float R = r0 + (1.0f - r0) * (((mm * mm) * (mm * mm)) * mm);
    V3 refraction;
    if (k < 0.0f) { R = 1.0f; refraction = reflection; }
    else refraction = scale_l(eta, d) + scale_l(eta * cosi - __builtin_sqrtf(k), n);
    o_out[0] = p + scale_r(reflection, kEpsilon); d_out[0] = reflection;
    t_out[0] = throughput * scale_r(color, R);
    s_out[0] = seed;
    o_out[1] = p + scale_r(refraction, kEpsilon); d_out[1] = refraction;
    t_out[1] = throughput * scale_r(color, 1.0f - R);
    (void)random_float(seed);
    s_out[1] = seed;
}

// The REFRACTION child of a GLASS hit alone, for kernels that let the reflection child travel through the ordinary shade (the
// stream form's split kernel): with ia = dot(d, n) and reflection = d - (2 ia) n in hand -- what the ordinary shade's bounce_axis
// computes by the same operations -- and the seed already past genVec's three draws, this is glass_children's k, Schlick weight R,
// refraction direction and second child (origin, direction, throughput throughput * (color ^* (1 - R)), seed one draw further),
// operation for operation; the first child is (p + reflection ^* epsilon, reflection, throughput * (color ^* R), seed), which is
// what the ordinary path makes of `next = reflection` and the factor R.  sqrt_rn == IEEE sqrtf.
__device__ __forceinline__ float glass_refraction_child(V3 color, GlassConstants gc, V3 p, V3 n, V3 d, float ia, V3 reflection, V3 throughput, Sfc32 seed,
                                                        V3 &o1, V3 &d1, V3 &t1, Sfc32 &s1)
{
    const float cosi = -ia;
    const float eta = gc.eta;
    const float k = 1.0f - (eta * eta) * (1.0f - cosi * cosi);
    const float r0 = gc.r0;
    const float mm = 1.0f - cosi;
    float R = r0 + (1.0f - r0) * (((mm * mm) * (mm * mm)) * mm);
    V3 refraction;
    if (k < 0.0f) { R = 1.0f; refraction = reflection; }
    else refraction = scale_l(eta, d) + scale_l(eta * cosi - sqrt_rn(k), n);
    o1 = p + scale_r(refraction, kEpsilon); d1 = refraction;
    t1 = throughput * scale_r(color, 1.0f - R);
    (void)random_float(seed);
    s1 = seed;
    return R;
}

inline unsigned int blocks_for(long long n, int block = kBlock) { return (unsigned int)((n + block - 1) / block); }

// Sample chunks (render_inline_kernel): only when the launch has few rounds of waves and every copy keeps >= 64 samples
// (every copy re-evaluates the primary hit and moves the planes once more).  Sets b.spp_chunks (>= 1) and clears the flags.
// `rounds`: how many rounds of waves the launch should have at least.  16 for the kernels whose copies are cheap to start (Inline and the Streams
// chain: one part of 8 of a 4K image at 1024 spp is flat between 5 and 8 copies, 21.9 ms, against 22.6 with 2 and 22.4 with 16); 10 for the tree walk,
// every copy of which evaluates its pixels' start records -- up to three traces and a glass split -- again (C5 per part: 29.2-29.3 ms with 4 copies,
// 29.6-29.8 with 7, 30.7 with one; 1080p / 256 spp: 28.5 with one or two, 28.9 with 4).
inline hipError_t choose_sample_chunks(RenderArgs &b, unsigned int per_copy, int waves_per_simd, hipStream_t stream, unsigned long long rounds = 16)
{
    const int wanted = b.spp_chunks;                           // 0 = automatic, 1 = off, k = forced
    b.spp_chunks = 1;
    if (!b.chunk_done || b.chunk_capacity < per_copy || wanted == 1 || b.screen_x) return hipSuccess;
    const int cus = b.cus > 0 ? b.cus : 256;                   // of the context's device (ptmi_create)
    const unsigned long long slots = (unsigned long long)cus * 4ull * (unsigned long long)waves_per_simd;
    int k = wanted > 1 ? wanted : (int)((rounds * slots + per_copy - 1) / per_copy);
    if (wanted <= 0 && k > b.n_spp / 64) k = b.n_spp / 64;
    if (k > b.n_spp) k = b.n_spp;
    if (k > 64) k = 64;
    if (k < 2) return hipSuccess;
    b.spp_chunks = k;
    if (hipError_t e = hipMemsetAsync(b.chunk_done, 0, (size_t)per_copy * sizeof(unsigned int), stream)) return e;
    return hipMemsetAsync(b.chunk_done + b.chunk_capacity, 0, sizeof(unsigned int), stream);      // the ticket counter
}

inline bool renders_nothing(const RenderArgs &a) { return (long long)a.rows_local * a.width <= 0; }
inline bool scene_fits_lds(const RenderArgs &a) { return (size_t)a.scene.total_f4() * sizeof(float4) <= kMaxSceneLds; }

// How a per-pixel kernel (Inline, the Streams chain, the tree walk) maps waves to pixels: 8x8 tiles once the image has whole tiles and
// rows of 64 otherwise (kAuto), or the one an explicit variant asks for.
enum class Mapping { kAuto, kTiles, kRows };

// The launch of a per-pixel kernel: nothing for a part without pixels; the tiled kernel with the sample chunks choose_sample_chunks picks
// for `waves_per_simd` and `rounds`, or the row kernel over every pixel.  lds_scene: the packed scene is staged in LDS (dynamic LDS of its
// size), not read through scalar loads.  extra: the kernels' arguments after the RenderArgs (a BVH scene's BvhView).
template <typename... P, typename... A>
inline hipError_t launch_per_pixel(const RenderArgs &a, Mapping mapping, void (*tiled)(RenderArgs, P...), void (*rows)(RenderArgs, P...),
                                   bool lds_scene, int waves_per_simd, unsigned long long rounds, hipStream_t stream, const A &...extra)
{
    if (renders_nothing(a)) return hipSuccess;
    const size_t lds = lds_scene ? (size_t)a.scene.total_f4() * sizeof(float4) : 0;
    if (mapping == Mapping::kRows || (mapping == Mapping::kAuto && !tiles_pay(a)))
        return launch(rows, dim3(blocks_for((long long)a.rows_local * a.width, kRenderBlock)), dim3(kRenderBlock), lds, stream, a, extra...);
    RenderArgs b = a;
    const unsigned int per_copy = tile_grid(a, 8);
    if (hipError_t e = choose_sample_chunks(b, per_copy, waves_per_simd, stream, rounds)) return e;
    return launch(tiled, dim3(per_copy * (unsigned int)b.spp_chunks), dim3(kRenderBlock), lds, stream, b, extra...);
}

// Streams' step figure is per launch: every shard of stream_iterations starts at zero (nothing for a part that launches nothing)
inline hipError_t clear_stream_iterations(const RenderArgs &a, hipStream_t stream)
{
    if (renders_nothing(a)) return hipSuccess;
    return hipMemsetAsync(a.stream_iterations, 0, (size_t)kStatShards * 2 * kStatStride * sizeof(unsigned int), stream);
}

}  // namespace

}  // namespace ptmi
