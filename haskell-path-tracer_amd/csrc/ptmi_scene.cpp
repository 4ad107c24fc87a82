// ptmi_scene.cpp -- the scene's calls of include/ptmi.h: setting a scene (linear, BVH, mesh), moving and replacing its spheres and triangles on
// the device, reading the hierarchies back.  Every call prepares a Candidate -- the fresh blocks and what they hold -- and, when all of it
// stands on the device, hands it to commit(), the one place that installs into the context's SceneState (ptmi_ctx.h).  A call that fails
// before that leaves the scene it found: the candidate's destructor frees what was made.
#include "ptmi_ctx.h"

#include <cmath>
#include <string>
#include <vector>

#include "ptmi_bvh.h"
#include "ptmi_bvh_box.h"
#include "ptmi_bvh_spatial.h"
#include "ptmi_mesh.h"
#include "ptmi_mesh_box.h"
#include "ptmi_mesh_morton.h"
#include "ptmi_share.h"

using namespace ptmi;

namespace {

// What a call wants the scene to become.  Its blocks are the call's own until commit() takes them; whatever it still holds when it dies is freed
// (the stream is drained by then: drain(), or nothing was enqueued).  Runtime calls go through alloc / copy / then, which stop at the first error.
struct Candidate {
    ptmi_ctx *c;
    bool whole = false;                                    // a whole scene of `kind`: nothing of the old one stays
    SceneKind kind = SceneKind::Linear;
    DeviceBlock packed, packed_shadow;
    PackedRows rows;
    uint64_t share_xy = 0;                                 // of `packed` (shared_xy_mask, ptmi_share.h): a linear scene's; 0 for the hierarchies
    float sphere_reach = 0.0f;                             // of `packed`, a linear scene's (sphere_reach_of); the hierarchies have their boxes
    Hierarchy<SphereLayout> spheres;                       // block, plan (and, a refit's first, shadow) with their layouts, levels and box
    Hierarchy<MeshLayout> triangles;                       // block, shadow, plan
    bool refit_spheres = false, refit_triangles = false;   // the second blocks were written: they swap with the scene's (the boxes are new)
    DeviceBlock sort, work;                                // scratch of the device builds
    int glass_spheres = -1, glass_planes = -1, glass_triangles = -1;   // -1: as they were
    hipError_t e = hipSuccess;

    explicit Candidate(ptmi_ctx *ctx) : c(ctx) {}
    Candidate(ptmi_ctx *ctx, SceneKind k) : c(ctx), whole(true), kind(k) {}
    Candidate(const Candidate &) = delete;
    Candidate &operator=(const Candidate &) = delete;
    ~Candidate()
    {
        for (DeviceBlock *b : {&packed, &packed_shadow, &spheres.block, &spheres.shadow, &spheres.plan, &triangles.block, &triangles.shadow, &triangles.plan, &sort, &work})
            release(*b);
    }

    void alloc(DeviceBlock &b, size_t bytes) { if (e == hipSuccess) e = allocate(b, bytes); }
    void copy(void *dst, const void *src, size_t bytes, hipMemcpyKind kind_of) { if (e == hipSuccess) e = hipMemcpyAsync(dst, src, bytes, kind_of, c->stream); }
    template <class F> void then(F &&f) { if (e == hipSuccess) e = f(); }
    int status() { return e == hipSuccess ? PTMI_OK : fail_hip(c, e, "e"); }
    // The stream is drained before anything is freed or installed (grow()'s rule), and a launch that failed on the device is seen while the
    // old scene still stands.
    int drain()
    {
        const hipError_t drained = hipStreamSynchronize(c->stream);
        if (e == hipSuccess) e = drained;
        return status();
    }
};

// The views the kernels take, into whichever blocks the scene holds now
void point_views(SceneState &s)
{
    s.bvh = BvhView{};
    s.mesh = MeshView{};
    if (!s.hierarchical()) return;
    const float4 *sb = s.spheres.block.as<float4>();
    s.bvh.nodes = sb;
    s.bvh.geom = sb + s.spheres.layout.geom_at();
    s.bvh.index = reinterpret_cast<const int *>(sb + s.spheres.layout.index_at());
    for (int a = 0; a < 3; ++a) { s.bvh.lo[a] = s.spheres.lo[a]; s.bvh.hi[a] = s.spheres.hi[a]; }
    if (s.kind != SceneKind::Mesh) return;
    const float4 *tb = s.triangles.block.as<float4>();
    const MeshLayout &l = s.triangles.layout;
    s.mesh.spheres = s.bvh;
    s.mesh.nodes = tb;
    s.mesh.geom = tb + l.geom_at();
    s.mesh.index = reinterpret_cast<const int *>(tb + l.index_at());
    s.mesh.by_index = tb + l.by_index_at();
    s.mesh.n_triangles = (int)l.nt;
    s.mesh.n_kept = (int)l.kept;
    for (int a = 0; a < 3; ++a) { s.mesh.lo[a] = s.triangles.lo[a]; s.mesh.hi[a] = s.triangles.hi[a]; }
}

// THE installation: the candidate's blocks over the scene's, what they replace and what depended on it freed, the views, GLASS, the version.
// Nothing here can fail, and nothing else writes the scene.  The stream is drained (Candidate::drain) unless the candidate only swaps.
void commit(Candidate &k)
{
    SceneState &s = k.c->scene;
    auto take = [](DeviceBlock &into, DeviceBlock &from) { release(into); into = from; from = DeviceBlock{}; };
    auto take_tree = [&](auto &into, auto &from) {
        take(into.block, from.block);
        take(into.plan, from.plan);
        into.layout = from.layout;
        into.plan_layout = from.plan_layout;
        into.level_first = std::move(from.level_first);
    };
    if (k.whole) {
        s.each_block([](DeviceBlock &b) { release(b); });
        s.spheres = Hierarchy<SphereLayout>{};
        s.triangles = Hierarchy<MeshLayout>{};
        s.kind = k.kind;
    }
    // the sphere refit's second blocks are copies of `packed` and of spheres.block (the materials, the planes, the references and indices
    // never move): whatever replaces either block frees the pair, and the next refit makes it afresh
    if (k.packed.p || k.spheres.block.p) { release(s.packed_shadow); release(s.spheres.shadow); }
    if (k.packed.p) { take(s.packed, k.packed); s.rows = k.rows; }
    // the sharing mask is the packed block's: whatever replaces the block (or the whole scene) replaces the mask, so none outlives its spheres
    if (k.packed.p || k.whole) { s.share_xy = k.share_xy; s.sphere_reach = k.sphere_reach; }
    if (k.spheres.block.p) take_tree(s.spheres, k.spheres);
    // (the mesh refit's second block comes with the block it copies)
    if (k.triangles.block.p) { take_tree(s.triangles, k.triangles); take(s.triangles.shadow, k.triangles.shadow); }
    if (k.refit_spheres) {
        if (k.spheres.shadow.p) { take(s.spheres.shadow, k.spheres.shadow); take(s.packed_shadow, k.packed_shadow); }
        std::swap(s.spheres.block, s.spheres.shadow);
        std::swap(s.packed, s.packed_shadow);
    }
    if (k.refit_triangles) std::swap(s.triangles.block, s.triangles.shadow);
    if (k.spheres.block.p || k.refit_spheres || k.whole) s.spheres.set_box(k.spheres.lo, k.spheres.hi);
    if (k.triangles.block.p || k.refit_triangles || k.whole) s.triangles.set_box(k.triangles.lo, k.triangles.hi);
    if (k.glass_spheres >= 0) s.glass_spheres = k.glass_spheres != 0;
    if (k.glass_planes >= 0) s.glass_planes = k.glass_planes != 0;
    if (k.glass_triangles >= 0) s.glass_triangles = k.glass_triangles != 0;
    s.has_glass = s.glass_spheres || s.glass_planes || s.glass_triangles;
    point_views(s);
    ++s.version;
}

// ---- steps the calls share --------------------------------------------------------------------------------------------------------------

template <class T> int check_tags(ptmi_ctx *c, const T *prims, int n, const char *what)
{
    for (int i = 0; i < n; ++i)
        if (prims[i].brdf_tag < PTMI_MATTE || prims[i].brdf_tag > PTMI_GLASS) return fail(c, PTMI_EINVAL, std::string(what) + " with unknown brdf_tag");
    return PTMI_OK;
}

template <class T> int any_glass(const T *prims, int n)
{
    for (int i = 0; i < n; ++i)
        if (prims[i].brdf_tag == PTMI_GLASS) return 1;
    return 0;
}

// What ptmi_set_scene_bvh and ptmi_set_scene_mesh refuse alike (a BVH scene has no triangles)
int refuse_hierarchy_scene(ptmi_ctx *c, SceneKind kind, const ptmi_sphere *spheres, int n_spheres, const ptmi_plane *planes, int n_planes,
                           const ptmi_triangle *triangles, int n_triangles)
{
    const std::string a_scene = kind == SceneKind::Mesh ? "a mesh scene" : "a BVH scene";
    if (n_spheres < 0 || n_planes < 0 || n_triangles < 0 || (n_spheres > 0 && !spheres) || (n_planes > 0 && !planes) || (n_triangles > 0 && !triangles))
        return fail(c, PTMI_EINVAL, "bad scene arguments");
    // expMinWith _ [] = error "Invalid call to 'expMinWith'"   (src/Util.hs:172)
    if ((long long)n_spheres + n_planes + n_triangles == 0) return fail(c, PTMI_EINVAL, "empty scene (expMinWith on an empty list)");
    if (n_spheres > PTMI_MAX_BVH_SPHERES) return fail(c, PTMI_ELIMIT, "more spheres than PTMI_MAX_BVH_SPHERES");
    if (n_planes > PTMI_MAX_BVH_PLANES) return fail(c, PTMI_ELIMIT, "more planes than PTMI_MAX_BVH_PLANES");
    if (n_triangles > PTMI_MAX_MESH_TRIANGLES) return fail(c, PTMI_ELIMIT, "more triangles than PTMI_MAX_MESH_TRIANGLES");
    if (c->variant != kVariantAuto) return fail(c, PTMI_EINVAL, a_scene + " renders through the default kernels: ptmi_set_variant(ctx, 0) first");
    if (c->opt_form == PTMI_FORM_STREAM)
        return fail(c, PTMI_EINVAL, a_scene + " has no stream form: set PTMI_OPT_STREAMS_FORM to PTMI_FORM_AUTO or PTMI_FORM_PIXEL first");
    if (kind == SceneKind::Mesh && c->opt_arithmetic == PTMI_ARITH_CONTRACTED)
        return fail(c, PTMI_EINVAL, a_scene + " has no contracted-arithmetic kernel: set PTMI_OPT_ARITHMETIC back first");
    if (int rc = check_tags(c, spheres, n_spheres, "sphere")) return rc;
    if (int rc = check_tags(c, planes, n_planes, "plane")) return rc;
    return check_tags(c, triangles, n_triangles, "triangle");
}

// The packed scene of `rows` on the host (triangles: their materials only, primitive ns + np + k)
void pack_scene(const PackedRows &rows, const ptmi_sphere *sph, const ptmi_plane *pl, const ptmi_triangle *tri, std::vector<float4> &out)
{
    out.assign(rows.rows(), float4{0, 0, 0, 0});
    for (size_t i = 0; i < rows.ns; ++i)
        out[i] = float4{sph[i].position[0], sph[i].position[1], sph[i].position[2], sph[i].radius * sph[i].radius};
    for (size_t j = 0; j < rows.np; ++j) {
        out[rows.planes_at() + 2 * j] = float4{pl[j].position[0], pl[j].position[1], pl[j].position[2], 0.0f};
        out[rows.planes_at() + 2 * j + 1] = float4{pl[j].direction[0], pl[j].direction[1], pl[j].direction[2], 0.0f};
    }
    size_t k = rows.materials_at();
    auto mat = [&](const float *color, float illum, int32_t tag, float p) {
        out[k++] = float4{color[0], color[1], color[2], illum};
        out[k++] = float4{u2f((uint32_t)tag), p, p / kPi, 0.5f * (1.0f - p)};
    };
    for (size_t i = 0; i < rows.ns; ++i) mat(sph[i].color, sph[i].illuminance, sph[i].brdf_tag, sph[i].brdf_param);
    for (size_t j = 0; j < rows.np; ++j) mat(pl[j].color, pl[j].illuminance, pl[j].brdf_tag, pl[j].brdf_param);
    for (size_t t = 0; t < rows.nt; ++t) mat(tri[t].color, tri[t].illuminance, tri[t].brdf_tag, tri[t].brdf_param);
}

// The largest magnitude among the sphere rows (cx, cy, cz, r * r) of a packed linear scene, +inf when one of them is not finite
float sphere_reach_of(const float4 *rows, int n_spheres)
{
    float reach = 0.0f;
    for (int i = 0; i < n_spheres; ++i)
        for (float v : {rows[i].x, rows[i].y, rows[i].z, rows[i].w})
            reach = std::isfinite(v) ? std::fmax(reach, std::fabs(v)) : INFINITY;
    return reach;
}

// The sphere hierarchy of a host build: its block (nodes, the spheres in leaf order as pack_scene makes them, their indices) and its plan
// block (what ptmi_update_spheres needs of it: the result words, the nodes by level) on the host, and their description in k.spheres
void stage_sphere_hierarchy(const BvhBuild &bb, const std::vector<float4> &packed, Candidate &k, std::vector<float4> &hier, std::vector<char> &plan_block)
{
    Hierarchy<SphereLayout> &h = k.spheres;
    const size_t ns = bb.order.size();
    h.layout = SphereLayout{bb.nodes.size(), ns};
    hier.assign(h.layout.bytes() / sizeof(float4), float4{0, 0, 0, 0});
    std::memcpy(hier.data(), bb.nodes.data(), bb.nodes.size() * sizeof(ptmi_bvh_node));
    for (size_t i = 0; i < ns; ++i) hier[h.layout.geom_at() + i] = packed[(size_t)bb.order[i]];
    if (ns > 0) std::memcpy(&hier[h.layout.index_at()], bb.order.data(), ns * sizeof(int32_t));
    BvhLevelPlan plan;
    bvh_level_plan(bb.nodes, plan);
    h.plan_layout = PlanLayout{0, plan.level_nodes.size()};
    plan_block.assign(h.plan_layout.bytes(), 0);
    std::memcpy(&plan_block[h.plan_layout.levels_at()], plan.level_nodes.data(), plan.level_nodes.size() * sizeof(int32_t));
    h.level_first = std::move(plan.level_first);
    h.set_box(bb.lo, bb.hi);
}

// A check kernel's verdict.  The three check kernels (ptmi_mesh_box.h, ptmi_mesh_morton.h, ptmi_bvh_box.h) report alike: word 0 the smallest
// (primitive << 2 | code) refused or all ones, then the box as ordered keys, then counts -- preset to all ones before the box's high corner
// and to zero from there, read back with the call's first synchronisation.
static_assert(kRefitError == 0 && kBuildError == 0 && kSphError == 0 && kRefitLo == 1 && kBuildLo == 1 && kSphLo == 1 && kRefitHi == 4 && kBuildHi == 4 && kSphHi == 4,
              "the check kernels' result words begin alike");
enum { kCheckError = 0, kCheckLo = 1, kCheckHi = 4 };

template <size_t Words, class Launch> int run_check(ptmi_ctx *c, unsigned int *result, unsigned int (&got)[Words], Launch &&launch)
{
    PTMI_HIP(c, hipMemsetAsync(result, 0xff, kCheckHi * sizeof(unsigned int), c->stream));
    PTMI_HIP(c, hipMemsetAsync(result + kCheckHi, 0, (Words - kCheckHi) * sizeof(unsigned int), c->stream));
    PTMI_HIP(c, launch());
    PTMI_HIP(c, hipMemcpyAsync(got, result, sizeof got, hipMemcpyDeviceToHost, c->stream));
    PTMI_HIP(c, hipStreamSynchronize(c->stream));
    return PTMI_OK;
}

bool refused(const unsigned int *got) { return got[kCheckError] != 0xffffffffu; }
std::string who(const char *what, const unsigned int *got) { return std::string(what) + " " + std::to_string(got[kCheckError] >> 2); }
unsigned int why(const unsigned int *got) { return got[kCheckError] & 3u; }

// (the box of nothing is the origin)
void box_of(const unsigned int *got, bool any, float lo[3], float hi[3])
{
    for (int a = 0; a < 3; ++a) {
        lo[a] = any ? ordered_value(got[kCheckLo + a]) : 0.0f;
        hi[a] = any ? ordered_value(got[kCheckHi + a]) : 0.0f;
    }
}

// One launch per level of a hierarchy, the deepest first: launch(the level's nodes, how many)
template <class Launch> hipError_t each_level(const std::vector<int32_t> &level_first, const int32_t *level_nodes, Launch &&launch)
{
    for (size_t lv = 0; lv + 1 < level_first.size(); ++lv) {
        const hipError_t e = launch(level_nodes + level_first[lv], level_first[lv + 1] - level_first[lv]);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

// The device, and -- the host-pointer entries (`staging` given) -- the caller's array staged: `array` is device memory afterwards
int on_device(ptmi_ctx *c, DeviceBlock *staging, const char *what, size_t bytes, const float *&array)
{
    PTMI_HIP(c, hipSetDevice(c->device));
    if (!staging) return PTMI_OK;
    if (bytes > 0) {
        if (int rc = grow(c, *staging, bytes, what)) return rc;
        CopySpan span{staging->p, const_cast<float *>(array), bytes};
        PTMI_HIP(c, copy_to_device(c, &span, 1));
    }
    array = staging->as<float>();
    return PTMI_OK;
}

// ---- the device calls: ptmi_x(host array) and ptmi_x_device(device array) ---------------------------------------------------------------

// Moving the vertices of the current mesh scene (see include/ptmi.h).  One validation path, on the device: the check kernel reads the new
// vertices only; the host reads its verdict and the new box back with the call's ONE synchronisation; only then are the writing kernels
// enqueued -- into the second mesh block, which becomes the scene's when all of them are out.
int update_mesh_vertices(ptmi_ctx *c, const float *vertices, int n, bool from_host)
{
    if (!c) return PTMI_EINVAL;
    std::lock_guard<std::mutex> lock(c->mu);
    SceneState &s = c->scene;
    if (s.kind != SceneKind::Mesh) return fail(c, PTMI_ESTATE, "the current scene is not a mesh scene (ptmi_set_scene_mesh): there are no vertices to move");
    if (n != s.mesh.n_triangles)
        return fail(c, PTMI_EINVAL, "the scene has " + std::to_string(s.mesh.n_triangles) + " triangles, not " + std::to_string(n) +
                                        ": an update moves vertices, it does not change the topology");
    if (n > 0 && !vertices) return fail(c, PTMI_EINVAL, "bad vertex arguments");
    if (int rc = on_device(c, from_host ? &s.triangles.staging : nullptr, "vertex staging", (size_t)n * 9 * sizeof(float), vertices)) return rc;
    const Hierarchy<MeshLayout> &h = s.triangles;
    unsigned int got[kRefitWords];
    if (int rc = run_check(c, h.result(), got, [&] { return launch_mesh_refit_check(vertices, n, h.leaf_pos(), h.result(), c->stream); })) return rc;
    if (refused(got)) {
        switch (why(got)) {
        case kRefitBadVertex: return fail(c, PTMI_EINVAL, who("triangle", got) + ": a vertex is not finite: a box cannot bound it");
        case kRefitBadNormal: return fail(c, PTMI_EINVAL, who("triangle", got) + ": its edges, normal or normal^2 are not finite");
        default:
            return fail(c, PTMI_EINVAL, who("triangle", got) + " had zero area when the scene was set and is in no leaf: it cannot gain area, set the scene again (ptmi_set_scene_mesh)");
        }
    }
    float4 *shadow = h.shadow.as<float4>(), *geom = shadow + h.layout.geom_at();
    PTMI_HIP(c, launch_mesh_refit_records(vertices, n, h.leaf_pos(), shadow + h.layout.by_index_at(), geom, c->stream));
    PTMI_HIP(c, each_level(h.level_first, h.level_nodes(), [&](const int32_t *nodes, int count) { return launch_mesh_refit_level(shadow, geom, nodes, count, c->stream); }));
    Candidate k(c);
    k.refit_triangles = true;
    box_of(got, h.layout.kept > 0, k.triangles.lo, k.triangles.hi);
    commit(k);
    return PTMI_OK;
}

// New triangles for the current mesh scene (see include/ptmi.h).  The check kernel reads the new triangles only; the host reads its
// verdict, the kept count, the box and the GLASS flag back together; then fresh blocks -- the scene block with the new material tail,
// both mesh blocks, the refit's plan -- are filled on the stream and become the scene's when all of it is through: update_mesh_vertices'
// discipline with fresh allocations, the sizes change.
int set_mesh_triangles(ptmi_ctx *c, const float *triangles, int n, bool from_host)
{
    if (!c) return PTMI_EINVAL;
    std::lock_guard<std::mutex> lock(c->mu);
    SceneState &s = c->scene;
    if (s.kind != SceneKind::Mesh) return fail(c, PTMI_ESTATE, "the current scene is not a mesh scene (ptmi_set_scene_mesh): there are no triangles to replace");
    if (n < 0 || (n > 0 && !triangles)) return fail(c, PTMI_EINVAL, "bad triangle arguments");
    if (n > PTMI_MAX_MESH_TRIANGLES) return fail(c, PTMI_ELIMIT, "more triangles than PTMI_MAX_MESH_TRIANGLES");
    if (n == 0 && s.rows.ns + s.rows.np == 0) return fail(c, PTMI_EINVAL, "empty scene (expMinWith on an empty list)");
    if (int rc = on_device(c, from_host ? &s.triangles.staging : nullptr, "triangle staging", (size_t)n * sizeof(ptmi_triangle), triangles)) return rc;
    unsigned int got[kBuildWords];
    if (int rc = run_check(c, s.triangles.result(), got, [&] { return launch_mesh_build_check(triangles, n, s.triangles.result(), c->stream); })) return rc;
    if (refused(got)) {
        switch (why(got)) {
        case kBuildBadVertex: return fail(c, PTMI_EINVAL, who("triangle", got) + ": a vertex is not finite: a box cannot bound it");
        case kBuildBadMaterial: return fail(c, PTMI_EINVAL, who("triangle", got) + ": its colour, illuminance or brdf_param is not finite");
        case kBuildBadNormal: return fail(c, PTMI_EINVAL, who("triangle", got) + ": its edges, normal or normal^2 are not finite");
        default: return fail(c, PTMI_EINVAL, who("triangle", got) + ": unknown brdf_tag");
        }
    }
    if (got[kBuildKept] > (unsigned int)n) return fail(c, PTMI_EHIP, "the check kernel counted more kept triangles than there are");
    const int kept = (int)got[kBuildKept];
    Candidate k(c);
    Hierarchy<MeshLayout> &h = k.triangles;
    box_of(got, kept > 0, h.lo, h.hi);
    k.glass_triangles = got[kBuildGlass] != 0;
    // the topology and its levels are functions of the kept count alone (ptmi_mesh_morton.h)
    MeshBuild mb;
    MeshRefitPlan plan;
    morton_topology(kept, mb.nodes);
    mesh_refit_plan(mb, 0, plan);
    k.rows = PackedRows{s.rows.ns, s.rows.np, (size_t)n};
    h.layout = MeshLayout{mb.nodes.size(), (size_t)kept, (size_t)n};
    h.plan_layout = PlanLayout{(size_t)n, plan.level_nodes.size()};
    k.alloc(k.packed, k.rows.bytes());
    k.alloc(h.block, h.layout.bytes());
    k.alloc(h.shadow, h.layout.bytes());
    k.alloc(h.plan, h.plan_layout.bytes());
    if (kept > 0) k.alloc(k.sort, mesh_build_sort_bytes(n));
    if (int rc = k.status()) return rc;
    float4 *nodes = h.block.as<float4>(), *geom = nodes + h.layout.geom_at();
    int32_t *order = reinterpret_cast<int32_t *>(nodes + h.layout.index_at());
    // the spheres and planes, and their materials, stay
    if (s.rows.triangle_materials_at() > 0) k.copy(k.packed.p, s.packed.p, s.rows.triangle_materials_at() * sizeof(float4), hipMemcpyDeviceToDevice);
    k.then([&] {
        CopySpan spans[2] = {{nodes, mb.nodes.data(), mb.nodes.size() * sizeof(ptmi_bvh_node)}, {h.level_nodes(), plan.level_nodes.data(), plan.level_nodes.size() * sizeof(int32_t)}};
        return copy_to_device(c, spans, 2);
    });
    if (n > 0)
        k.then([&] {
            if (kept > 0) return launch_mesh_build_order(triangles, n, kept, h.lo, h.hi, k.sort.p, h.leaf_pos(), order, c->stream);
            return hipMemsetAsync(h.leaf_pos(), 0xff, (size_t)n * sizeof(int32_t), c->stream);                // no triangle is in a leaf
        });
    k.then([&] {
        return launch_mesh_build_scatter(triangles, n, kept, h.leaf_pos(), nodes + h.layout.by_index_at(), geom, k.packed.as<float4>() + k.rows.triangle_materials_at(), c->stream);
    });
    k.then([&] { return each_level(plan.level_first, h.level_nodes(), [&](const int32_t *level, int count) { return launch_mesh_refit_level(nodes, geom, level, count, c->stream); }); });
    // (the second block starts as a copy: an update rewrites every record and every box of it, the references and indices never move)
    k.copy(h.shadow.p, h.block.p, h.block.bytes, hipMemcpyDeviceToDevice);
    if (int rc = k.drain()) return rc;                     // `mb` and `plan` die at return
    h.level_first = std::move(plan.level_first);
    commit(k);
    return PTMI_OK;
}

// Moving the spheres of the current BVH or mesh scene (see include/ptmi.h).  One validation path, on the device: the check kernel reads the
// new geometry only; the host reads its verdict and the new box of the centres back with the call's ONE synchronisation; only then are
// the writing kernels enqueued -- into the second hierarchy and scene blocks, which become the scene's when all of them are out.
int update_spheres(ptmi_ctx *c, const float *geometry, int n, bool from_host)
{
    if (!c) return PTMI_EINVAL;
    std::lock_guard<std::mutex> lock(c->mu);
    SceneState &s = c->scene;
    if (!s.hierarchical())
        return fail(c, PTMI_ESTATE, "the current scene is not a BVH or mesh scene (ptmi_set_scene_bvh, ptmi_set_scene_mesh): there is no hierarchy to refit");
    if ((size_t)n != s.rows.ns || n < 0)
        return fail(c, PTMI_EINVAL, "the scene has " + std::to_string(s.rows.ns) + " spheres, not " + std::to_string(n) +
                                        ": an update moves spheres, it does not change their count (ptmi_set_bvh_spheres does)");
    if (n > 0 && !geometry) return fail(c, PTMI_EINVAL, "bad sphere arguments");
    if (int rc = on_device(c, from_host ? &s.spheres.staging : nullptr, "sphere staging", (size_t)n * 4 * sizeof(float), geometry)) return rc;
    if (n == 0) return PTMI_OK;                            // (a scene without spheres: nothing moves)
    const Hierarchy<SphereLayout> &h = s.spheres;
    unsigned int got[kSphWords];
    if (int rc = run_check(c, h.result(), got, [&] { return launch_bvh_check(geometry, 4, n, h.result(), c->stream); })) return rc;
    if (refused(got)) return fail(c, PTMI_EINVAL, who("sphere", got) + ": its position, radius or radius^2 is not finite: a box cannot bound it");
    Candidate k(c);
    k.refit_spheres = true;
    box_of(got, true, k.spheres.lo, k.spheres.hi);
    if (!h.shadow.p || !s.packed_shadow.p) {
        // (after the verdict: a refused update allocates nothing)  The second blocks start as copies of the scene's: an update rewrites
        // every box, every sphere record and every sphere row of them
        k.alloc(k.spheres.shadow, h.block.bytes);
        k.alloc(k.packed_shadow, s.packed.bytes);
        k.copy(k.spheres.shadow.p, h.block.p, h.block.bytes, hipMemcpyDeviceToDevice);
        k.copy(k.packed_shadow.p, s.packed.p, s.packed.bytes, hipMemcpyDeviceToDevice);
        if (int rc = k.status()) return rc;
    }
    float4 *shadow = (k.spheres.shadow.p ? k.spheres.shadow : h.shadow).as<float4>(), *rows = (k.packed_shadow.p ? k.packed_shadow : s.packed_shadow).as<float4>();
    float4 *geom = shadow + h.layout.geom_at();
    const int32_t *order = reinterpret_cast<const int32_t *>(shadow + h.layout.index_at());
    k.then([&] { return launch_bvh_records(geometry, 4, n, order, geom, rows, nullptr, c->stream); });
    k.then([&] { return each_level(h.level_first, h.level_nodes(), [&](const int32_t *level, int count) { return launch_bvh_level(shadow, geometry, 4, n, order, level, count, c->stream); }); });
    if (k.e != hipSuccess) return k.drain();               // (fresh second blocks are freed on the way out: what was enqueued into them is through first)
    commit(k);
    return PTMI_OK;
}

// New spheres for the current BVH or mesh scene (see include/ptmi.h).  The check kernel reads the new spheres only; the host reads its
// verdict, the box of the centres and the GLASS flag back together (the first synchronisation); then fresh blocks -- the scene block for
// the new count, the hierarchy, its plan -- are filled on the stream and become the scene's when all of it is through (the second).  Under
// PTMI_BVH_BUILD_SPATIAL the topology is built on the device first and the counts of its levels are read back (one synchronisation more,
// three in all).
int set_bvh_spheres(ptmi_ctx *c, const float *spheres, int n, bool from_host)
{
    if (!c) return PTMI_EINVAL;
    std::lock_guard<std::mutex> lock(c->mu);
    SceneState &s = c->scene;
    if (!s.hierarchical())
        return fail(c, PTMI_ESTATE, "the current scene is not a BVH or mesh scene (ptmi_set_scene_bvh, ptmi_set_scene_mesh): there are no spheres to replace");
    if (n < 0 || (n > 0 && !spheres)) return fail(c, PTMI_EINVAL, "bad sphere arguments");
    if (n > PTMI_MAX_BVH_SPHERES) return fail(c, PTMI_ELIMIT, "more spheres than PTMI_MAX_BVH_SPHERES");
    if (n == 0 && s.rows.np + s.rows.nt == 0) return fail(c, PTMI_EINVAL, "empty scene (expMinWith on an empty list)");
    if (int rc = on_device(c, from_host ? &s.spheres.staging : nullptr, "sphere staging", (size_t)n * sizeof(ptmi_sphere), spheres)) return rc;
    unsigned int got[kSphWords];
    if (int rc = run_check(c, s.spheres.result(), got, [&] { return launch_bvh_check(spheres, 10, n, s.spheres.result(), c->stream); })) return rc;
    if (refused(got)) {
        switch (why(got)) {
        case kSphBadGeometry: return fail(c, PTMI_EINVAL, who("sphere", got) + ": its position, radius or radius^2 is not finite: a box cannot bound it");
        case kSphBadMaterial: return fail(c, PTMI_EINVAL, who("sphere", got) + ": its colour, illuminance or brdf_param is not finite");
        default: return fail(c, PTMI_EINVAL, who("sphere", got) + ": unknown brdf_tag");
        }
    }
    Candidate k(c);
    Hierarchy<SphereLayout> &h = k.spheres;
    box_of(got, n > 0, h.lo, h.hi);
    k.glass_spheres = got[kSphGlass] != 0;
    const bool spatial = c->opt_bvh_build == PTMI_BVH_BUILD_SPATIAL;
    std::vector<ptmi_bvh_node> topology;
    BvhLevelPlan plan;
    size_t n_nodes = 0;
    const uint32_t *sorted = nullptr;
    int level_count[kSpatialWords] = {0};
    int levels = 0;
    if (!spatial) {
        // the topology and its levels are functions of the count alone (ptmi_mesh_morton.h)
        morton_topology(n, topology);
        bvh_level_plan(topology, plan);
        n_nodes = topology.size();
    } else {
        // the topology is the keys' (ptmi_bvh_spatial.h): built level by level into scratch, and the levels' counts read back -- this
        // build's extra synchronisation -- before the hierarchy can be allocated
        if (n > 0) k.alloc(k.sort, mesh_build_sort_bytes(n));
        k.alloc(k.work, bvh_spatial_work_bytes(n));
        k.then([&] { return launch_bvh_spatial_tree(spheres, n, h.lo, h.hi, k.sort.p, k.work.p, &sorted, c->stream); });
        if (k.e == hipSuccess) k.copy(level_count, bvh_spatial_report(k.work.p, n), sizeof level_count, hipMemcpyDeviceToHost);
        if (int rc = k.drain()) return rc;
        // levels of 1, <= 2, <= 4 ... nodes, then none: anything else is not a tree this build makes
        bool sane = level_count[0] == 1;
        for (levels = 0; levels < PTMI_BVH_MAX_DEPTH && level_count[levels] > 0; ++levels) {
            sane = sane && level_count[levels] <= spatial_level_bound(n, levels) && (levels == 0 || level_count[levels] <= 2 * level_count[levels - 1]);
            n_nodes += (size_t)level_count[levels];
        }
        for (int l = levels; l < PTMI_BVH_MAX_DEPTH; ++l) sane = sane && level_count[l] == 0;
        if (!sane || n_nodes > (size_t)spatial_node_bound(n)) return fail(c, PTMI_EHIP, "the device build of the sphere hierarchy reported levels that are no tree");
        plan.level_first.assign(1, 0);
        for (int l = levels - 1; l >= 0; --l) plan.level_first.push_back(plan.level_first.back() + level_count[l]);      // the deepest first
    }
    k.rows = PackedRows{(size_t)n, s.rows.np, s.rows.nt};
    h.layout = SphereLayout{n_nodes, (size_t)n};
    h.plan_layout = PlanLayout{0, n_nodes};
    k.alloc(k.packed, k.rows.bytes());
    k.alloc(h.block, h.layout.bytes());
    k.alloc(h.plan, h.plan_layout.bytes());
    if (n > 0 && !spatial) k.alloc(k.sort, mesh_build_sort_bytes(n));
    if (int rc = k.status()) return rc;
    float4 *scene = k.packed.as<float4>(), *nodes = h.block.as<float4>(), *geom = nodes + h.layout.geom_at();
    const float4 *old_scene = s.packed.as<float4>();
    int32_t *order = reinterpret_cast<int32_t *>(nodes + h.layout.index_at());
    // the planes' rows, and the materials of planes and triangles, move to the offsets of the new count
    if (s.rows.np > 0) k.copy(scene + k.rows.planes_at(), old_scene + s.rows.planes_at(), 2 * s.rows.np * sizeof(float4), hipMemcpyDeviceToDevice);
    if (s.rows.np + s.rows.nt > 0)
        k.copy(scene + k.rows.kept_materials_at(), old_scene + s.rows.kept_materials_at(), 2 * (s.rows.np + s.rows.nt) * sizeof(float4), hipMemcpyDeviceToDevice);
    if (!spatial) {
        k.then([&] {
            CopySpan spans[2] = {{nodes, topology.data(), topology.size() * sizeof(ptmi_bvh_node)}, {h.level_nodes(), plan.level_nodes.data(), plan.level_nodes.size() * sizeof(int32_t)}};
            return copy_to_device(c, spans, 2);
        });
        k.then([&] { return launch_bvh_build_order(spheres, n, h.lo, h.hi, k.sort.p, order, c->stream); });
    } else {
        k.then([&] { return launch_bvh_spatial_finish(k.work.p, n, level_count, levels, nodes, h.level_nodes(), c->stream); });
        if (n > 0) k.copy(order, sorted, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToDevice);      // order[position] = original index
    }
    k.then([&] { return launch_bvh_records(spheres, 10, n, order, geom, scene, scene + k.rows.materials_at(), c->stream); });
    k.then([&] { return each_level(plan.level_first, h.level_nodes(), [&](const int32_t *level, int count) { return launch_bvh_level(nodes, spheres, 10, n, order, level, count, c->stream); }); });
    if (int rc = k.drain()) return rc;                     // `topology` and `plan` die at return
    h.level_first = std::move(plan.level_first);
    commit(k);
    return PTMI_OK;
}

}  // namespace

extern "C" {

int ptmi_set_scene(ptmi_ctx *c, const ptmi_sphere *spheres, int n_spheres, const ptmi_plane *planes, int n_planes)
{
    if (!c) return PTMI_EINVAL;
    std::lock_guard<std::mutex> lock(c->mu);
    if (n_spheres < 0 || n_planes < 0 || (n_spheres > 0 && !spheres) || (n_planes > 0 && !planes))
        return fail(c, PTMI_EINVAL, "bad scene arguments");
    // expMinWith _ [] = error "Invalid call to 'expMinWith'"   (src/Util.hs:172)
    if (n_spheres + n_planes == 0) return fail(c, PTMI_EINVAL, "empty scene (expMinWith on an empty list)");
    if (n_spheres + n_planes > PTMI_MAX_PRIMITIVES) return fail(c, PTMI_ELIMIT, "too many primitives");
    if (int rc = check_tags(c, spheres, n_spheres, "sphere")) return rc;
    if (int rc = check_tags(c, planes, n_planes, "plane")) return rc;
    PTMI_HIP(c, hipSetDevice(c->device));
    Candidate k(c, SceneKind::Linear);
    k.rows = PackedRows{(size_t)n_spheres, (size_t)n_planes, 0};
    k.glass_spheres = any_glass(spheres, n_spheres); k.glass_planes = any_glass(planes, n_planes); k.glass_triangles = 0;
    std::vector<float4> packed;
    pack_scene(k.rows, spheres, planes, nullptr, packed);
    k.share_xy = shared_xy_mask(&packed[0].x, 4, n_spheres);  // of the rows the kernels read
    k.sphere_reach = sphere_reach_of(packed.data(), n_spheres);
    PTMI_HIP(c, hipStreamSynchronize(c->stream));
    // the new scene stands complete before the old one goes
    k.alloc(k.packed, k.rows.bytes());
    k.copy(k.packed.p, packed.data(), k.packed.bytes, hipMemcpyHostToDevice);
    if (int rc = k.drain()) return rc;                     // `packed` dies at return
    commit(k);
    return PTMI_OK;
}

int ptmi_set_scene_bvh(ptmi_ctx *c, const ptmi_sphere *spheres, int n_spheres, const ptmi_plane *planes, int n_planes)
{
    if (!c) return PTMI_EINVAL;
    std::lock_guard<std::mutex> lock(c->mu);
#ifdef PTMI_ABLATIONS
    (void)spheres; (void)n_spheres; (void)planes; (void)n_planes;
    return fail(c, PTMI_EINVAL, "the ablation library has no BVH kernels: use libptmi for BVH scenes");
#else
    if (int rc = refuse_hierarchy_scene(c, SceneKind::Bvh, spheres, n_spheres, planes, n_planes, nullptr, 0)) return rc;
    BvhBuild bb;
    std::string reason;
    if (int rc = bvh_build(spheres, n_spheres, bb, &reason)) return fail(c, rc, reason);
    PTMI_HIP(c, hipSetDevice(c->device));
    Candidate k(c, SceneKind::Bvh);
    k.rows = PackedRows{(size_t)n_spheres, (size_t)n_planes, 0};
    k.glass_spheres = any_glass(spheres, n_spheres); k.glass_planes = any_glass(planes, n_planes); k.glass_triangles = 0;
    std::vector<float4> packed, hier;
    std::vector<char> plan_block;
    pack_scene(k.rows, spheres, planes, nullptr, packed);
    stage_sphere_hierarchy(bb, packed, k, hier, plan_block);
    PTMI_HIP(c, hipStreamSynchronize(c->stream));
    // all blocks stand complete before the old scene goes
    k.alloc(k.packed, k.rows.bytes());
    k.alloc(k.spheres.block, k.spheres.layout.bytes());
    k.alloc(k.spheres.plan, plan_block.size());
    k.copy(k.packed.p, packed.data(), k.packed.bytes, hipMemcpyHostToDevice);
    k.copy(k.spheres.block.p, hier.data(), k.spheres.block.bytes, hipMemcpyHostToDevice);
    k.copy(k.spheres.plan.p, plan_block.data(), k.spheres.plan.bytes, hipMemcpyHostToDevice);
    if (int rc = k.drain()) return rc;                     // `packed`, `hier` and `plan_block` die at return
    commit(k);
    return PTMI_OK;
#endif
}

int ptmi_set_scene_mesh(ptmi_ctx *c, const ptmi_sphere *spheres, int n_spheres, const ptmi_triangle *triangles, int n_triangles,
                        const ptmi_plane *planes, int n_planes)
{
    if (!c) return PTMI_EINVAL;
    std::lock_guard<std::mutex> lock(c->mu);
#ifdef PTMI_ABLATIONS
    (void)spheres; (void)n_spheres; (void)triangles; (void)n_triangles; (void)planes; (void)n_planes;
    return fail(c, PTMI_EINVAL, "the ablation library has no mesh kernels: use libptmi for mesh scenes");
#else
    if (int rc = refuse_hierarchy_scene(c, SceneKind::Mesh, spheres, n_spheres, planes, n_planes, triangles, n_triangles)) return rc;
    BvhBuild bb;
    MeshBuild mb;
    std::string reason;
    if (int rc = bvh_build(spheres, n_spheres, bb, &reason)) return fail(c, rc, reason);
    if (int rc = mesh_build(triangles, n_triangles, mb, &reason)) return fail(c, rc, reason);
    PTMI_HIP(c, hipSetDevice(c->device));
    Candidate k(c, SceneKind::Mesh);
    k.rows = PackedRows{(size_t)n_spheres, (size_t)n_planes, (size_t)n_triangles};
    k.glass_spheres = any_glass(spheres, n_spheres); k.glass_planes = any_glass(planes, n_planes); k.glass_triangles = any_glass(triangles, n_triangles);
    std::vector<float4> packed, hier;
    std::vector<char> plan_block;
    pack_scene(k.rows, spheres, planes, triangles, packed);
    stage_sphere_hierarchy(bb, packed, k, hier, plan_block);
    // the triangle hierarchy's block: the nodes, the kept triangles in leaf order, their original indices, and every triangle by original index
    Hierarchy<MeshLayout> &h = k.triangles;
    const size_t kept = mb.order.size();
    h.layout = MeshLayout{mb.nodes.size(), kept, (size_t)n_triangles};
    h.set_box(mb.lo, mb.hi);
    std::vector<float4> tri(h.layout.bytes() / sizeof(float4));
    std::memcpy(tri.data(), mb.nodes.data(), mb.nodes.size() * sizeof(ptmi_bvh_node));
    for (size_t i = 0; i < kept; ++i) std::memcpy(&tri[h.layout.geom_at() + 3 * i], &mb.records[(size_t)mb.order[i] * 12], 12 * sizeof(float));
    if (kept > 0) std::memcpy(&tri[h.layout.index_at()], mb.order.data(), kept * sizeof(int32_t));
    if (n_triangles > 0) std::memcpy(&tri[h.layout.by_index_at()], mb.records.data(), (size_t)n_triangles * 12 * sizeof(float));
    // ... and its plan: what ptmi_update_mesh_vertices needs of it (the result words, the leaf positions, the nodes by level)
    MeshRefitPlan plan;
    mesh_refit_plan(mb, n_triangles, plan);
    h.plan_layout = PlanLayout{(size_t)n_triangles, plan.level_nodes.size()};
    std::vector<char> refit(h.plan_layout.bytes(), 0);
    if (n_triangles > 0) std::memcpy(&refit[PlanLayout::leaf_pos_at()], plan.leaf_pos.data(), (size_t)n_triangles * sizeof(int32_t));
    std::memcpy(&refit[h.plan_layout.levels_at()], plan.level_nodes.data(), plan.level_nodes.size() * sizeof(int32_t));
    h.level_first = std::move(plan.level_first);
    PTMI_HIP(c, hipStreamSynchronize(c->stream));
    // all blocks stand complete before the old scene goes
    k.alloc(k.packed, k.rows.bytes());
    k.alloc(k.spheres.block, k.spheres.layout.bytes());
    k.alloc(k.spheres.plan, plan_block.size());
    k.copy(k.spheres.plan.p, plan_block.data(), k.spheres.plan.bytes, hipMemcpyHostToDevice);
    k.alloc(h.block, h.layout.bytes());
    k.alloc(h.shadow, h.layout.bytes());
    k.alloc(h.plan, refit.size());
    k.copy(k.packed.p, packed.data(), k.packed.bytes, hipMemcpyHostToDevice);
    k.copy(k.spheres.block.p, hier.data(), k.spheres.block.bytes, hipMemcpyHostToDevice);
    k.copy(h.block.p, tri.data(), h.block.bytes, hipMemcpyHostToDevice);
    // (the second block starts as a copy: an update rewrites every record and every box of it, the references and indices never move)
    k.copy(h.shadow.p, h.block.p, h.block.bytes, hipMemcpyDeviceToDevice);
    k.copy(h.plan.p, refit.data(), h.plan.bytes, hipMemcpyHostToDevice);
    if (int rc = k.drain()) return rc;                     // the host vectors die at return
    commit(k);
    return PTMI_OK;
#endif
}

int ptmi_update_mesh_vertices_device(ptmi_ctx *c, const float *d_vertices, int n_triangles) { return update_mesh_vertices(c, d_vertices, n_triangles, false); }
int ptmi_update_mesh_vertices(ptmi_ctx *c, const float *vertices, int n_triangles) { return update_mesh_vertices(c, vertices, n_triangles, true); }

int ptmi_set_mesh_triangles_device(ptmi_ctx *c, const ptmi_triangle *d_triangles, int n_triangles)
{
    return set_mesh_triangles(c, reinterpret_cast<const float *>(d_triangles), n_triangles, false);
}
int ptmi_set_mesh_triangles(ptmi_ctx *c, const ptmi_triangle *triangles, int n_triangles)
{
    return set_mesh_triangles(c, reinterpret_cast<const float *>(triangles), n_triangles, true);
}

int ptmi_update_spheres_device(ptmi_ctx *c, const float *d_geometry, int n_spheres) { return update_spheres(c, d_geometry, n_spheres, false); }
int ptmi_update_spheres(ptmi_ctx *c, const float *geometry, int n_spheres) { return update_spheres(c, geometry, n_spheres, true); }

int ptmi_set_bvh_spheres_device(ptmi_ctx *c, const ptmi_sphere *d_spheres, int n_spheres)
{
    return set_bvh_spheres(c, reinterpret_cast<const float *>(d_spheres), n_spheres, false);
}
int ptmi_set_bvh_spheres(ptmi_ctx *c, const ptmi_sphere *spheres, int n_spheres)
{
    return set_bvh_spheres(c, reinterpret_cast<const float *>(spheres), n_spheres, true);
}

int ptmi_mesh_read_layout(ptmi_ctx *c, ptmi_bvh_node *nodes, int node_capacity, int32_t *order, int *n_kept)
{
    if (!c) return PTMI_EINVAL;
    std::lock_guard<std::mutex> lock(c->mu);
    if (c->scene.kind != SceneKind::Mesh) return fail(c, PTMI_ESTATE, "the current scene is not a mesh scene (ptmi_set_scene_mesh)");
    const size_t n_nodes = c->scene.triangles.layout.n_nodes, kept = c->scene.triangles.layout.kept;
    if (!nodes && !order) {                                  // the sizes only
        if (n_kept) *n_kept = (int)kept;
        return (int)n_nodes;
    }
    if (!nodes || (kept > 0 && !order)) return fail(c, PTMI_EINVAL, "bad layout arguments");
    if (node_capacity < 0 || (size_t)node_capacity < n_nodes) return fail(c, PTMI_ELIMIT, "node_capacity is smaller than the hierarchy");
    PTMI_HIP(c, hipSetDevice(c->device));
    CopySpan spans[2] = {{const_cast<float4 *>(c->scene.mesh.nodes), nodes, n_nodes * sizeof(ptmi_bvh_node)},
                         {const_cast<int *>(c->scene.mesh.index), order, kept * sizeof(int32_t)}};
    PTMI_HIP(c, copy_to_host(c, spans, 2));
    if (n_kept) *n_kept = (int)kept;
    return (int)n_nodes;
}

int ptmi_bvh_read_layout(ptmi_ctx *c, ptmi_bvh_node *nodes, int node_capacity, int32_t *order)
{
    if (!c) return PTMI_EINVAL;
    std::lock_guard<std::mutex> lock(c->mu);
    if (!c->scene.hierarchical()) return fail(c, PTMI_ESTATE, "the current scene is not a BVH or mesh scene (ptmi_set_scene_bvh, ptmi_set_scene_mesh)");
    const size_t n_nodes = c->scene.spheres.layout.n_nodes, ns = c->scene.spheres.layout.ns;
    if (!nodes && !order) return (int)n_nodes;               // the size only
    if (!nodes) return fail(c, PTMI_EINVAL, "bad layout arguments");
    if (node_capacity < 0 || (size_t)node_capacity < n_nodes) return fail(c, PTMI_ELIMIT, "node_capacity is smaller than the hierarchy");
    PTMI_HIP(c, hipSetDevice(c->device));
    CopySpan spans[2] = {{const_cast<float4 *>(c->scene.bvh.nodes), nodes, n_nodes * sizeof(ptmi_bvh_node)},
                         {const_cast<int *>(c->scene.bvh.index), order, order ? ns * sizeof(int32_t) : 0}};      // (no order: the nodes alone)
    PTMI_HIP(c, copy_to_host(c, spans, 2));
    return (int)n_nodes;
}

}  // extern "C"
