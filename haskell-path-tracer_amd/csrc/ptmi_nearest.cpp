// ptmi_nearest.cpp -- the nearest-primitive query of include/ptmi.h: ptmi_nearest_device / ptmi_nearest_indexed_device (argument checks and
// the launch of ptmi_nearest.hip's kernels) and ptmi_nearest, the host twin: the specification by enumeration, from ptmi_nearest.h's
// functions -- the definition the device is held to.
#include <algorithm>
#include <thread>

#include "ptmi_bvh.h"
#include "ptmi_ctx.h"
#include "ptmi_mesh.h"
#include "ptmi_nearest.h"

using namespace ptmi;

// The refusals of ptmi_trace_rays_multi_device (nothing enqueued, nothing written), then one launch on the context's stream -- no
// synchronisation, no allocation, no scratch.  The context's state planes, statistics and dispatch order are not touched.
static int nearest(ptmi_ctx *c, const float *d_points, const float *d_r_max, int n, const int32_t *d_index, int m, bool indexed, float *d_dist, int32_t *d_idx,
                   float *d_point)
{
    if (!c) return PTMI_EINVAL;
    std::lock_guard<std::mutex> lock(c->mu);
    if (n < 0 || (n > 0 && (!d_points || !d_dist || !d_idx)) || (indexed && (m < 0 || (m > 0 && !d_index))))
        return fail(c, PTMI_EINVAL, "bad nearest-primitive arguments");
    if (!c->scene.packed.p) return fail(c, PTMI_ESTATE, "ptmi_set_scene has not been called");
    if (n == 0 || (indexed && m == 0)) return PTMI_OK;
    PTMI_HIP(c, hipSetDevice(c->device));
    const RayCallScene r = ray_call_scene(c);
    PTMI_HIP(c, launch_nearest(r.scene, r.bvh, r.mesh, d_points, d_r_max, n, indexed ? d_index : nullptr, m, d_dist, d_idx, d_point, c->stream));
    return PTMI_OK;
}

extern "C" int ptmi_nearest_device(ptmi_ctx *c, const float *d_points, const float *d_r_max, int n, float *d_dist, int32_t *d_idx, float *d_point)
{
    return nearest(c, d_points, d_r_max, n, nullptr, 0, false, d_dist, d_idx, d_point);
}

extern "C" int ptmi_nearest_indexed_device(ptmi_ctx *c, const float *d_points, const float *d_r_max, int n, const int32_t *d_index, int m, float *d_dist,
                                           int32_t *d_idx, float *d_point)
{
    return nearest(c, d_points, d_r_max, n, d_index, m, true, d_dist, d_idx, d_point);
}

// ---- the host twin ----
namespace {

V3 v3(const float *v) { return mk(v[0], v[1], v[2]); }

// Point p's answer by enumeration: spheres, planes, then the triangles' records (12 floats each, mesh_build's; a NaN normal: zero area)
void nearest_one(const ptmi_sphere *s, int ns, const ptmi_plane *pl, int np, const float *records, int nt, V3 p, float lim, float *dist, int32_t *idx, float *point)
{
    float best_key = lim;
    int best = 0x7fffffff;
    Nearest won;
    won.s = 0.0f; won.at = mk(0.0f, 0.0f, 0.0f);
    auto take = [&](const Nearest &a, int j) {
        if (nearest_better(__builtin_fabsf(a.s), j, lim, best_key, best)) { best_key = __builtin_fabsf(a.s); best = j; won = a; }
    };
    if (lim > 0.0f) {
        for (int i = 0; i < ns; ++i) take(nearest_sphere(v3(s[i].position), s[i].radius * s[i].radius, p), i);
        for (int j = 0; j < np; ++j) take(nearest_plane(v3(pl[j].position), v3(pl[j].direction), p), ns + j);
        for (int k = 0; k < nt; ++k) {
            const float *r = records + 12 * (size_t)k;
            if (r[3] != r[3]) continue;
            take(nearest_triangle(v3(r), v3(r + 4), v3(r + 8), p), ns + np + k);
        }
    }
    const bool found = best != 0x7fffffff;
    *dist = won.s;
    *idx = found ? best : -1;
    if (point) { point[0] = won.at.x; point[1] = won.at.y; point[2] = won.at.z; }
}

}  // namespace

// What the scene calls refuse in the scene data, by their own checks: with triangles the scene can only be a mesh scene, and the twin runs
// what ptmi_set_scene_mesh runs over the data -- the counts' limits and the tags of refuse_hierarchy_scene, then bvh_build and mesh_build
// whole (non-finite geometry or triangle material, a leaf the depth limit cannot hold).  What that call refuses in the CONTEXT (a variant,
// a stream form, contracted arithmetic) has no counterpart here.  Without triangles it may be a linear scene, which takes its data as it
// comes -- a non-finite sphere or plane then has a NaN or inf key and is no candidate.
namespace {

template <class T> bool tags_known(const T *prims, int n)
{
    for (int i = 0; i < n; ++i)
        if (prims[i].brdf_tag < PTMI_MATTE || prims[i].brdf_tag > PTMI_GLASS) return false;
    return true;
}

}  // namespace

extern "C" int ptmi_nearest(const ptmi_sphere *spheres, int n_spheres, const ptmi_plane *planes, int n_planes, const ptmi_triangle *triangles, int n_triangles,
                            const float *points, const float *r_max, int n, float *dist, int32_t *idx, float *point)
{
    if (n_spheres < 0 || n_planes < 0 || n_triangles < 0 || (n_spheres > 0 && !spheres) || (n_planes > 0 && !planes) || (n_triangles > 0 && !triangles))
        return PTMI_EINVAL;
    if ((long long)n_spheres + n_planes + n_triangles == 0) return PTMI_EINVAL;          // an empty scene, as the scene calls refuse it
    if (n < 0 || (n > 0 && (!points || !dist || !idx))) return PTMI_EINVAL;
    MeshBuild mb;
    if (n_triangles > 0) {
        if (n_spheres > PTMI_MAX_BVH_SPHERES || n_planes > PTMI_MAX_BVH_PLANES || n_triangles > PTMI_MAX_MESH_TRIANGLES) return PTMI_ELIMIT;
        if (!tags_known(spheres, n_spheres) || !tags_known(planes, n_planes) || !tags_known(triangles, n_triangles)) return PTMI_EINVAL;
        BvhBuild bb;
        if (int rc = bvh_build(spheres, n_spheres, bb, nullptr)) return rc;
        if (int rc = mesh_build(triangles, n_triangles, mb, nullptr)) return rc;
    }
    const float *records = mb.records.data();
    auto run = [&](int from, int to) {
        for (int i = from; i < to; ++i)
            nearest_one(spheres, n_spheres, planes, n_planes, records, n_triangles, v3(points + 3 * (size_t)i), r_max ? r_max[i] : __builtin_inff(), dist + i, idx + i,
                        point ? point + 3 * (size_t)i : nullptr);
    };
    const long long work = (long long)n * ((long long)n_spheres + n_planes + n_triangles);
    const int workers = work < (1ll << 22) ? 1 : (int)std::min<long long>(std::max(1u, std::min(8u, std::thread::hardware_concurrency())), n);
    if (workers <= 1) { run(0, n); return PTMI_OK; }
    std::vector<std::thread> pool;
    for (int w = 0; w < workers; ++w) pool.emplace_back(run, (int)((long long)n * w / workers), (int)((long long)n * (w + 1) / workers));
    for (std::thread &t : pool) t.join();
    return PTMI_OK;
}
