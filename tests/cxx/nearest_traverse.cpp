/* nearest_traverse.cpp -- TEST-ONLY: the nearest-primitive query's walk over the hierarchies (csrc/ptmi_nearest_device.h: nearest_search
 * over nearest_planes, nearest_spheres, nearest_triangles) on the CPU.  It INCLUDES csrc/ptmi_nearest.h -- the primitives' distances and
 * the box bound are the library's own functions, not a restatement -- and restates only the walk: bvh_walk's loop over the node format
 * ptmi_bvh_layout* / ptmi_mesh_layout* export, the admission rule, the order planes, spheres, triangles.  tests/test_nearest_traversal.py
 * holds its answers to the host twin (ptmi_nearest) bit for bit without a GPU.  Per point it reports whether the walk served it and how
 * many primitives of the hierarchies it tested (spheres and triangles; the planes are always all tested).
 *
 * THE SWITCH exists to show what the margin is for; the device has none:
 *     margin   nearest_box_bound's factor on p1: kNearestMargin as the device, 0 the distance to the box as computed */
#include <math.h>
#include <stdint.h>

#include <thread>
#include <vector>

#include "../../haskell-path-tracer_amd/csrc/ptmi_mesh_box.h"
#include "../../haskell-path-tracer_amd/csrc/ptmi_nearest.h"
#include "../../include/ptmi.h"

using namespace ptmi;

namespace {

struct Best { float key; int idx; };

V3 v3(const float *v) { return mk(v[0], v[1], v[2]); }

void take(Best &b, float s, int j, float lim)
{
    const float key = fabsf(s);
    if (nearest_better(key, j, lim, b.key, b.idx)) { b.key = key; b.idx = j; }
}

float reach_of(const float lo[3], const float hi[3], const float o[3])
{
    float P2 = 0.0f;
    for (int a = 0; a < 3; ++a) {
        const float pa = fmaxf(fabsf(lo[a] - o[a]), fabsf(hi[a] - o[a]));
        P2 = P2 + pa * pa;
    }
    return sqrtf(P2) * (1.0f + 0x1p-20f);
}

Nearest sphere_of(const ptmi_sphere &s, V3 p) { return nearest_sphere(v3(s.position), s.radius * s.radius, p); }
Nearest triangle_of(const float *r, V3 p) { return nearest_triangle(v3(r), v3(r + 4), v3(r + 8), p); }

/* bvh_walk with the bound at the best key, over either hierarchy: s != NULL walks the spheres through (nodes, order), else the triangle
 * records (first: the index of triangle 0).  The farther child is held to the bound again after the nearer one's leaf.  Returns -2 where
 * the device's stack would overflow. */
int walk(const ptmi_bvh_node *nodes, const int32_t *order, const ptmi_sphere *s, const float *recs, int32_t first, V3 p, float lim, float margin, Best &b,
         int64_t *tests)
{
    int stack[PTMI_BVH_MAX_DEPTH], sp = 0, node = 0;
    for (;;) {
        const ptmi_bvh_node *nd = &nodes[node];
        float lb[2];
        int h[2];
        for (int c = 0; c < 2; ++c) {
            lb[c] = nearest_box_bound(v3(nd->center[c]), v3(nd->half[c]), p, margin);
            h[c] = nd->ref[c] != -1 && lb[c] <= b.key;
        }
        const int swap = h[1] && (!h[0] || lb[1] < lb[0]);           /* the nearer child first */
        const int32_t ra = swap ? nd->ref[1] : nd->ref[0], rb = swap ? nd->ref[0] : nd->ref[1];
        const int ha = swap ? h[1] : h[0], hb = swap ? h[0] : h[1];
        const float tb = swap ? lb[0] : lb[1];
        int next = -1;
        for (int pass = 0; pass < 2; ++pass) {
            const int32_t ref = pass ? rb : ra;
            if (!(pass ? hb : ha)) continue;
            if (pass && !(tb <= b.key)) continue;                    /* the bound may have moved */
            if (ref >= 0) {
                if (next < 0) next = ref;
                else { if (sp >= PTMI_BVH_MAX_DEPTH) return -2; stack[sp++] = ref; }
                continue;
            }
            const uint32_t v = (uint32_t)(-1 - ref);
            for (uint32_t k = 0; k < (v & 255u); ++k) {
                const int32_t i = order[(v >> 8) + k];
                if (!s && recs[12 * (size_t)i + 3] != recs[12 * (size_t)i + 3]) continue;      /* collapsed by a refit: in its leaf, no candidate */
                take(b, s ? sphere_of(s[i], p).s : triangle_of(recs + 12 * (size_t)i, p).s, first + i, lim);
                ++*tests;
            }
        }
        if (next < 0) {
            if (sp == 0) break;
            next = stack[--sp];
        }
        node = next;
    }
    return 0;
}

}  // namespace

/* The records mesh_build derives (ptmi_mesh.cpp), from ptmi_mesh_box.h's triangle_normal: (v0, nx) (v1, ny) (v2, nz), a NaN normal for zero area */
extern "C" void nearest_records(const ptmi_triangle *t, int n, float *out)
{
    for (int i = 0; i < n; ++i) {
        const TriangleNormal tn = triangle_normal(t[i].v0, t[i].v1, t[i].v2);
        float *r = out + 12 * (size_t)i;
        const float *v[3] = {t[i].v0, t[i].v1, t[i].v2};
        for (int k = 0; k < 3; ++k) { r[4 * k] = v[k][0]; r[4 * k + 1] = v[k][1]; r[4 * k + 2] = v[k][2]; }
        if (!(tn.nn > 0.0f)) { r[3] = r[7] = r[11] = NAN; continue; }
        const float len = sqrtf(tn.nn);
        r[3] = tn.n[0] / len; r[7] = tn.n[1] / len; r[11] = tn.n[2] / len;
    }
}

/* nearest_search for a BVH scene (is_mesh == 0) and a mesh scene: the sphere hierarchy (snodes, sorder) in the box (slo, shi) of the
 * centres, the triangle hierarchy (tnodes, torder, n_kept of the nt records recs) in the box (tlo, thi) of the kept vertices.  r_max: n
 * words or NULL.  Returns the points whose walk would overflow the device's stack. */
extern "C" int nearest_hierarchy(const ptmi_bvh_node *snodes, const int32_t *sorder, const float *slo, const float *shi, const ptmi_bvh_node *tnodes,
                                 const int32_t *torder, int n_kept, const float *tlo, const float *thi, const ptmi_sphere *s, int ns, const ptmi_plane *pl, int np,
                                 const float *recs, int nt, int is_mesh, const float *points, const float *r_max, int n, float margin, float *dist_out,
                                 int32_t *idx_out, float *point_out, int32_t *served_out, int32_t *tests_out)
{
    std::vector<int> overflow(n > 0 ? n : 0, 0);
    auto run = [&](int from, int to) {
        for (int i = from; i < to; ++i) {
            const float *o = points + 3 * (size_t)i;
            const V3 p = v3(o);
            const float lim = r_max ? r_max[i] : INFINITY;
            Best b;
            b.key = lim; b.idx = 0x7fffffff;
            const float P = is_mesh ? fmaxf(reach_of(slo, shi, o), reach_of(tlo, thi, o)) : reach_of(slo, shi, o);
            const int served = isfinite(o[0]) && isfinite(o[1]) && isfinite(o[2]) && P <= 0x1p40f;
            int64_t tests = 0;
            int over = 0;
            if (lim > 0.0f) {
                if (served) {
                    for (int j = 0; j < np; ++j) take(b, nearest_plane(v3(pl[j].position), v3(pl[j].direction), p).s, ns + j, lim);
                    if (ns > 0) over |= walk(snodes, sorder, s, nullptr, 0, p, lim, margin, b, &tests);
                    if (is_mesh && n_kept > 0) over |= walk(tnodes, torder, nullptr, recs, ns + np, p, lim, margin, b, &tests);
                } else {
                    for (int j = 0; j < ns; ++j) take(b, sphere_of(s[j], p).s, j, lim);
                    for (int j = 0; j < np; ++j) take(b, nearest_plane(v3(pl[j].position), v3(pl[j].direction), p).s, ns + j, lim);
                    for (int j = 0; is_mesh && j < nt; ++j) {
                        const float *r = recs + 12 * (size_t)j;
                        if (r[3] != r[3]) continue;
                        take(b, triangle_of(r, p).s, ns + np + j, lim);
                    }
                }
            }
            overflow[i] = over != 0;
            const bool found = b.idx != 0x7fffffff;
            Nearest a;
            a.s = 0.0f; a.at = mk(0.0f, 0.0f, 0.0f);
            if (found) {
                if (b.idx < ns) a = sphere_of(s[b.idx], p);
                else if (b.idx < ns + np) a = nearest_plane(v3(pl[b.idx - ns].position), v3(pl[b.idx - ns].direction), p);
                else a = triangle_of(recs + 12 * (size_t)(b.idx - ns - np), p);
            }
            dist_out[i] = a.s; idx_out[i] = found ? b.idx : -1;
            point_out[3 * (size_t)i] = a.at.x; point_out[3 * (size_t)i + 1] = a.at.y; point_out[3 * (size_t)i + 2] = a.at.z;
            served_out[i] = served; tests_out[i] = (int32_t)tests;
        }
    };
    const int workers = n < 256 ? 1 : 8;
    std::vector<std::thread> pool;
    for (int w = 0; w < workers; ++w) pool.emplace_back(run, (int)((long long)n * w / workers), (int)((long long)n * (w + 1) / workers));
    for (std::thread &t : pool) t.join();
    int total = 0;
    for (int v : overflow) total += v;
    return total;
}
