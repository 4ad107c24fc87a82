/* any_hit_traverse.c -- TEST-ONLY: ptmi_occluded_device's any-hit walks (csrc/ptmi_query_device.h: occluded_linear, occluded_bvh,
 * occluded_mesh over any_hit_planes, any_hit_spheres_linear, any_hit_spheres, any_hit_triangles) on the CPU, with the conventions of
 * bvh_traverse.c and mesh_traverse.c: the oracle's sphere and plane tests, the triangle test of triangle_test.h, the box tests and
 * margins of traverse_slabs.h (the files those two walks use), the node format ptmi_bvh_layout* / ptmi_mesh_layout* export, built with
 * the oracle's flags (no contraction, no fast-math).  tests/test_any_hit_traversal.py holds its answers to the specification
 *     occluded = h.just && h.t < t_max,   h the literal fold's closest hit
 * without a GPU.  Per ray it reports
 *     answer   0 or 1
 *     path     how the answer came about (ANY_* below)
 *     tests    the primitives of the hierarchy tested (spheres of a linear or BVH scene, triangles of a mesh scene); a ray that takes
 *              the full search after a walk is charged every primitive on top
 * THE FULL SEARCH is the literal fold here: bvh_traverse.c and mesh_traverse.c show the closest-hit walks equal to it.
 *
 * THE SWITCHES (struct any_knobs) exist to show that the tests would notice a walk that is subtly wrong; the device has neither:
 *     widen    the factor on the slab margin m: 1 as the device, 0 the unwidened boxes, 0.5 a margin half as large
 *     strict   a child is entered at t_near < lim instead of t_near <= lim */
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "../../oracle/pt_oracle.h"
#include "../../include/ptmi.h"
#include "traverse_slabs.h"
#include "triangle_test.h"

#define INF_KEY 3.40282346638528859812e+38f

enum { ANY_NOT_SERVED = 0,      /* the admission test sent the ray to the full search */
       ANY_EARLY = 1,           /* left at an occluder */
       ANY_TO_THE_END = 2,      /* walked everything the bound let it and met none */
       ANY_FULL_BY_KEY = 3,     /* a Just key not below FLT_MAX sent it to the full search */
       ANY_NO_LIMIT = 4 };      /* !(t_max > 0): answered 0 before any search */

enum { kAnyNone = 0, kAnyHit = 1, kAnyFull = 2 };

typedef struct { float widen; int strict; } any_knobs;
typedef struct { float t; int just; } closest;

static ora_ray ray_of(const float *q)
{
    ora_ray r;
    r.origin.x = q[0]; r.origin.y = q[1]; r.origin.z = q[2];
    r.direction.x = q[3]; r.direction.y = q[4]; r.direction.z = q[5];
    return r;
}

/* the literal fold over spheres ++ planes ++ triangles (bvh_traverse.c: fold; mesh_traverse.c: fold_all), the hit's t and Just only */
static closest fold_all(const ora_sphere *s, int ns, const ora_plane *p, int np, const trec *tr, int nt, ora_ray r)
{
    float acc_key = 0.0f, acc_t = 0.0f;
    int acc_just = 0;
    for (int i = 0; i < ns + np; ++i) {
        const ora_maybe_float d = i < ns ? ora_distance_to_sphere(r, &s[i]) : ora_distance_to_plane(r, &p[i - ns]);
        const float key = d.is_just ? d.value : INF_KEY;
        if (i == 0 || !(acc_key <= key)) { acc_key = key; acc_t = d.value; acc_just = d.is_just; }
    }
    const v3 o = mk(r.origin.x, r.origin.y, r.origin.z), d = mk(r.direction.x, r.direction.y, r.direction.z);
    for (int k = 0; k < nt; ++k) {
        float t;
        const int just = tri_test(&tr[k], o, d, &t);
        const float key = just ? t : INF_KEY;
        if ((ns + np == 0 && k == 0) || !(acc_key <= key)) { acc_key = key; acc_t = t; acc_just = just; }
    }
    const closest h = {acc_t, acc_just};
    return h;
}

static int occluded_by(closest h, float t_max) { return h.just && h.t < t_max; }

/* any_hit_key: one Just key against the limit */
static int key_of(int just, float t, float lim)
{
    if (!just) return kAnyNone;
    if (!(t < INF_KEY)) return kAnyFull;
    return t < lim ? kAnyHit : kAnyNone;
}

/* any_hit_planes: all of them, kAnyFull outranks kAnyHit (a non-candidate is a Nothing of ora_distance_to_plane) */
static int planes_of(const ora_plane *p, int np, ora_ray r, float lim)
{
    int found = kAnyNone;
    for (int j = 0; j < np; ++j) {
        const ora_maybe_float q = ora_distance_to_plane(r, &p[j]);
        const int k = key_of(q.is_just, q.value, lim);
        found = k > found ? k : found;
    }
    return found;
}

/* bvh_eta, bvh_reach, bvh_ray_finite */
static float eta_of(const float d[3]) { return fabsf(((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]) - 1.0f); }
static float reach_of(const float lo[3], const float hi[3], const float o[3])
{
    float P2 = 0.0f;
    for (int a = 0; a < 3; ++a) {
        const float pa = fmaxf(fabsf(lo[a] - o[a]), fabsf(hi[a] - o[a]));
        P2 = P2 + pa * pa;
    }
    return sqrtf(P2) * (1.0f + 0x1p-20f);
}
static int finite_ray(const float o[3], const float d[3])
{
    int finite = 1;
    for (int a = 0; a < 3; ++a) finite &= isfinite(o[a]) && isfinite(d[a]);
    return finite;
}

/* bvh_walk with the bound held at lim, over either hierarchy: sphere != 0 walks spheres s through (nodes, order) with the sphere
 * margin, else the triangle records tr with the mesh margin.  Returns kAny*, -2 where the device's stack would overflow. */
static int walk(const ptmi_bvh_node *nodes, const int32_t *order, int sphere, const ora_sphere *s, const trec *tr, ora_ray r, float eta,
                float lim, any_knobs K, int64_t *tests)
{
    const float o[3] = {r.origin.x, r.origin.y, r.origin.z}, d[3] = {r.direction.x, r.direction.y, r.direction.z};
    const v3 ov = mk(o[0], o[1], o[2]), dv = mk(d[0], d[1], d[2]);
    const float G = 0x1p-19f + 2.0f * eta, G_lin = G + 0x1p-19f, sqrt_G = sqrtf(G);
    const float inv[3] = {inv_of(d[0]), inv_of(d[1]), inv_of(d[2])};
    const float ainv[3] = {fabsf(inv[0]), fabsf(inv[1]), fabsf(inv[2])};
    const float o1 = (fabsf(o[0]) + fabsf(o[1])) + fabsf(o[2]);
    int stack[PTMI_BVH_MAX_DEPTH], sp = 0, node = 0;
    for (;;) {
        const ptmi_bvh_node *nd = &nodes[node];
        float tn[2];
        int h[2];
        for (int c = 0; c < 2; ++c) {
            const int in_box = sphere ? sphere_child_slab(nd, c, o, inv, G, G_lin, sqrt_G, K.widen, &tn[c])
                                      : mesh_child_slab(nd, c, o, inv, ainv, o1, K.widen, &tn[c]);
            h[c] = in_box && nd->ref[c] != -1 && (K.strict ? tn[c] < lim : tn[c] <= lim);
        }
        const int swap = h[1] && (!h[0] || tn[1] < tn[0]);           /* the nearer child first */
        const int32_t ra = swap ? nd->ref[1] : nd->ref[0], rb = swap ? nd->ref[0] : nd->ref[1];
        const int ha = swap ? h[1] : h[0], hb = swap ? h[0] : h[1];
        int next = -1;
        for (int pass = 0; pass < 2; ++pass) {
            const int32_t ref = pass ? rb : ra;
            if (!(pass ? hb : ha)) continue;                         /* (the bound does not move: hb needs no second look) */
            if (ref >= 0) {
                if (next < 0) next = ref;
                else { if (sp >= PTMI_BVH_MAX_DEPTH) return -2; stack[sp++] = ref; }
                continue;
            }
            const uint32_t v = (uint32_t)(-1 - ref);
            for (uint32_t k = 0; k < (v & 255u); ++k) {              /* the leaf: left at the first primitive that answers */
                const int32_t i = order[(v >> 8) + k];
                float t;
                int just;
                if (sphere) { const ora_maybe_float q = ora_distance_to_sphere(r, &s[i]); just = q.is_just; t = q.value; }
                else just = tri_test(&tr[i], ov, dv, &t);
                ++*tests;
                const int found = key_of(just, t, lim);
                if (found != kAnyNone) return found;
            }
        }
        if (next < 0) {
            if (sp == 0) break;
            next = stack[--sp];
        }
        node = next;
    }
    return kAnyNone;
}

static int path_of(int found) { return found == kAnyHit ? ANY_EARLY : found == kAnyNone ? ANY_TO_THE_END : ANY_FULL_BY_KEY; }

/* SceneState.sphere_reach (csrc/ptmi_scene.cpp: sphere_reach_of): the largest |centre component| or r * r, +inf when one is not finite */
float any_sphere_reach(const ora_sphere *s, int ns)
{
    float reach = 0.0f;
    for (int i = 0; i < ns; ++i) {
        const float row[4] = {s[i].position[0], s[i].position[1], s[i].position[2], s[i].radius * s[i].radius};
        for (int k = 0; k < 4; ++k) reach = isfinite(row[k]) ? fmaxf(reach, fabsf(row[k])) : INFINITY;
    }
    return reach;
}

/* occluded_linear */
void any_linear(const ora_sphere *s, int ns, const ora_plane *p, int np, const float *rays, const float *t_max, int n,
                int32_t *answer, int32_t *path, int32_t *tests)
{
    const float reach = any_sphere_reach(s, ns);
#pragma omp parallel for schedule(dynamic, 256)
    for (int i = 0; i < n; ++i) {
        const ora_ray r = ray_of(rays + 6 * (size_t)i);
        const float *o = rays + 6 * (size_t)i, *d = o + 3;
        const float lim = fminf(t_max[i], INF_KEY);
        const float oo = fmaxf(fmaxf(fabsf(o[0]), fabsf(o[1])), fabsf(o[2]));
        int64_t made = 0;
        answer[i] = 0; tests[i] = 0;
        if (!(finite_ray(o, d) && eta_of(d) <= 0x1p-12f && oo <= 0x1p40f && reach <= 0x1p40f)) {
            path[i] = ANY_NOT_SERVED;
            answer[i] = t_max[i] > 0.0f && occluded_by(fold_all(s, ns, p, np, NULL, 0, r), t_max[i]);
            continue;
        }
        if (!(t_max[i] > 0.0f)) { path[i] = ANY_NO_LIMIT; continue; }
        int found = planes_of(p, np, r, lim);
        for (int k = 0; k < ns && found == kAnyNone; ++k) {           /* any_hit_spheres_linear: in index order */
            const ora_maybe_float q = ora_distance_to_sphere(r, &s[k]);
            ++made;
            found = key_of(q.is_just, q.value, lim);
        }
        path[i] = path_of(found);
        if (found == kAnyFull) { answer[i] = occluded_by(fold_all(s, ns, p, np, NULL, 0, r), t_max[i]); made += ns; }
        else answer[i] = found == kAnyHit;
        tests[i] = (int32_t)made;
    }
}

/* occluded_bvh (tr == NULL) and occluded_mesh: the sphere hierarchy (snodes, sorder) in the box (slo, shi), the triangle hierarchy
 * (tnodes, torder, n_kept of the nt records tr) in the box (tlo, thi).  Returns the rays whose walk would overflow the device's stack. */
int any_hierarchy(const ptmi_bvh_node *snodes, const int32_t *sorder, const float *slo, const float *shi,
                  const ptmi_bvh_node *tnodes, const int32_t *torder, int n_kept, const float *tlo, const float *thi,
                  const ora_sphere *s, int ns, const ora_plane *p, int np, const float *recs, int nt, int is_mesh,
                  const float *rays, const float *t_max, int n, float widen, int strict, int32_t *answer, int32_t *path, int32_t *tests)
{
    const trec *tr = (const trec *)recs;
    const any_knobs K = {widen, strict};
    int overflow = 0;
#pragma omp parallel for schedule(dynamic, 256) reduction(+ : overflow)
    for (int i = 0; i < n; ++i) {
        const ora_ray r = ray_of(rays + 6 * (size_t)i);
        const float *o = rays + 6 * (size_t)i, *d = o + 3;
        const float lim = fminf(t_max[i], INF_KEY), eta = eta_of(d);
        const float P = is_mesh ? fmaxf(reach_of(slo, shi, o), reach_of(tlo, thi, o)) : reach_of(slo, shi, o);
        int64_t sphere_tests = 0, triangle_tests = 0;
        answer[i] = 0; tests[i] = 0;
        if (!(finite_ray(o, d) && eta <= 0x1p-12f && P <= 0x1p40f)) {
            path[i] = ANY_NOT_SERVED;
            answer[i] = t_max[i] > 0.0f && occluded_by(fold_all(s, ns, p, np, tr, nt, r), t_max[i]);
            continue;
        }
        if (!(t_max[i] > 0.0f)) { path[i] = ANY_NO_LIMIT; continue; }
        int found = planes_of(p, np, r, lim);
        if (found == kAnyNone && ns > 0) found = walk(snodes, sorder, 1, s, NULL, r, eta, lim, K, &sphere_tests);
        if (is_mesh && found == kAnyNone && n_kept > 0) found = walk(tnodes, torder, 0, NULL, tr, r, eta, lim, K, &triangle_tests);
        if (found == -2) { ++overflow; path[i] = -2; continue; }
        path[i] = path_of(found);
        int64_t made = is_mesh ? triangle_tests : sphere_tests;
        if (found == kAnyFull) { answer[i] = occluded_by(fold_all(s, ns, p, np, tr, nt, r), t_max[i]); made += is_mesh ? nt : ns; }
        else answer[i] = found == kAnyHit;
        tests[i] = (int32_t)made;
    }
    return overflow;
}
