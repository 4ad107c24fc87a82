/* multi_hit_traverse.c -- TEST-ONLY: ptmi_trace_rays_multi_device's k-bounded walk over the hierarchies (csrc/ptmi_multi_hit_device.h:
 * multi_hit_search over multi_hit_planes, multi_hit_spheres, multi_hit_triangles) on the CPU, in the style of any_hit_traverse.c: the
 * oracle's sphere and plane tests, the triangle test of triangle_test.h, the box tests and margins of traverse_slabs.h, the node format
 * ptmi_bvh_layout* / ptmi_mesh_layout* export, built with the oracle's flags.  tests/test_multi_hit_traversal.py holds its rows to the
 * specification (multi_hit_reference.c) without a GPU.  The lane's list is the ascending (t, idx) list of at most k; the bound is lim
 * until it is full and its last t from then on; a leaf inserts every primitive that qualifies and the walk never leaves early.  A ray
 * the admission test does not serve enumerates every primitive.  Per ray it reports whether it was served and the primitives of the
 * hierarchies it tested (spheres and triangles; the planes are always all tested).
 *
 * THE SWITCHES exist to show that the tests would notice a walk that is subtly wrong; the device has neither:
 *     widen    the factor on the slab margin m: 1 as the device, 0 the unwidened boxes
 *     strict   a child is entered at t_near < bound instead of t_near <= bound */
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "../../oracle/pt_oracle.h"
#include "../../include/ptmi.h"
#include "traverse_slabs.h"
#include "triangle_test.h"

#define K_MAX 64

typedef struct { float t[K_MAX]; int32_t j[K_MAX]; int k, held; float lim; } hit_list;

static float bound_of(const hit_list *L) { return L->held == L->k ? L->t[L->k - 1] : L->lim; }

static void insert(hit_list *L, int just, float t, int32_t j)
{
    if (!just || !(t < L->lim)) return;
    if (L->held == L->k) {
        const float lt = L->t[L->k - 1];
        if (!(t < lt || (t == lt && j < L->j[L->k - 1]))) return;
    }
    int at = L->held < L->k ? L->held++ : L->k - 1;
    while (at > 0 && (t < L->t[at - 1] || (t == L->t[at - 1] && j < L->j[at - 1]))) { L->t[at] = L->t[at - 1]; L->j[at] = L->j[at - 1]; --at; }
    L->t[at] = t; L->j[at] = j;
}

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

/* bvh_walk with the bound at the list's last slot, over either hierarchy: sphere != 0 walks spheres s through (nodes, order) with the
 * sphere margin, else the triangle records tr (first: the index of triangle 0) with the mesh margin.  The farther child is held to the
 * bound again after the nearer one's leaf.  Returns -2 where the device's stack would overflow. */
static int walk(const ptmi_bvh_node *nodes, const int32_t *order, int sphere, const ora_sphere *s, const trec *tr, int32_t first, ora_ray r, float eta,
                hit_list *L, float widen, int strict, int64_t *tests)
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
            const int in_box = sphere ? sphere_child_slab(nd, c, o, inv, G, G_lin, sqrt_G, widen, &tn[c])
                                      : mesh_child_slab(nd, c, o, inv, ainv, o1, widen, &tn[c]);
            const float b = bound_of(L);
            h[c] = in_box && nd->ref[c] != -1 && (strict ? tn[c] < b : tn[c] <= b);
        }
        const int swap = h[1] && (!h[0] || tn[1] < tn[0]);           /* the nearer child first */
        const int32_t ra = swap ? nd->ref[1] : nd->ref[0], rb = swap ? nd->ref[0] : nd->ref[1];
        const int ha = swap ? h[1] : h[0], hb = swap ? h[0] : h[1];
        const float tb = swap ? tn[0] : tn[1];
        int next = -1;
        for (int pass = 0; pass < 2; ++pass) {
            const int32_t ref = pass ? rb : ra;
            if (!(pass ? hb : ha)) continue;
            if (pass) { const float b = bound_of(L); if (!(strict ? tb < b : tb <= b)) continue; }      /* the bound may have moved */
            if (ref >= 0) {
                if (next < 0) next = ref;
                else { if (sp >= PTMI_BVH_MAX_DEPTH) return -2; stack[sp++] = ref; }
                continue;
            }
            const uint32_t v = (uint32_t)(-1 - ref);
            for (uint32_t k = 0; k < (v & 255u); ++k) {
                const int32_t i = order[(v >> 8) + k];
                float t;
                int just;
                if (sphere) { const ora_maybe_float q = ora_distance_to_sphere(r, &s[i]); just = q.is_just; t = q.value; }
                else just = tri_test(&tr[i], ov, dv, &t);
                ++*tests;
                insert(L, just, t, first + i);
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

/* multi_hit_search for a BVH scene (is_mesh == 0) and a mesh scene: the sphere hierarchy (snodes, sorder) in the box (slo, shi), the
 * triangle hierarchy (tnodes, torder, n_kept of the nt records recs) in the box (tlo, thi).  t_max: n words or NULL.  1 <= k <= 64.
 * Returns the rays whose walk would overflow the device's stack. */
int multi_hit_hierarchy(const ptmi_bvh_node *snodes, const int32_t *sorder, const float *slo, const float *shi,
                        const ptmi_bvh_node *tnodes, const int32_t *torder, int n_kept, const float *tlo, const float *thi,
                        const ora_sphere *s, int ns, const ora_plane *p, int np, const float *recs, int nt, int is_mesh,
                        const float *rays, const float *t_max, int n, int k, float widen, int strict,
                        float *t_out, int32_t *idx_out, int32_t *count_out, int32_t *served_out, int32_t *tests_out)
{
    const trec *tr = (const trec *)recs;
    int overflow = 0;
#pragma omp parallel for schedule(dynamic, 64) reduction(+ : overflow)
    for (int i = 0; i < n; ++i) {
        const float *o = rays + 6 * (size_t)i, *d = o + 3;
        ora_ray r;
        r.origin.x = o[0]; r.origin.y = o[1]; r.origin.z = o[2];
        r.direction.x = d[0]; r.direction.y = d[1]; r.direction.z = d[2];
        const v3 ov = mk(o[0], o[1], o[2]), dv = mk(d[0], d[1], d[2]);
        hit_list L;
        L.k = k; L.held = 0; L.lim = t_max ? t_max[i] : INFINITY;
        const float eta = eta_of(d);
        const float P = is_mesh ? fmaxf(reach_of(slo, shi, o), reach_of(tlo, thi, o)) : reach_of(slo, shi, o);
        const int served = finite_ray(o, d) && eta <= 0x1p-12f && P <= 0x1p40f;
        int64_t tests = 0;
        int over = 0;
        if (L.lim > 0.0f) {
            if (served) {
                for (int j = 0; j < np; ++j) { const ora_maybe_float q = ora_distance_to_plane(r, &p[j]); insert(&L, q.is_just, q.value, ns + j); }
                if (ns > 0) over |= walk(snodes, sorder, 1, s, NULL, 0, r, eta, &L, widen, strict, &tests);
                if (is_mesh && n_kept > 0) over |= walk(tnodes, torder, 0, NULL, tr, ns + np, r, eta, &L, widen, strict, &tests);
            } else {
                for (int j = 0; j < ns; ++j) { const ora_maybe_float q = ora_distance_to_sphere(r, &s[j]); insert(&L, q.is_just, q.value, j); }
                for (int j = 0; j < np; ++j) { const ora_maybe_float q = ora_distance_to_plane(r, &p[j]); insert(&L, q.is_just, q.value, ns + j); }
                for (int j = 0; is_mesh && j < nt; ++j) { float t; const int just = tri_test(&tr[j], ov, dv, &t); insert(&L, just, t, ns + np + j); }
            }
        }
        if (over) ++overflow;
        for (int c = 0; c < k; ++c) {
            t_out[(size_t)i * k + c] = c < L.held ? L.t[c] : 0.0f;
            idx_out[(size_t)i * k + c] = c < L.held ? L.j[c] : -1;
        }
        count_out[i] = L.held; served_out[i] = served; tests_out[i] = (int32_t)tests;
    }
    return overflow;
}
