/* bvh_traverse.c -- TEST-ONLY: checkHit through the hierarchy ptmi_bvh_layout exports, on the CPU, with the oracle's sphere test
 * (ora_distance_to_sphere, whose arithmetic the device's sphere test matches).  It walks the layout the way check_hit_bvh
 * (csrc/ptmi_bvh_device.h) does -- the same admission of a ray, the same per-ray margin, the same slab test, the same pruning against
 * the best key -- so that tests/test_bvh_traversal.py can show, without a GPU, that the padding and the pruning never lose the hit
 * the linear fold (ora_check_hit) finds.  Built by that test with the oracle's flags (no contraction, no fast-math).
 * Also the linear fold itself with the index kept (ora_check_hit returns the hit record only).  The box test is traverse_slabs.h's, which
 * any_hit_traverse.c (the occlusion walks) shares. */
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "../../oracle/pt_oracle.h"
#include "../../include/ptmi.h"
#include "traverse_slabs.h"

#define INF_KEY 3.40282346638528859812e+38f    /* kInfinite: maybe infinite fst (Trace.hs:450-451) */

typedef struct { float t; int idx; int just; } sel;

/* the literal fold of ora_check_hit, keeping the index; a miss is reported as (0, -1, 0) */
static sel fold(const ora_sphere *s, int ns, const ora_plane *p, int np, ora_ray r)
{
    sel acc = {0.0f, 0, 0};
    float acc_key = 0.0f;
    for (int i = 0; i < ns + np; ++i) {
        const ora_maybe_float d = i < ns ? ora_distance_to_sphere(r, &s[i]) : ora_distance_to_plane(r, &p[i - ns]);
        const float key = d.is_just ? d.value : INF_KEY;
        if (i == 0 || !(acc_key <= key)) { acc_key = key; acc.t = d.value; acc.idx = i; acc.just = d.is_just; }
    }
    if (!acc.just) { acc.t = 0.0f; acc.idx = -1; }
    return acc;
}

static ora_ray ray_of(const float *q)
{
    ora_ray r;
    r.origin.x = q[0]; r.origin.y = q[1]; r.origin.z = q[2];
    r.direction.x = q[3]; r.direction.y = q[4]; r.direction.z = q[5];
    return r;
}

void lin_check_hit(const ora_sphere *s, int ns, const ora_plane *p, int np, const float *rays, int n, float *t, int32_t *idx, int32_t *just)
{
#pragma omp parallel for schedule(dynamic, 256)
    for (int i = 0; i < n; ++i) {
        const sel h = fold(s, ns, p, np, ray_of(rays + 6 * (size_t)i));
        t[i] = h.t; idx[i] = h.idx; just[i] = h.just;
    }
}

static sel bvh_one(const ptmi_bvh_node *nodes, const int32_t *order, const float lo[3], const float hi[3],
                   const ora_sphere *s, int ns, const ora_plane *p, int np, ora_ray r, int64_t *tests)
{
    const float o[3] = {r.origin.x, r.origin.y, r.origin.z}, d[3] = {r.direction.x, r.direction.y, r.direction.z};
    const float eta = fabsf(((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]) - 1.0f);
    float P2 = 0.0f;
    for (int a = 0; a < 3; ++a) {
        const float pa = fmaxf(fabsf(lo[a] - o[a]), fabsf(hi[a] - o[a]));
        P2 = P2 + pa * pa;
    }
    const float P = sqrtf(P2) * (1.0f + 0x1p-20f);
    int finite = 1;
    for (int a = 0; a < 3; ++a) finite &= isfinite(o[a]) && isfinite(d[a]);
    if (!(finite && eta <= 0x1p-12f && P <= 0x1p40f)) { *tests += ns; return fold(s, ns, p, np, r); }

    float best_key = INF_KEY;
    int best_idx = 0x7fffffff, best_just = 0;
    if (ns > 0) {
        const float G = 0x1p-19f + 2.0f * eta, G_lin = G + 0x1p-19f, sqrt_G = sqrtf(G);
        const float inv[3] = {inv_of(d[0]), inv_of(d[1]), inv_of(d[2])};
        int stack[PTMI_BVH_MAX_DEPTH];
        int node = 0, sp = 0;
        for (;;) {
            const ptmi_bvh_node *nd = &nodes[node];
            float tn[2];
            int h[2];
            for (int c = 0; c < 2; ++c) {
                float t_near;
                const int in_box = sphere_child_slab(nd, c, o, inv, G, G_lin, sqrt_G, 1.0f, &t_near);      /* traverse_slabs.h */
                tn[c] = t_near;
                h[c] = in_box && nd->ref[c] != -1 && t_near <= best_key;
            }
            const int sw = h[1] && (!h[0] || tn[1] < tn[0]);
            const int ra = sw ? nd->ref[1] : nd->ref[0], rb = sw ? nd->ref[0] : nd->ref[1];
            const int ha = sw ? h[1] : h[0], hb = sw ? h[0] : h[1];
            const float tb = sw ? tn[0] : tn[1];
            int next = -1;
            for (int pass = 0; pass < 2; ++pass) {
                const int ref = pass == 0 ? ra : rb;
                if (!(pass == 0 ? ha : (hb && tb <= best_key))) continue;
                if (ref < 0) {
                    const uint32_t v = (uint32_t)(-1 - ref);
                    for (uint32_t k = 0; k < (v & 255u); ++k) {
                        const int i = order[(v >> 8) + k];
                        const ora_maybe_float q = ora_distance_to_sphere(r, &s[i]);
                        ++*tests;
                        if (q.is_just && (q.value < best_key || (q.value == best_key && i < best_idx))) { best_key = q.value; best_idx = i; best_just = 1; }
                    }
                } else if (next < 0) {
                    next = ref;
                } else {
                    if (sp >= PTMI_BVH_MAX_DEPTH) return (sel){0.0f, -2, -2};      /* the device's stack would overflow: reported */
                    stack[sp++] = ref;
                }
            }
            if (next < 0) {
                if (sp == 0) break;
                next = stack[--sp];
            }
            node = next;
        }
    }
    if (!best_just) { best_key = NAN; best_idx = 0; }
    for (int j = 0; j < np; ++j) {
        const ora_maybe_float q = ora_distance_to_plane(r, &p[j]);
        const float key = q.is_just ? q.value : INF_KEY;
        if (!(best_key <= key)) { best_key = key; best_idx = ns + j; best_just = q.is_just; }
    }
    if (best_just && !(best_key < INF_KEY)) return fold(s, ns, p, np, r);
    sel out = {best_key, best_idx, best_just};
    if (!out.just) { out.t = 0.0f; out.idx = -1; }
    return out;
}

/* returns the sphere tests made */
int64_t bvh_check_hit(const ptmi_bvh_node *nodes, const int32_t *order, const float *lo, const float *hi,
                      const ora_sphere *s, int ns, const ora_plane *p, int np, const float *rays, int n, float *t, int32_t *idx, int32_t *just)
{
    int64_t tests = 0;
#pragma omp parallel for schedule(dynamic, 256) reduction(+ : tests)
    for (int i = 0; i < n; ++i) {
        const sel h = bvh_one(nodes, order, lo, hi, s, ns, p, np, ray_of(rays + 6 * (size_t)i), &tests);
        t[i] = h.t; idx[i] = h.idx; just[i] = h.just;
    }
    return tests;
}
