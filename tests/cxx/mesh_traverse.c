/* mesh_traverse.c -- TEST-ONLY: checkHit over a mesh scene (ptmi_set_scene_mesh) on the CPU.
 *   mesh_lin_check_hit: the literal left fold over spheres ++ planes ++ triangles (the oracle's sphere and plane tests, the triangle
 *     test below), keeping the index; a miss is reported as (0, -1, 0).
 *   mesh_walk_check_hit: the spheres and planes by the same fold, then the triangle hierarchy ptmi_mesh_layout exports, walked as
 *     check_hit_mesh (csrc/ptmi_mesh_device.h) walks it -- the same admission of a ray, margin, slab test, pruning against the best key
 *     and tie rule -- so that tests can show that the padding and the pruning never lose the hit the linear fold finds.
 * Built with the oracle's flags (no contraction, no fast-math).  The box test is traverse_slabs.h's and the triangle test triangle_test.h's;
 * any_hit_traverse.c (the occlusion walks) shares both.
 *
 * The triangle test, verbatim from ptmi_mesh_device.h (every operation an f32 operation rounded on its own):
 *   n = cross(v1 - v0, v2 - v0) (linear's component order), nn = dot(n, n); zero area iff !(nn > 0) -- never hit; else
 *   n^ = n / sqrt(nn) per component
 *   denom = dot(d, n^);  cand = !(denom > 1e-6)
 *   t = dot(v0 - o, n^) / denom
 *   p = o + d ^* t
 *   w0 = dot(cross(v1 - v0, p - v0), n^),  w1 = dot(cross(v2 - v1, p - v1), n^),  w2 = dot(cross(v0 - v2, p - v2), n^)
 *   Just t  iff  cand && !(t < 0) && w0 >= 0 && w1 >= 0 && w2 >= 0 */
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "../../oracle/pt_oracle.h"
#include "../../include/ptmi.h"
#include "traverse_slabs.h"
#include "triangle_test.h"

#define INF_KEY 3.40282346638528859812e+38f

typedef struct { float t; int idx; int just; } sel;

static trec record_of(const ptmi_triangle *t)
{
    trec r;
    r.v0 = mk(t->v0[0], t->v0[1], t->v0[2]); r.v1 = mk(t->v1[0], t->v1[1], t->v1[2]); r.v2 = mk(t->v2[0], t->v2[1], t->v2[2]);
    const v3 n = cross(sub(r.v1, r.v0), sub(r.v2, r.v0));
    const float nn = dot(n, n);
    if (!(nn > 0.0f)) { r.n = mk(NAN, NAN, NAN); return r; }
    const float len = sqrtf(nn);
    r.n = mk(n.x / len, n.y / len, n.z / len);
    return r;
}

static ora_ray ray_of(const float *q)
{
    ora_ray r;
    r.origin.x = q[0]; r.origin.y = q[1]; r.origin.z = q[2];
    r.direction.x = q[3]; r.direction.y = q[4]; r.direction.z = q[5];
    return r;
}

/* the literal fold over spheres ++ planes ++ triangles, accumulator (key, selection) */
static void fold_sp(const ora_sphere *s, int ns, const ora_plane *p, int np, ora_ray r, sel *acc, float *acc_key)
{
    for (int i = 0; i < ns + np; ++i) {
        const ora_maybe_float d = i < ns ? ora_distance_to_sphere(r, &s[i]) : ora_distance_to_plane(r, &p[i - ns]);
        const float key = d.is_just ? d.value : INF_KEY;
        if (i == 0 || !(*acc_key <= key)) { *acc_key = key; acc->t = d.value; acc->idx = i; acc->just = d.is_just; }
    }
}

static sel fold_all(const ora_sphere *s, int ns, const ora_plane *p, int np, const trec *tr, int nt, ora_ray r)
{
    sel acc = {0.0f, 0, 0};
    float acc_key = 0.0f;
    fold_sp(s, ns, p, np, r, &acc, &acc_key);
    const v3 o = mk(r.origin.x, r.origin.y, r.origin.z), d = mk(r.direction.x, r.direction.y, r.direction.z);
    for (int k = 0; k < nt; ++k) {
        float t;
        const int just = tri_test(&tr[k], o, d, &t);
        const float key = just ? t : INF_KEY;
        if ((ns + np == 0 && k == 0) || !(acc_key <= key)) { acc_key = key; acc.t = t; acc.idx = ns + np + k; acc.just = just; }
    }
    if (!acc.just) { acc.t = 0.0f; acc.idx = -1; }
    return acc;
}

void mesh_records(const ptmi_triangle *t, int nt, float *out)      /* 12 floats per triangle: v0, v1, v2, n^ */
{
    for (int k = 0; k < nt; ++k) {
        const trec r = record_of(&t[k]);
        memcpy(out + 12 * (size_t)k, &r, sizeof r);
    }
}

void mesh_lin_check_hit(const ora_sphere *s, int ns, const ora_plane *p, int np, const float *recs, int nt,
                        const float *rays, int n, float *t, int32_t *idx, int32_t *just)
{
    const trec *tr = (const trec *)recs;
#pragma omp parallel for schedule(dynamic, 256)
    for (int i = 0; i < n; ++i) {
        const sel h = fold_all(s, ns, p, np, tr, nt, ray_of(rays + 6 * (size_t)i));
        t[i] = h.t; idx[i] = h.idx; just[i] = h.just;
    }
}

/* check_hit_mesh with the spheres and planes by the fold: returns the triangles tested (-1 if the ray is not served) */
static int64_t walk_one(const ptmi_bvh_node *nodes, const int32_t *order, int n_kept, const float lo[3], const float hi[3],
                        const ora_sphere *s, int ns, const ora_plane *p, int np, const trec *tr, int nt, ora_ray r, sel *out)
{
    const float o3[3] = {r.origin.x, r.origin.y, r.origin.z}, d3[3] = {r.direction.x, r.direction.y, r.direction.z};
    const v3 o = mk(o3[0], o3[1], o3[2]), d = mk(d3[0], d3[1], d3[2]);
    const float eta = fabsf(dot(d, d) - 1.0f);
    float P2 = 0.0f;
    for (int a = 0; a < 3; ++a) {
        const float pa = fmaxf(fabsf(lo[a] - o3[a]), fabsf(hi[a] - o3[a]));
        P2 = P2 + pa * pa;
    }
    const float P = sqrtf(P2) * (1.0f + 0x1p-20f);
    int finite = 1;
    for (int a = 0; a < 3; ++a) finite &= isfinite(o3[a]) && isfinite(d3[a]);
    if (!(finite && eta <= 0x1p-12f && P <= 0x1p40f)) { *out = fold_all(s, ns, p, np, tr, nt, r); return -1; }
    /* the spheres and planes: check_hit_bvh's result (shown equal to the fold by tests/test_bvh_traversal.py), in its accumulator form */
    sel acc = {0.0f, 0, 0};
    float best_key = 0.0f;
    int best_idx = 0, best_just = 0;
    if (ns + np > 0) {
        fold_sp(s, ns, p, np, r, &acc, &best_key);
        best_idx = acc.idx; best_just = acc.just;          /* (a Nothing: key FLT_MAX, where the device may hold NaN -- the same outcome) */
    } else {
        best_key = NAN;
    }
    int64_t tests = 0;
    if (n_kept > 0) {
        const int first = ns + np;
        const v3 inv = mk(inv_of(d.x), inv_of(d.y), inv_of(d.z));
        const v3 ainv = mk(fabsf(inv.x), fabsf(inv.y), fabsf(inv.z));
        const float o1 = (fabsf(o.x) + fabsf(o.y)) + fabsf(o.z);
        const float inv3[3] = {inv.x, inv.y, inv.z}, ainv3[3] = {ainv.x, ainv.y, ainv.z};
        int stack[PTMI_BVH_MAX_DEPTH + 1], sp = 0, node = 0;
        for (;;) {
            const ptmi_bvh_node *nd = &nodes[node];
            float tn[2];
            int h[2];
            for (int c = 0; c < 2; ++c) {
                const int in_box = mesh_child_slab(nd, c, o3, inv3, ainv3, o1, 1.0f, &tn[c]);      /* traverse_slabs.h */
                const float bound = best_key == best_key ? best_key : INF_KEY;
                h[c] = in_box && nd->ref[c] != -1 && tn[c] <= bound;
            }
            const int swap = h[1] && (!h[0] || tn[1] < tn[0]);
            const int32_t ra = swap ? nd->ref[1] : nd->ref[0], rb = swap ? nd->ref[0] : nd->ref[1];
            const int ha = swap ? h[1] : h[0], hb = swap ? h[0] : h[1];
            const float tb = swap ? tn[0] : tn[1];
            int next = -1;
            for (int pass = 0; pass < 2; ++pass) {
                const int32_t ref = pass ? rb : ra;
                const float bound = best_key == best_key ? best_key : INF_KEY;
                if (!(pass ? (hb && tb <= bound) : ha)) continue;
                if (ref >= 0) {
                    if (next < 0) next = ref;
                    else { if (sp > PTMI_BVH_MAX_DEPTH) return -2; stack[sp++] = ref; }
                    continue;
                }
                const uint32_t v = (uint32_t)(-1 - ref);
                for (int k = 0; k < (int)(v & 255u); ++k) {
                    const int32_t j = order[(v >> 8) + (uint32_t)k];
                    const int i = first + j;
                    float t;
                    const int just = tri_test(&tr[j], o, d, &t);
                    ++tests;
                    if (just && (!(best_key <= t) || (t == best_key && i < best_idx))) { best_key = t; best_idx = i; best_just = 1; }
                }
            }
            if (next < 0) {
                if (sp == 0) break;
                next = stack[--sp];
            }
            node = next;
        }
    }
    if (best_just && !(best_key < INF_KEY)) { *out = fold_all(s, ns, p, np, tr, nt, r); return tests; }
    out->just = best_just;
    out->t = best_just ? best_key : 0.0f;
    out->idx = best_just ? best_idx : -1;
    return tests;
}

int64_t mesh_walk_check_hit(const ptmi_bvh_node *nodes, const int32_t *order, int n_kept, const float *lo, const float *hi,
                            const ora_sphere *s, int ns, const ora_plane *p, int np, const float *recs, int nt,
                            const float *rays, int n, float *t, int32_t *idx, int32_t *just)
{
    const trec *tr = (const trec *)recs;
    int64_t total = 0;
#pragma omp parallel for schedule(dynamic, 256) reduction(+ : total)
    for (int i = 0; i < n; ++i) {
        sel h;
        const int64_t k = walk_one(nodes, order, n_kept, lo, hi, s, ns, p, np, tr, nt, ray_of(rays + 6 * (size_t)i), &h);
        if (k == -2) { just[i] = -2; continue; }
        total += k > 0 ? k : 0;
        t[i] = h.t; idx[i] = h.idx; just[i] = h.just;
    }
    return total;
}
