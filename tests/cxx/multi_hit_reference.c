/* multi_hit_reference.c -- TEST-ONLY: the SPECIFICATION of ptmi_trace_rays_multi_device (include/ptmi.h, "multi-hit") on the CPU, by
 * enumeration: every primitive of the scene -- spheres, then planes, then triangles -- is tested with the oracle's own distance functions
 * (ora_distance_to_sphere, ora_distance_to_plane) and the triangle test of triangle_test.h (mesh_reference.c's, on the stored records);
 * the pairs (t, j) of the Justs with t < lim are kept, sorted ascending by (t, j), and truncated to k.  No hierarchy, no bound, no fold.
 * Built with the oracle's flags (no contraction, no fast-math).  Per ray it also reports
 *     total    |H|, whatever k is
 *     flags    bit 0: some primitive's key is a NaN (a Just whose t is a NaN); bit 1: some Just has t = +inf
 *     tie      two of the listed hits have the same t */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>

#include "../../oracle/pt_oracle.h"
#include "triangle_test.h"

typedef struct { float t; int32_t j; } hit;

static int before(hit a, hit b) { return a.t < b.t || (a.t == b.t && a.j < b.j); }

/* (t, j) into the ascending list of at most k */
static void keep(hit *list, int *held, int k, hit h)
{
    if (*held == k && !before(h, list[k - 1])) return;
    int at = *held < k ? (*held)++ : k - 1;
    while (at > 0 && before(h, list[at - 1])) { list[at] = list[at - 1]; --at; }
    list[at] = h;
}

/* t_max: n words, or NULL for +inf.  recs: nt records of 12 words (v0, v1, v2, n) by original index, or NULL.  k: any positive number. */
void multi_hit_reference(const ora_sphere *s, int ns, const ora_plane *p, int np, const float *recs, int nt, const float *rays, const float *t_max,
                         int n, int k, float *t_out, int32_t *idx_out, int32_t *count_out, int32_t *total_out, int32_t *flags_out, int32_t *tie_out)
{
    const trec *tr = (const trec *)recs;
#pragma omp parallel for schedule(dynamic, 64)
    for (int i = 0; i < n; ++i) {
        const float *q = rays + 6 * (size_t)i;
        ora_ray r;
        r.origin.x = q[0]; r.origin.y = q[1]; r.origin.z = q[2];
        r.direction.x = q[3]; r.direction.y = q[4]; r.direction.z = q[5];
        const v3 o = mk(q[0], q[1], q[2]), d = mk(q[3], q[4], q[5]);
        const float lim = t_max ? t_max[i] : INFINITY;
        hit *list = (hit *)malloc(sizeof(hit) * (size_t)k);
        int held = 0, total = 0, flags = 0;
        for (int j = 0; j < ns + np + nt; ++j) {
            float t;
            int just;
            if (j < ns + np) {
                const ora_maybe_float m = j < ns ? ora_distance_to_sphere(r, &s[j]) : ora_distance_to_plane(r, &p[j - ns]);
                just = m.is_just; t = m.value;
            } else {
                just = tri_test(&tr[j - ns - np], o, d, &t);
            }
            if (!just) continue;
            if (isnan(t)) flags |= 1;
            if (isinf(t)) flags |= 2;
            if (!(t < lim)) continue;
            ++total;
            const hit h = {t, j};
            keep(list, &held, k, h);
        }
        int tie = 0;
        for (int c = 0; c < k; ++c) {
            t_out[(size_t)i * k + c] = c < held ? list[c].t : 0.0f;
            idx_out[(size_t)i * k + c] = c < held ? list[c].j : -1;
            if (c > 0 && c < held && list[c].t == list[c - 1].t) tie = 1;
        }
        count_out[i] = held; total_out[i] = total; flags_out[i] = flags; tie_out[i] = tie;
        free(list);
    }
}
