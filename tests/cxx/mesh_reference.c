/* mesh_reference.c -- TEST-ONLY: the oracle's render loops (oracle/pt_oracle.c, unmodified) with checkHit over a MESH scene
 * (ptmi_set_scene_mesh): the literal left fold over spheres ++ planes ++ triangles.  tests/mesh_rays.py builds it with the oracle's
 * flags: pt_oracle.c is compiled to an object of its own whose ora_check_hit is made WEAK (objcopy --weaken-symbol), and this unit's
 * ora_check_hit -- a strong definition -- takes its place at every call the render loops make (the oracle is position-independent
 * code, so those calls go through the symbol, not inlined).  The triangles are set once before a render (mesh_reference_set) and
 * only read while it runs.
 *
 * The triangle, verbatim from csrc/ptmi_mesh_device.h (every operation an f32 operation rounded on its own):
 *   n = cross(v1 - v0, v2 - v0), nn = dot(n, n); zero area iff !(nn > 0) -- never hit; else n^ = n / sqrt(nn) per component
 *   denom = dot(d, n^);  t = dot(v0 - o, n^) / denom;  p = o + d ^* t
 *   w0 = dot(cross(v1 - v0, p - v0), n^),  w1 = dot(cross(v2 - v1, p - v1), n^),  w2 = dot(cross(v0 - v2, p - v2), n^)
 *   Just t  iff  !(denom > 1e-6) && !(t < 0) && w0 >= 0 && w1 >= 0 && w2 >= 0
 *   hit: position p (hit's o + d ^* t), normal n^, the triangle's material. */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "../../oracle/pt_oracle.h"
#include "../../include/ptmi.h"

#define INF_KEY 3.40282346638528859812e+38f

static ora_v3 mk(float x, float y, float z) { ora_v3 r; r.x = x; r.y = y; r.z = z; return r; }
static ora_v3 sub(ora_v3 a, ora_v3 b) { return mk(a.x - b.x, a.y - b.y, a.z - b.z); }
static float dot(ora_v3 a, ora_v3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
static ora_v3 cross(ora_v3 a, ora_v3 b) { return mk(a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x); }

typedef struct { ora_v3 v0, v1, v2, n; ora_material m; } tri;
static tri *g_tri = NULL;
static int g_nt = 0;

void mesh_reference_set(const ptmi_triangle *t, int n)
{
    free(g_tri);
    g_tri = n > 0 ? (tri *)malloc((size_t)n * sizeof(tri)) : NULL;
    g_nt = n;
    for (int k = 0; k < n; ++k) {
        tri *r = &g_tri[k];
        r->v0 = mk(t[k].v0[0], t[k].v0[1], t[k].v0[2]);
        r->v1 = mk(t[k].v1[0], t[k].v1[1], t[k].v1[2]);
        r->v2 = mk(t[k].v2[0], t[k].v2[1], t[k].v2[2]);
        const ora_v3 nv = cross(sub(r->v1, r->v0), sub(r->v2, r->v0));
        const float nn = dot(nv, nv);
        if (!(nn > 0.0f)) r->n = mk(NAN, NAN, NAN);
        else { const float len = sqrtf(nn); r->n = mk(nv.x / len, nv.y / len, nv.z / len); }
        r->m.color = mk(t[k].color[0], t[k].color[1], t[k].color[2]);
        r->m.illuminance = t[k].illuminance;
        r->m.brdf_tag = t[k].brdf_tag;
        r->m.brdf_param = t[k].brdf_param;
    }
}

static ora_maybe_float distance_to_triangle(ora_ray r, const tri *tr)
{
    const ora_v3 o = r.origin, d = r.direction;
    const float denom = dot(d, tr->n);
    const float t = dot(sub(tr->v0, o), tr->n) / denom;
    const ora_v3 p = mk(o.x + d.x * t, o.y + d.y * t, o.z + d.z * t);
    const float w0 = dot(cross(sub(tr->v1, tr->v0), sub(p, tr->v0)), tr->n);
    const float w1 = dot(cross(sub(tr->v2, tr->v1), sub(p, tr->v1)), tr->n);
    const float w2 = dot(cross(sub(tr->v0, tr->v2), sub(p, tr->v2)), tr->n);
    ora_maybe_float m;
    m.is_just = !(denom > 1e-6f) && !(t < 0.0f) && w0 >= 0.0f && w1 >= 0.0f && w2 >= 0.0f && !isnan(tr->n.x);
    m.value = m.is_just ? t : 0.0f;
    return m;
}

/* checkHit (Trace.hs:443-447) over spheres ++ planes ++ triangles: the oracle's fold, continued over the triangles */
ora_maybe_hit ora_check_hit(const ora_scene *scene, ora_ray r)
{
    ora_maybe_hit acc; float acc_key = 0.0f; int first = 1;
    memset(&acc, 0, sizeof acc);
    const int n = scene->n_spheres + scene->n_planes + g_nt;
    for (int i = 0; i < n; ++i) {
        ora_maybe_float d;
        ora_maybe_hit h;
        memset(&h, 0, sizeof h);
        if (i < scene->n_spheres) {
            d = ora_distance_to_sphere(r, &scene->spheres[i]);
            if (d.is_just) h = ora_hit_sphere(r, d.value, &scene->spheres[i]);
        } else if (i < scene->n_spheres + scene->n_planes) {
            const ora_plane *p = &scene->planes[i - scene->n_spheres];
            d = ora_distance_to_plane(r, p);
            if (d.is_just) h = ora_hit_plane(r, d.value, p);
        } else {
            const tri *tr = &g_tri[i - scene->n_spheres - scene->n_planes];
            d = distance_to_triangle(r, tr);
            if (d.is_just) {
                h.is_just = 1;
                h.normal_p.origin = mk(r.origin.x + r.direction.x * d.value, r.origin.y + r.direction.y * d.value,
                                       r.origin.z + r.direction.z * d.value);
                h.normal_p.direction = tr->n;
                h.material = tr->m;
            }
        }
        const float key = d.is_just ? d.value : INF_KEY;
        if (first) { acc = h; acc_key = key; first = 0; }
        else if (!(acc_key <= key)) { acc = h; acc_key = key; }
    }
    return acc;
}
