/* ray_streams_reference.c -- TEST-ONLY: what ptmi_trace_streams_device computes, the contract of include/ptmi.h ("render Streams along a
 * caller's rays") in plain C over the oracle's public functions: ora_check_hit, ora_calc_next_ray, ora_gen_vec, ora_random_float and
 * ora_near_zero_v3.  The walk is the one ora_render_streams_tree runs for a pixel, with the ray given where that loop makes a camera's
 * and the seed rule ora_render_streams_ex states (ORA_SEED_FROM_RESULT: every hit leaves the seed its ray carried).  glass_children is
 * restated here from the formula in include/ptmi.h; tests/test_ray_streams_reference.py holds all of it to the oracle's render loops.
 * Built by tests/ray_streams_inputs.py with the oracle's flags and linked against the oracle library (spheres and planes), or against the
 * mesh reference library of tests/mesh_rays.py (the mesh checkHit: spheres ++ planes ++ triangles). */
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "../../oracle/pt_oracle.h"

#define RS_EPSILON 0.002f
#define RS_MAX_STACK 64

typedef struct { ora_ray ray; ora_v3 throughput; ora_sfc32 seed; int steps; } rs_state;

static ora_v3 rs_v3(float x, float y, float z) { ora_v3 r; r.x = x; r.y = y; r.z = z; return r; }
static ora_v3 rs_add(ora_v3 a, ora_v3 b) { return rs_v3(a.x + b.x, a.y + b.y, a.z + b.z); }
static ora_v3 rs_sub(ora_v3 a, ora_v3 b) { return rs_v3(a.x - b.x, a.y - b.y, a.z - b.z); }
static ora_v3 rs_mul(ora_v3 a, ora_v3 b) { return rs_v3(a.x * b.x, a.y * b.y, a.z * b.z); }
static ora_v3 rs_scale_r(ora_v3 v, float a) { return rs_v3(v.x * a, v.y * a, v.z * a); }
static ora_v3 rs_scale_l(float a, ora_v3 v) { return rs_v3(a * v.x, a * v.y, a * v.z); }
static float rs_dot(ora_v3 a, ora_v3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }

/* GLASS ior, from include/ptmi.h:
 *   (rv, seed') = genVec seed ; dn = d . n ; cosi = -dn ; eta = 1 / ior ; k = 1 - (eta*eta) * (1 - cosi*cosi)
 *   reflection = d - (2*dn) *^ n ; r0 = ((1-ior)/(1+ior))^2 ; m = 1 - cosi ; R = r0 + (1-r0) * (((m*m)*(m*m))*m)
 *   k < 0:  R = 1, refraction = reflection ; else refraction = eta *^ d + (eta*cosi - sqrt k) *^ n
 *   child 0 = (p + reflection ^* epsilon, reflection), throughput * (color ^* R),     seed'
 *   child 1 = (p + refraction ^* epsilon, refraction), throughput * (color ^* (1-R)), seed' advanced one draw */
static void rs_glass_children(const ora_material *m, ora_ray normal_p, ora_ray ray, ora_v3 throughput, ora_sfc32 seed, rs_state out[2])
{
    const ora_v3 n = normal_p.direction, d = ray.direction, p = normal_p.origin;
    (void)ora_gen_vec(&seed);
    const float ior = m->brdf_param;
    const float dn = rs_dot(d, n);
    const float cosi = -dn;
    const float eta = 1.0f / ior;
    const float k = 1.0f - (eta * eta) * (1.0f - cosi * cosi);
    const ora_v3 reflection = rs_sub(d, rs_scale_l(2.0f * dn, n));
    float r0 = (1.0f - ior) / (1.0f + ior);
    r0 = r0 * r0;
    const float mm = 1.0f - cosi;
    float R = r0 + (1.0f - r0) * (((mm * mm) * (mm * mm)) * mm);
    ora_v3 refraction;
    if (k < 0.0f) { R = 1.0f; refraction = reflection; }
    else refraction = rs_add(rs_scale_l(eta, d), rs_scale_l(eta * cosi - sqrtf(k), n));
    out[0].ray.origin = rs_add(p, rs_scale_r(reflection, RS_EPSILON)); out[0].ray.direction = reflection;
    out[0].throughput = rs_mul(throughput, rs_scale_r(m->color, R));
    out[0].seed = seed;
    out[1].ray.origin = rs_add(p, rs_scale_r(refraction, RS_EPSILON)); out[1].ray.direction = refraction;
    out[1].throughput = rs_mul(throughput, rs_scale_r(m->color, 1.0f - R));
    (void)ora_random_float(&seed);
    out[1].seed = seed;
}

enum { RS_GLASS_HITS = 0, RS_DEEPEST = 1, RS_DROPPED = 2, RS_TRUNCATED = 3, RS_HITS = 4, RS_FIRST_GLASS = 5, RS_FIRST_CHILDREN = 6, RS_GLASS_BELOW = 7, RS_DIAG = 8 };

/* rays: n x 6 floats (origin, direction); color: n x 3 floats and seed: n x 4 words (a, b, c, counter), both read and written.
 * lost, unless NULL: two words ADDED to -- the rays the cap cut, the children a full stack dropped.
 * diag, unless NULL: RS_DIAG words per ray over all its samples -- glass hits, the deepest stack, dropped, truncated, hits, whether the
 * ray's first hit was glass, how many of that hit's two children hit something, glass hits below the first hit. */
void ray_streams_reference(int step_cap, int n_spp, int from_result, int stack_depth, const ora_sphere *spheres, int n_spheres, const ora_plane *planes,
                           int n_planes, const float *rays, int n, float *color, uint32_t *seed, int64_t *lost, int32_t *diag)
{
    ora_scene scene;
    scene.spheres = spheres; scene.n_spheres = n_spheres; scene.planes = planes; scene.n_planes = n_planes;
    if (stack_depth > RS_MAX_STACK) stack_depth = RS_MAX_STACK;
    int64_t n_truncated = 0, n_dropped = 0;
#ifdef _OPENMP
#pragma omp parallel for schedule(dynamic, 16) reduction(+:n_truncated, n_dropped)
#endif
    for (int i = 0; i < n; ++i) {
        const float *q = rays + 6 * (size_t)i;
        float *c = color + 3 * (size_t)i;
        uint32_t *w = seed + 4 * (size_t)i;
        ora_ray primary;
        primary.origin = rs_v3(q[0], q[1], q[2]);
        primary.direction = rs_v3(q[3], q[4], q[5]);
        ora_sfc32 pixel_seed = { w[0], w[1], w[2], w[3] };
        ora_v3 acc = rs_v3(c[0], c[1], c[2]);
        int32_t dg[RS_DIAG] = { 0 };
        rs_state stack[RS_MAX_STACK];
        for (int s = 0; s < n_spp; ++s) {
            int sp = 0, have = 1;
            rs_state cur;
            cur.ray = primary; cur.throughput = rs_v3(1.0f, 1.0f, 1.0f); cur.seed = pixel_seed; cur.steps = 0;
            while (have) {
                int ended = 1;
                if (cur.steps >= step_cap) { ++n_truncated; ++dg[RS_TRUNCATED]; }
                else {
                    const ora_maybe_hit hit = ora_check_hit(&scene, cur.ray);
                    const int first = cur.steps == 0;
                    ++cur.steps;
                    if (hit.is_just) {
                        const ora_v3 emittance = rs_scale_r(hit.material.color, hit.material.illuminance);
                        acc = rs_add(acc, rs_mul(emittance, cur.throughput));
                        ++dg[RS_HITS];
                        if (from_result) pixel_seed = cur.seed;
                        if (!ora_near_zero_v3(cur.throughput)) {
                            if (hit.material.brdf_tag == ORA_GLASS) {
                                rs_state kids[2];
                                rs_glass_children(&hit.material, hit.normal_p, cur.ray, cur.throughput, cur.seed, kids);
                                ++dg[RS_GLASS_HITS];
                                if (!first) ++dg[RS_GLASS_BELOW];
                                if (first && s == 0) {
                                    dg[RS_FIRST_GLASS] = 1;
                                    dg[RS_FIRST_CHILDREN] = ora_check_hit(&scene, kids[0].ray).is_just + ora_check_hit(&scene, kids[1].ray).is_just;
                                }
                                if (cur.steps >= step_cap) { n_truncated += 2; dg[RS_TRUNCATED] += 2; }
                                else {
                                    if (sp < stack_depth) {
                                        stack[sp] = kids[1]; stack[sp].steps = cur.steps; ++sp;
                                        if (sp > dg[RS_DEEPEST]) dg[RS_DEEPEST] = sp;
                                    } else { ++n_dropped; ++dg[RS_DROPPED]; }
                                    cur.ray = kids[0].ray; cur.throughput = kids[0].throughput; cur.seed = kids[0].seed;
                                    ended = 0;
                                }
                            } else {
                                ora_ray next_ray; ora_v3 tmod; ora_sfc32 seed2;
                                ora_calc_next_ray(&hit.material, hit.normal_p, cur.ray, cur.seed, &next_ray, &tmod, &seed2);
                                cur.throughput = rs_mul(cur.throughput, tmod);
                                cur.ray = next_ray; cur.seed = seed2;
                                if (cur.steps >= step_cap) { ++n_truncated; ++dg[RS_TRUNCATED]; } else ended = 0;
                            }
                        }
                    }
                }
                if (ended) {
                    if (sp > 0) { --sp; cur = stack[sp]; }
                    else have = 0;
                }
            }
            (void)ora_random_float(&pixel_seed);      /* updateSeed */
        }
        c[0] = acc.x; c[1] = acc.y; c[2] = acc.z;
        w[0] = pixel_seed.a; w[1] = pixel_seed.b; w[2] = pixel_seed.c; w[3] = pixel_seed.counter;
        if (diag) for (int k = 0; k < RS_DIAG; ++k) diag[RS_DIAG * (size_t)i + k] = dg[k];
    }
    if (lost) { lost[0] += n_truncated; lost[1] += n_dropped; }
}
