/* ray_bounce_reference.c -- TEST-ONLY: what ptmi_bounce_rays_device computes, as ONE prepareRay (Trace.hs:359-383) written over the oracle's
 * own functions -- ora_near_zero_v3, ora_check_hit, ora_calc_next_ray -- the body of ora_trace_inline's loop with its state in the
 * caller's arrays:
 *     nearZero throughput || isNothing (checkHit scene ray)  ->  throughput = 0; ray, radiance and seed stay
 *     otherwise computeRay:  radiance += emittance * throughput;  throughput *= tmod;  ray = next ray;  seed = seed'
 * Built by tests/ray_bounce_inputs.py with the oracle's flags and linked against the oracle library (spheres and planes), or against the
 * mesh reference library of tests/mesh_rays.py, whose ora_check_hit is the mesh checkHit: spheres ++ planes ++ triangles. */
#include <stddef.h>
#include <stdint.h>

#include "../../oracle/pt_oracle.h"

enum { BOUNCE_FROZEN = 0, BOUNCE_MISSED = 1, BOUNCE_HIT = 2 };

/* rays: n x 6 floats, throughput and radiance: n x 3 floats, seed: n x 4 words (a, b, c, counter) -- all read and written.
 * outcome, unless NULL: BOUNCE_* per ray.  hit, unless NULL: n x 6 floats, the position and normal checkHit gave (zeros unless BOUNCE_HIT). */
void ray_bounce_reference(const ora_sphere *spheres, int n_spheres, const ora_plane *planes, int n_planes, float *rays, int n, float *throughput,
                          float *radiance, uint32_t *seed, int32_t *outcome, float *hit)
{
    ora_scene scene;
    scene.spheres = spheres; scene.n_spheres = n_spheres; scene.planes = planes; scene.n_planes = n_planes;
#ifdef _OPENMP
#pragma omp parallel for schedule(dynamic, 16)
#endif
    for (int i = 0; i < n; ++i) {
        float *q = rays + 6 * (size_t)i, *tp = throughput + 3 * (size_t)i, *rp = radiance + 3 * (size_t)i;
        uint32_t *w = seed + 4 * (size_t)i;
        ora_ray ray;
        ray.origin.x = q[0]; ray.origin.y = q[1]; ray.origin.z = q[2];
        ray.direction.x = q[3]; ray.direction.y = q[4]; ray.direction.z = q[5];
        const ora_v3 thr = { tp[0], tp[1], tp[2] };
        int what = BOUNCE_FROZEN;
        float rec[6] = { 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f };
        if (!ora_near_zero_v3(thr)) {
            const ora_maybe_hit next_hit = ora_check_hit(&scene, ray);
            what = next_hit.is_just ? BOUNCE_HIT : BOUNCE_MISSED;
            if (next_hit.is_just) {                              /* computeRay */
                const ora_sfc32 s = { w[0], w[1], w[2], w[3] };
                const float il = next_hit.material.illuminance;
                const ora_v3 c = next_hit.material.color;
                const ora_v3 emittance = { c.x * il, c.y * il, c.z * il };           /* mColor ^* illuminance */
                ora_ray next_ray; ora_v3 tmod; ora_sfc32 s2;
                ora_calc_next_ray(&next_hit.material, next_hit.normal_p, ray, s, &next_ray, &tmod, &s2);
                rp[0] = rp[0] + emittance.x * thr.x; rp[1] = rp[1] + emittance.y * thr.y; rp[2] = rp[2] + emittance.z * thr.z;
                tp[0] = thr.x * tmod.x; tp[1] = thr.y * tmod.y; tp[2] = thr.z * tmod.z;
                q[0] = next_ray.origin.x; q[1] = next_ray.origin.y; q[2] = next_ray.origin.z;
                q[3] = next_ray.direction.x; q[4] = next_ray.direction.y; q[5] = next_ray.direction.z;
                w[0] = s2.a; w[1] = s2.b; w[2] = s2.c; w[3] = s2.counter;
                rec[0] = next_hit.normal_p.origin.x; rec[1] = next_hit.normal_p.origin.y; rec[2] = next_hit.normal_p.origin.z;
                rec[3] = next_hit.normal_p.direction.x; rec[4] = next_hit.normal_p.direction.y; rec[5] = next_hit.normal_p.direction.z;
            }
        }
        if (what != BOUNCE_HIT) { tp[0] = 0.0f; tp[1] = 0.0f; tp[2] = 0.0f; }
        if (outcome) outcome[i] = what;
        if (hit) for (int k = 0; k < 6; ++k) hit[6 * (size_t)i + k] = rec[k];
    }
}
