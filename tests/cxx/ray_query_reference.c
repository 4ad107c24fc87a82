/* ray_query_reference.c -- TEST-ONLY: the hit records of rays that hit SPHERES, by the oracle's own function (ora_hit_sphere: the hit
 * position o + d ^* t and normalize (position - centre), Intersection.hs:29-32, :50), for tests/test_gpu_ray_query.py to hold
 * ptmi_trace_rays_device's records against.  Built by that test with the oracle's flags and linked against the oracle library. */
#include <stddef.h>
#include <stdint.h>

#include "../../oracle/pt_oracle.h"

/* For every ray i with 0 <= idx[i] < n_spheres: out[6 i ..] = (position, normal) of its hit at distance t[i] on sphere idx[i]; other
 * rows are left as they are.  rays: n x 6 floats (origin, direction). */
void ray_query_sphere_records(const ora_sphere *spheres, int n_spheres, const float *rays, const float *t, const int32_t *idx, int n, float *out)
{
    for (int i = 0; i < n; ++i) {
        if (idx[i] < 0 || idx[i] >= n_spheres) continue;
        const float *q = rays + 6 * (size_t)i;
        ora_ray r;
        r.origin.x = q[0]; r.origin.y = q[1]; r.origin.z = q[2];
        r.direction.x = q[3]; r.direction.y = q[4]; r.direction.z = q[5];
        const ora_maybe_hit h = ora_hit_sphere(r, t[i], &spheres[idx[i]]);
        float *o = out + 6 * (size_t)i;
        o[0] = h.normal_p.origin.x; o[1] = h.normal_p.origin.y; o[2] = h.normal_p.origin.z;
        o[3] = h.normal_p.direction.x; o[4] = h.normal_p.direction.y; o[5] = h.normal_p.direction.z;
    }
}
