/* ray_paths_reference.c -- TEST-ONLY: what ptmi_trace_paths_device computes, by the oracle's own traceInline (ora_trace_inline,
 * Trace.hs:344-383) in the loop ora_render_inline_ex runs for a pixel, with the ray given where that loop makes a camera's:
 *     repeat n_spp times:  (new, seed') = traceInline limit scene ray_i seed_i;  color_i = new + color_i;  seed_i = seed'
 * Built by tests/ray_paths_inputs.py with the oracle's flags and linked against the oracle library (spheres and planes), or against the
 * mesh reference library of tests/mesh_rays.py (the same traceInline over the mesh checkHit: spheres ++ planes ++ triangles). */
#include <stddef.h>
#include <stdint.h>

#include "../../oracle/pt_oracle.h"

/* The primary rays of a width x height image, row by row (pixel (x, y) at y * width + x), as ora_render_inline_ex makes them: rays, n x 6 floats */
void ray_paths_primaries(const ora_camera *cam, int width, int height, float *rays)
{
    const ora_primary_uniforms u = ora_primary_setup(cam, width, height);
    for (int y = 0; y < height; ++y)
        for (int x = 0; x < width; ++x) {
            const ora_ray r = ora_primary_ray(&u, x, y, width, height);
            float *q = rays + 6 * ((size_t)y * width + x);
            q[0] = r.origin.x; q[1] = r.origin.y; q[2] = r.origin.z;
            q[3] = r.direction.x; q[4] = r.direction.y; q[5] = r.direction.z;
        }
}

/* rays: n x 6 floats (origin, direction); color: n x 3 floats and seed: n x 4 words (a, b, c, counter), both read and written.
 * live_min / live_max, unless NULL: the fewest and the most live bounces of a sample of ray i (0 and 0 when n_spp <= 0). */
void ray_paths_reference(int limit, int n_spp, const ora_sphere *spheres, int n_spheres, const ora_plane *planes, int n_planes, const float *rays, int n,
                         float *color, uint32_t *seed, int32_t *live_min, int32_t *live_max)
{
    ora_scene scene;
    scene.spheres = spheres; scene.n_spheres = n_spheres; scene.planes = planes; scene.n_planes = n_planes;
#ifdef _OPENMP
#pragma omp parallel for schedule(dynamic, 16)
#endif
    for (int i = 0; i < n; ++i) {
        const float *q = rays + 6 * (size_t)i;
        float *c = color + 3 * (size_t)i;
        uint32_t *w = seed + 4 * (size_t)i;
        ora_ray primary;
        primary.origin.x = q[0]; primary.origin.y = q[1]; primary.origin.z = q[2];
        primary.direction.x = q[3]; primary.direction.y = q[4]; primary.direction.z = q[5];
        ora_sfc32 s = { w[0], w[1], w[2], w[3] };
        ora_v3 acc = { c[0], c[1], c[2] };
        int lo = 0, hi = 0;
        for (int k = 0; k < n_spp; ++k) {
            ora_v3 nw; ora_sfc32 s2; int live;
            ora_trace_inline(limit, &scene, primary, s, &nw, &s2, &live);
            acc.x = nw.x + acc.x; acc.y = nw.y + acc.y; acc.z = nw.z + acc.z;      /* new + old */
            s = s2;
            lo = (k == 0 || live < lo) ? live : lo;
            hi = (k == 0 || live > hi) ? live : hi;
        }
        c[0] = acc.x; c[1] = acc.y; c[2] = acc.z;
        w[0] = s.a; w[1] = s.b; w[2] = s.c; w[3] = s.counter;
        if (live_min) live_min[i] = lo;
        if (live_max) live_max[i] = hi;
    }
}
