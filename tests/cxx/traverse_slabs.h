/* traverse_slabs.h -- TEST-ONLY: the box tests of the two hierarchies as the device makes them (bvh_slab, bvh_sphere_slab: csrc/ptmi_bvh_device.h;
 * mesh_slab: csrc/ptmi_mesh_device.h), one child of one node at a time, for the CPU restatements of the walks: bvh_traverse.c and
 * mesh_traverse.c (the closest hit) and any_hit_traverse.c (occlusion).  Every operation is an f32 operation rounded on its own (the
 * files are built with -ffp-contract=off).  widen: 1.0f is the device's margin; any_hit_traverse.c alone passes another factor, to show
 * that its tests would notice a margin that is too small. */
#ifndef PTMI_TESTS_TRAVERSE_SLABS_H
#define PTMI_TESTS_TRAVERSE_SLABS_H

#include <math.h>

#include "../../include/ptmi.h"

#define SLAB_K_FAR (1.0f + 2.0f * (3.0f * 0x1p-24f) / (1.0f - 3.0f * 0x1p-24f))      /* 1 + 2 gamma_3 */

static inline float inv_of(float v)
{
    const float c = fabsf(v) < 0x1p-80f ? copysignf(0x1p-80f, v) : v;
    return 1.0f / c;
}

/* The sphere hierarchy's child c of node nd for the ray (o, 1 / d = inv), eta = | |d|^2 - 1 |: G = 2^-19 + 2 eta, G_lin = G + 2^-19,
 * sqrt_G = sqrt(G).  Assigns the entry distance; returns t_near <= t_far. */
static inline int sphere_child_slab(const ptmi_bvh_node *nd, int c, const float o[3], const float inv[3], float G, float G_lin, float sqrt_G,
                                    float widen, float *t_near_out)
{
    float e[3], ab[3];
    for (int a = 0; a < 3; ++a) { e[a] = nd->center[c][a] - o[a]; ab[a] = fabsf(e[a]) + nd->half[c][a]; }
    const float p1 = (ab[0] + ab[1]) + ab[2], p2 = (ab[0] * ab[0] + ab[1] * ab[1]) + ab[2] * ab[2];
    float m = ((fminf(sqrt_G * p1, (G * p2) * nd->inv_2r[c]) + G_lin * p1) + 0x1p-30f) * (1.0f + 0x1p-10f);
    if (widen != 1.0f) m = m * widen;
    float tlo[3], thi[3];
    for (int a = 0; a < 3; ++a) {
        const float tm = e[a] * inv[a], hh = (nd->half[c][a] + m) * fabsf(inv[a]);
        tlo[a] = tm - hh; thi[a] = tm + hh;
    }
    const float t_near = fmaxf(fmaxf(tlo[0], tlo[1]), fmaxf(tlo[2], 0.0f));
    const float t_far = fminf(fminf(thi[0], thi[1]), thi[2]) * SLAB_K_FAR;
    *t_near_out = t_near;
    return t_near <= t_far;
}

/* The triangle hierarchy's child c of node nd for the ray (o, inv, ainv = |inv|), o1 the L1 norm of the origin */
static inline int mesh_child_slab(const ptmi_bvh_node *nd, int c, const float o[3], const float inv[3], const float ainv[3], float o1,
                                  float widen, float *t_near_out)
{
    const float ex = nd->center[c][0] - o[0], ey = nd->center[c][1] - o[1], ez = nd->center[c][2] - o[2];
    const float ax = fabsf(ex) + nd->half[c][0], ay = fabsf(ey) + nd->half[c][1], az = fabsf(ez) + nd->half[c][2];
    const float p1 = (ax + ay) + az;
    float m = ((p1 + o1) * 0x1p-16f + 0x1p-30f) * (1.0f + 0x1p-10f);
    if (widen != 1.0f) m = m * widen;
    const float tmx = ex * inv[0], hx = (nd->half[c][0] + m) * ainv[0];
    const float tmy = ey * inv[1], hy = (nd->half[c][1] + m) * ainv[1];
    const float tmz = ez * inv[2], hz = (nd->half[c][2] + m) * ainv[2];
    const float t_near = fmaxf(fmaxf(tmx - hx, tmy - hy), fmaxf(tmz - hz, 0.0f));
    const float tf = fminf(fminf(tmx + hx, tmy + hy), tmz + hz) * SLAB_K_FAR;
    *t_near_out = t_near;
    return t_near <= tf;
}

#endif
