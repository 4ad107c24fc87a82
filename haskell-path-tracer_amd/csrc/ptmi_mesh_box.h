// ptmi_mesh_box.h -- the arithmetic of the triangle hierarchy's boxes and of a triangle's derived normal, ONE definition for the host
// build (ptmi_mesh.cpp: mesh_build), the host refit (ptmi_mesh_refit_layout) and the device refit (ptmi_mesh_refit.hip): a refit is bit
// for bit the build's boxes because it runs the build's operations.  Boxes are unions in double of float data (exact), padded and
// stored as DESIGN.md 5.8 says; min / max are std::min / std::max written out (the FIRST of two equal operands is kept), so that the
// device takes the same operand where zeros of both signs meet.
#pragma once

#include "ptmi_core.h"

namespace ptmi {

constexpr double kMeshPadFactor = 1.0 / 65536.0;

PTMI_HD double box_min(double a, double b) { return b < a ? b : a; }      // std::min(a, b)
PTMI_HD double box_max(double a, double b) { return a < b ? b : a; }      // std::max(a, b)
PTMI_HD bool finite_f32(float x) { return (f2u(x) & 0x7f800000u) != 0x7f800000u; }

PTMI_HD void box_empty(double l[3], double h[3])
{
    for (int a = 0; a < 3; ++a) { l[a] = __builtin_inf(); h[a] = -__builtin_inf(); }
}

PTMI_HD void box_join(double l[3], double h[3], const double l2[3], const double h2[3])
{
    for (int a = 0; a < 3; ++a) { l[a] = box_min(l[a], l2[a]); h[a] = box_max(h[a], h2[a]); }
}

// ... with a stored child box (centre, half extent)
PTMI_HD void box_join_stored(double l[3], double h[3], const float center[3], const float half[3])
{
    for (int a = 0; a < 3; ++a) {
        l[a] = box_min(l[a], (double)center[a] - (double)half[a]);
        h[a] = box_max(h[a], (double)center[a] + (double)half[a]);
    }
}

// A triangle's box: its vertices' box padded by 2^-16 (max |coordinate| + extent), for the rounding of the hit point and the edge
// functions (the derivation is at check_hit_mesh, ptmi_mesh_device.h).
PTMI_HD void triangle_box(const float v0[3], const float v1[3], const float v2[3], double lo[3], double hi[3])
{
    double m = 0.0, ext = 0.0;
    for (int a = 0; a < 3; ++a) {
        const double l = box_min(box_min((double)v0[a], (double)v1[a]), (double)v2[a]);
        const double h = box_max(box_max((double)v0[a], (double)v1[a]), (double)v2[a]);
        m = box_max(box_max(m, __builtin_fabs(l)), __builtin_fabs(h));
        ext = box_max(ext, h - l);
        lo[a] = l; hi[a] = h;
    }
    const double pad = kMeshPadFactor * (m + ext);
    for (int a = 0; a < 3; ++a) { lo[a] = lo[a] - pad; hi[a] = hi[a] + pad; }
}

// (float)v, or its upper neighbour when that lies below v: a compare and a bit step (== std::nextafter towards +inf)
PTMI_HD float box_round_up(double v)
{
    float f = (float)v;
    if ((double)f < v) f = f == 0.0f ? u2f(1u) : (f > 0.0f ? u2f(f2u(f) + 1u) : u2f(f2u(f) - 1u));
    return f;
}

PTMI_HD void box_store(float center[3], float half[3], const double l[3], const double h[3])
{
    for (int a = 0; a < 3; ++a) {
        const float cf = (float)(0.5 * (l[a] + h[a]));
        center[a] = cf;
        half[a] = box_round_up(box_max(h[a] - (double)cf, (double)cf - l[a]));
    }
}

// A triangle's edges and normal by the device's f32 operations, each rounded on its own: e1 = v1 - v0, e2 = v2 - v0,
// n = cross(e1, e2) (linear's component order), nn = (nx^2 + ny^2) + nz^2.
struct TriangleNormal {
    float n[3], nn;
    bool vertices_finite, finite;      // every vertex / every edge, the normal and nn
};

PTMI_HD TriangleNormal triangle_normal(const float v0[3], const float v1[3], const float v2[3])
{
    TriangleNormal r;
    const float e1[3] = {v1[0] - v0[0], v1[1] - v0[1], v1[2] - v0[2]};
    const float e2[3] = {v2[0] - v0[0], v2[1] - v0[1], v2[2] - v0[2]};
    r.n[0] = e1[1] * e2[2] - e1[2] * e2[1];
    r.n[1] = e1[2] * e2[0] - e1[0] * e2[2];
    r.n[2] = e1[0] * e2[1] - e1[1] * e2[0];
    r.nn = (r.n[0] * r.n[0] + r.n[1] * r.n[1]) + r.n[2] * r.n[2];
    r.vertices_finite = true; r.finite = finite_f32(r.nn);
    for (int a = 0; a < 3; ++a) {
        r.vertices_finite = r.vertices_finite && finite_f32(v0[a]) && finite_f32(v1[a]) && finite_f32(v2[a]);
        r.finite = r.finite && finite_f32(e1[a]) && finite_f32(e2[a]) && finite_f32(r.n[a]);
    }
    return r;
}

// What the refit's first kernel reports (ptmi_mesh_refit.hip -> ptmi_scene.cpp): result[kRefitError] = the smallest (triangle << 2 | code)
// of a refused triangle, all ones when there is none; the box of the leaf triangles' vertices as order-preserving integer images.
enum { kRefitError = 0, kRefitLo = 1, kRefitHi = 4, kRefitWords = 8 };
enum { kRefitBadVertex = 0, kRefitBadNormal = 1, kRefitGainsArea = 2 };
PTMI_HD uint32_t ordered_image(float f) { const uint32_t u = f2u(f); return (u & 0x80000000u) ? ~u : (u | 0x80000000u); }
PTMI_HD float ordered_value(uint32_t k) { return u2f((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

}  // namespace ptmi
