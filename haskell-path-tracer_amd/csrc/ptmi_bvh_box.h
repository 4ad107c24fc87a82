// ptmi_bvh_box.h -- the arithmetic of the sphere hierarchy's boxes, ONE definition for the host build (ptmi_bvh.cpp: bvh_build), the host
// twins of the device calls (ptmi_bvh_refit_layout, ptmi_bvh_layout_morton) and the device kernels (ptmi_bvh_refit.hip,
// ptmi_bvh_build.hip): a refit is bit for bit the build's boxes because it runs the build's operations.  Everything is f64 arithmetic on
// f32 data, each operation rounded on its own (the library is compiled without contraction); min / max are ptmi_mesh_box.h's, std::min /
// std::max written out (the FIRST of two equal operands is kept); the division is the IEEE one on host and device.  The padding is
// derived in ptmi_bvh.cpp ("PADDING").
#pragma once

#include "ptmi_mesh_box.h"

namespace ptmi {

constexpr double kBvhRelPad = 1.0 / 256.0, kBvhAbsPad = 1.0 / 1048576.0;

// what a sphere's box is widened by beyond its centre: |r| (1 + 2^-8) + 2^-20 max(|centre|, |r|)
PTMI_HD double bvh_pad_of(const float position[3], float radius)
{
    const double r = __builtin_fabs((double)radius);
    double m = __builtin_fabs((double)position[0]);
    m = box_max(m, __builtin_fabs((double)position[1]));
    m = box_max(m, __builtin_fabs((double)position[2]));
    m = box_max(m, r);
    return r * (1.0 + kBvhRelPad) + kBvhAbsPad * m;
}

// (float)v, or its upper neighbour when that lies below v
PTMI_HD float bvh_round_up(double v) { return box_round_up(v); }

// the stored (centre, half) of a box holding [lo, hi]: centre = (float)(0.5 (lo + hi)), half rounded up
PTMI_HD void bvh_store(float center[3], float half[3], const double lo[3], const double hi[3]) { box_store(center, half, lo, hi); }

// A leaf child's box and smallest |radius| grow by one sphere: the union of the padded spheres
PTMI_HD void bvh_leaf_join(double lo[3], double hi[3], double &r_min, const float position[3], float radius)
{
    const double pad = bvh_pad_of(position, radius);
    for (int a = 0; a < 3; ++a) {
        lo[a] = box_min(lo[a], (double)position[a] - pad);
        hi[a] = box_max(hi[a], (double)position[a] + pad);
    }
    r_min = box_min(r_min, __builtin_fabs((double)radius));
}

// a leaf child's inv_2r = round_up(1 / (2 r_min)), +inf at r_min == 0
PTMI_HD float bvh_leaf_inv_2r(double r_min) { return r_min > 0.0 ? bvh_round_up(1.0 / (2.0 * r_min)) : __builtin_inff(); }

// An inner child's box: the union of that node's two boxes AS STORED (boxes nest exactly); its inv_2r: their maximum.  ref0 / ref1,
// inv0 / inv1: the node's references and inv_2r; an empty child (-1) adds nothing.
PTMI_HD void bvh_inner_box(double lo[3], double hi[3], const float center[2][3], const float half[2][3], int32_t ref0, int32_t ref1)
{
    box_empty(lo, hi);
    if (ref0 != -1) box_join_stored(lo, hi, center[0], half[0]);
    if (ref1 != -1) box_join_stored(lo, hi, center[1], half[1]);
}
PTMI_HD float bvh_inner_inv_2r(float inv0, float inv1, int32_t ref0, int32_t ref1)
{
    const float a = ref0 == -1 ? 0.0f : inv0, b = ref1 == -1 ? 0.0f : inv1;
    return a < b ? b : a;                                  // std::max(a, b)
}

// the empty child: the box (0, -1), inv_2r = 0
PTMI_HD void bvh_empty_child(float center[3], float half[3], float &inv_2r)
{
    for (int a = 0; a < 3; ++a) { center[a] = 0.0f; half[a] = -1.0f; }
    inv_2r = 0.0f;
}

// What the first kernel of ptmi_update_spheres / ptmi_set_bvh_spheres reports (ptmi_bvh_refit.hip, ptmi_bvh_build.hip -> ptmi_scene.cpp),
// in the mesh calls' form: result[kSphError] = the smallest (sphere << 2 | code) of a refused sphere, all ones when there is none; the box
// of the CENTRES as order-preserving integer images (ordered_image); whether any sphere is GLASS.  All ones in [0, kSphHi), zero behind,
// at launch.
enum { kSphError = 0, kSphLo = 1, kSphHi = 4, kSphGlass = 7, kSphWords = 8 };
enum { kSphBadGeometry = 0, kSphBadMaterial = 1, kSphBadTag = 2 };

}  // namespace ptmi
