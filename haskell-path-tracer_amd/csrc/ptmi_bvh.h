// ptmi_bvh.h -- the host side of the BVH scene (ptmi_set_scene_bvh): the hierarchy over the spheres, built by ptmi_bvh.cpp.
#pragma once

#include <stdint.h>

#include <string>
#include <vector>

#include "../../include/ptmi.h"

namespace ptmi {

struct BvhBuild {
    std::vector<ptmi_bvh_node> nodes;   // node 0 is the root
    std::vector<int32_t> order;         // leaf order -> original sphere index
    float lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0};   // box of the sphere CENTRES (the traversal's bound on |centre - origin|)
};

// PTMI_OK, PTMI_ELIMIT (too many spheres) or PTMI_EINVAL (non-finite sphere data); `why` says which.
int bvh_build(const ptmi_sphere *spheres, int n_spheres, BvhBuild &out, std::string *why);
const char *bvh_sphere_refusal(const ptmi_sphere &sphere);   // why no box can bound this sphere, or NULL

// The same for ptmi_bvh_layout_morton, the host twin of ptmi_set_bvh_spheres: leaf order by the Morton key of the centres
// (ptmi_mesh_morton.h), the topology a function of the count, bvh_refit's boxes; it also refuses what the scene calls refuse in a
// sphere's material.
int bvh_build_morton(const ptmi_sphere *spheres, int n_spheres, BvhBuild &out, std::string *why);
// ... and for ptmi_bvh_layout_spatial, the twin of the spatial device build (PTMI_BVH_BUILD_SPATIAL; ptmi_bvh_spatial.h): the same refusals,
// keys in cubic cells, splits at the highest differing key bit within the depth limit, nodes numbered breadth-first.  *fallbacks (may be
// NULL): how many nodes took the equal-count split.
int bvh_build_spatial(const ptmi_sphere *spheres, int n_spheres, BvhBuild &out, std::string *why, int *fallbacks);

// What the device refit (ptmi_update_spheres, ptmi_bvh_refit.hip) needs of a hierarchy besides the hierarchy itself.
struct BvhLevelPlan {
    std::vector<int32_t> level_nodes;   // every node, the deepest level first: children always come before their parent
    std::vector<int32_t> level_first;   // launches + 1 offsets into level_nodes, one launch per level
};
void bvh_level_plan(const std::vector<ptmi_bvh_node> &nodes, BvhLevelPlan &out);

// ptmi_bvh_refit_layout: the boxes and inv_2r of `nodes` recomputed for the moved `spheres`, topology (`ref`, `order`) kept.
// PTMI_OK or PTMI_EINVAL; `why` says which sphere or which part of the topology.
int bvh_refit(const ptmi_sphere *spheres, int n_spheres, ptmi_bvh_node *nodes, int n_nodes, const int32_t *order, std::string *why);

}  // namespace ptmi
