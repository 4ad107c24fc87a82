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

}  // namespace ptmi
