// ptmi_mesh.h -- the host side of the mesh scene (ptmi_set_scene_mesh): the hierarchy over the triangles, built by ptmi_mesh.cpp.
#pragma once

#include <stdint.h>

#include <string>
#include <vector>

#include "../../include/ptmi.h"

namespace ptmi {

struct MeshBuild {
    std::vector<ptmi_bvh_node> nodes;   // node 0 is the root
    std::vector<int32_t> order;         // leaf order -> original triangle index (triangles of non-zero area only)
    std::vector<float> records;         // 12 floats per triangle BY ORIGINAL INDEX: (v0, nx) (v1, ny) (v2, nz); zero area: a NaN normal
    float lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0};   // box of the kept triangles' vertices
};

// PTMI_OK, PTMI_ELIMIT (too many triangles) or PTMI_EINVAL (non-finite vertex or material data); `why` says which.
int mesh_build(const ptmi_triangle *triangles, int n_triangles, MeshBuild &out, std::string *why);

}  // namespace ptmi
