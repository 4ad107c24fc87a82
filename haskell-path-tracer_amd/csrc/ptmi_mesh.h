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

// The same for ptmi_mesh_layout_morton, the host twin of ptmi_set_mesh_triangles (ptmi_mesh_morton.h): leaf order by Morton key, the
// topology a function of the kept count, mesh_refit's boxes.
int mesh_build_morton(const ptmi_triangle *triangles, int n_triangles, MeshBuild &out, std::string *why);

// What the device refit (ptmi_update_mesh_vertices, ptmi_mesh_refit.hip) needs of a built hierarchy besides the hierarchy itself.
struct MeshRefitPlan {
    std::vector<int32_t> leaf_pos;      // per original triangle: its position in the leaf order, -1 when it is in no leaf (zero area)
    std::vector<int32_t> level_nodes;   // every node, the deepest level first: children always come before their parent
    std::vector<int32_t> level_first;   // launches + 1 offsets into level_nodes, one launch per level
};
void mesh_refit_plan(const MeshBuild &built, int n_triangles, MeshRefitPlan &out);

// ptmi_mesh_refit_layout: the boxes of `nodes` recomputed for the moved `triangles`, topology (`ref`, `order`) kept.
// PTMI_OK or PTMI_EINVAL; `why` says which triangle or which part of the topology.
int mesh_refit(const ptmi_triangle *triangles, int n_triangles, ptmi_bvh_node *nodes, int n_nodes, const int32_t *order, int n_kept, std::string *why);

}  // namespace ptmi
