// ptmi_mesh_morton.h -- the leaf order and the topology of a triangle hierarchy built WITHOUT geometry decisions on the host
// (ptmi_set_mesh_triangles, ptmi_mesh_layout_morton), ONE definition for the host twin (ptmi_mesh.cpp) and the device build
// (ptmi_mesh_build.hip): the two are bit-equal because they run these operations.
//
// Key of a kept (non-zero-area) triangle, per axis a, with lo / hi the f32 box of the kept triangles' vertices, every operation in f64
// and rounded on its own (the library is compiled without contraction), in exactly this order:
//     s   = ((double)v0[a] + (double)v1[a]) + (double)v2[a]
//     num = (s - 3.0 * (double)lo[a]) * 16384.0
//     den = 3.0 * ((double)hi[a] - (double)lo[a])
//     q   = hi[a] == lo[a] ? 0 : min(16383, (int)floor(num / den))          (IEEE division)
// and the 42-bit Morton interleave of (qx, qy, qz): bit i of qx is bit 3 i + 2 of the key, of qy bit 3 i + 1, of qz bit 3 i.
// The leaf order ascends by (key, original index).
//
// Topology: a pure function of the kept count k -- mesh_build's Builder::fill / child with the geometry taken out: the range [b, e)
// splits at b + n / 2 while n > PTMI_BVH_LEAF_MAX, the same reference encoding, children after their parent, an empty child -1 with
// the box (0, -1).  The depth is mesh_build's (ceil(log2(k / PTMI_BVH_LEAF_MAX)) levels: 20 at 2^22), so the walk's stack bound holds.
// The boxes are the refit's (ptmi_mesh_box.h), over this topology.
#pragma once

#include <vector>

#include "../../include/ptmi.h"
#include "ptmi_mesh_box.h"

namespace ptmi {

constexpr int kMortonBits = 14;                           // per axis
constexpr int kMortonKeyBits = 3 * kMortonBits;           // 42; a triangle in no leaf sorts behind every key: bit 42
constexpr uint64_t kMortonNoLeaf = 1ull << kMortonKeyBits;

PTMI_HD uint64_t morton_spread(uint32_t q)                // bit i -> bit 3 i, 14 bits
{
    uint64_t r = 0;
    for (int i = 0; i < kMortonBits; ++i) r |= (uint64_t)((q >> i) & 1u) << (3 * i);
    return r;
}

PTMI_HD uint32_t morton_axis(float v0, float v1, float v2, float lo, float hi)
{
    if (hi == lo) return 0u;
    const double s = ((double)v0 + (double)v1) + (double)v2;
    const double num = (s - 3.0 * (double)lo) * 16384.0;
    const double den = 3.0 * ((double)hi - (double)lo);
    const int q = (int)__builtin_floor(num / den);
    return (uint32_t)(q < 16383 ? q : 16383);
}

PTMI_HD uint64_t morton_key(const float v0[3], const float v1[3], const float v2[3], const float lo[3], const float hi[3])
{
    return (morton_spread(morton_axis(v0[0], v1[0], v2[0], lo[0], hi[0])) << 2) | (morton_spread(morton_axis(v0[1], v1[1], v2[1], lo[1], hi[1])) << 1) |
           morton_spread(morton_axis(v0[2], v1[2], v2[2], lo[2], hi[2]));
}

// What the build's first kernel reports (ptmi_mesh_build.hip -> ptmi_scene.cpp), in the refit's form (ptmi_mesh_box.h): the smallest
// (triangle << 2 | code) of a refused triangle, all ones when there is none; the box of the kept triangles' vertices as ordered images;
// how many triangles are kept; whether any is GLASS.  All ones in [0, kBuildHi), zero behind, at launch.
enum { kBuildError = 0, kBuildLo = 1, kBuildHi = 4, kBuildKept = 7, kBuildGlass = 8, kBuildWords = 12 };
enum { kBuildBadVertex = 0, kBuildBadMaterial = 1, kBuildBadNormal = 2, kBuildBadTag = 3 };

// The topology for k kept triangles: every node with its references, boxes zero but an empty child's (0, -1); node 0 is the root.
namespace morton_detail {
inline void fill(std::vector<ptmi_bvh_node> &nodes, int id, int b, int e);
inline int32_t child(std::vector<ptmi_bvh_node> &nodes, int b, int e)
{
    const int n = e - b;
    if (n <= PTMI_BVH_LEAF_MAX) return n == 0 ? -1 : -1 - (int32_t)(((uint32_t)b << 8) | (uint32_t)n);
    const int32_t ref = (int32_t)nodes.size();
    nodes.emplace_back();
    fill(nodes, ref, b, e);
    return ref;
}
inline void fill(std::vector<ptmi_bvh_node> &nodes, int id, int b, int e)
{
    const int n = e - b;
    const int mid = n > PTMI_BVH_LEAF_MAX ? b + n / 2 : e;
    ptmi_bvh_node nd{};
    nd.ref[0] = child(nodes, b, mid);
    nd.ref[1] = child(nodes, mid, e);
    for (int c = 0; c < 2; ++c)
        if (nd.ref[c] == -1)
            for (int a = 0; a < 3; ++a) nd.half[c][a] = -1.0f;
    nodes[(size_t)id] = nd;
}
}  // namespace morton_detail

inline void morton_topology(int k, std::vector<ptmi_bvh_node> &nodes)
{
    nodes.clear();
    nodes.reserve((size_t)(k / 2 > 1 ? k / 2 : 1));
    nodes.emplace_back();
    morton_detail::fill(nodes, 0, 0, k);
}

}  // namespace ptmi
