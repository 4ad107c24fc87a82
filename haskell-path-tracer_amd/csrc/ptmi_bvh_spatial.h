// ptmi_bvh_spatial.h -- the key and the split of the SPATIAL sphere build (PTMI_OPT_BVH_DEVICE_BUILD = PTMI_BVH_BUILD_SPATIAL;
// ptmi_bvh_layout_spatial), ONE definition for the host twin (ptmi_bvh.cpp: bvh_build_spatial) and the device build (ptmi_bvh_lbvh.hip):
// the two are bit-equal because they run these operations.
//
// Key of a centre c, with lo / hi the f32 box of all centres, every operation in f64 and rounded on its own:
//     den = max over a of ((double)hi[a] - (double)lo[a])                               (ONE denominator: the cells are cubes)
//     q   = den == 0 ? 0 : min(16383, (int)floor((((double)c[a] - (double)lo[a]) * 16384.0) / den))      (IEEE division)
// and ptmi_mesh_morton.h's 42-bit interleave of (qx, qy, qz).  An axis shorter than the longest uses the low part of its 14 bits only.
// The leaf order ascends by (key, original index).
//
// Topology, top-down over the sorted keys; the root is level 0 and holds [0, n).  A range of at most PTMI_BVH_LEAF_MAX is a leaf.  The
// node of [b, e) at level L splits at m:
//   * spatial: h = the highest bit in which key[b] and key[e - 1] differ, m = the first position whose key has bit h set (b < m < e);
//   * taken only if L + 1 + spatial_levels(max(m - b, e - m)) <= PTMI_BVH_MAX_DEPTH, spatial_levels(k) being the inner levels of
//     morton_topology's equal-count subtree over k items;
//   * otherwise, and when all keys of the range are equal, m = b + (e - b) / 2 -- which always fits: by induction a node at level L
//     holds at most a range whose equal-count subtree ends at level PTMI_BVH_MAX_DEPTH - 1 (spatial_levels(2^22) = 20 at the root).
// So no inner node lies below level PTMI_BVH_MAX_DEPTH - 1 and no leaf holds more than PTMI_BVH_LEAF_MAX spheres.
// Nodes are numbered breadth-first: level by level, within a level by ascending b.
#pragma once

#include "ptmi_mesh_morton.h"

namespace ptmi {

PTMI_HD double spatial_den(const float lo[3], const float hi[3])
{
    double den = (double)hi[0] - (double)lo[0];
    den = box_max(den, (double)hi[1] - (double)lo[1]);
    den = box_max(den, (double)hi[2] - (double)lo[2]);
    return den;
}

PTMI_HD uint32_t spatial_axis(float c, float lo, double den)
{
    if (den == 0.0) return 0u;
    const double num = ((double)c - (double)lo) * 16384.0;
    const int q = (int)__builtin_floor(num / den);
    return (uint32_t)(q < 16383 ? q : 16383);
}

PTMI_HD uint64_t spatial_key(const float c[3], const float lo[3], double den)
{
    return (morton_spread(spatial_axis(c[0], lo[0], den)) << 2) | (morton_spread(spatial_axis(c[1], lo[1], den)) << 1) |
           morton_spread(spatial_axis(c[2], lo[2], den));
}

// the inner levels of the equal-count subtree over k items (its larger half holds k - k / 2)
PTMI_HD int spatial_levels(int k)
{
    int levels = 0;
    for (; k > PTMI_BVH_LEAF_MAX; k -= k / 2) ++levels;
    return levels;
}

// Where the node of [b, e) at `level` splits (e - b > PTMI_BVH_LEAF_MAX; key ascends within the range).  *fallback (may be null): 1 when
// the equal-count split was taken.
PTMI_HD int spatial_split(const uint64_t *key, int b, int e, int level, int *fallback = nullptr)
{
    const uint64_t differ = key[b] ^ key[e - 1];
    if (fallback) *fallback = 1;
    if (differ != 0) {
        const int h = 63 - __builtin_clzll(differ);
        int clear = b, set = e - 1;                       // bit h of key[clear] is 0, of key[set] 1: the bits above h agree in the range
        while (set - clear > 1) {
            const int mid = clear + (set - clear) / 2;
            if ((key[mid] >> h) & 1u) set = mid; else clear = mid;
        }
        const int larger = set - b > e - set ? set - b : e - set;
        if (level + 1 + spatial_levels(larger) <= PTMI_BVH_MAX_DEPTH) {
            if (fallback) *fallback = 0;
            return set;
        }
    }
    return b + (e - b) / 2;
}

// the reference to the leaf of positions [b, e) of the leaf order (-1: an empty child)
PTMI_HD int32_t spatial_leaf_ref(int b, int e) { return e == b ? -1 : -1 - (int32_t)(((uint32_t)b << 8) | (uint32_t)(e - b)); }

// What the device build reports to the host (ptmi_bvh_lbvh.hip -> ptmi_scene.cpp): the number of nodes of every level, 0 ..
// PTMI_BVH_MAX_DEPTH - 1, and how many nodes took the equal-count split.
enum { kSpatialFallbacks = PTMI_BVH_MAX_DEPTH, kSpatialWords = PTMI_BVH_MAX_DEPTH + 1 };

// how many nodes a level can hold at most: an inner node holds more than PTMI_BVH_LEAF_MAX spheres, the nodes of a level are disjoint
inline int spatial_level_bound(int n, int level)
{
    const long long by_count = n / (PTMI_BVH_LEAF_MAX + 1) > 1 ? n / (PTMI_BVH_LEAF_MAX + 1) : 1, by_level = 1ll << level;
    return (int)(by_level < by_count ? by_level : by_count);
}
// ... and a tree at most (every split leaves both sides something): the capacity the build works in
inline int spatial_node_bound(int n) { return n > PTMI_BVH_LEAF_MAX + 1 ? n - PTMI_BVH_LEAF_MAX : 1; }
// the levels a tree of n spheres can have (every level of a chain takes a sphere)
inline int spatial_level_limit(int n) { return n - PTMI_BVH_LEAF_MAX < 1 ? 1 : (n - PTMI_BVH_LEAF_MAX < PTMI_BVH_MAX_DEPTH ? n - PTMI_BVH_LEAF_MAX : PTMI_BVH_MAX_DEPTH); }

}  // namespace ptmi
