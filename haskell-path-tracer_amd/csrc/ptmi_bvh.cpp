// ptmi_bvh.cpp -- the bounding-volume hierarchy of a BVH scene (ptmi_set_scene_bvh, ptmi_bvh_layout), host code.
//
// A binary hierarchy over the spheres, split at the MEDIAN of the sphere centres along the longest axis of their bounds (ties by
// original index, so the build is a pure function of its input), leaves of at most PTMI_BVH_LEAF_MAX spheres.  Median splits keep
// the tree balanced: ceil(log2(n / 4)) levels of inner nodes, 20 for PTMI_MAX_BVH_SPHERES, within the PTMI_BVH_MAX_DEPTH levels the
// device's traversal stack holds.  (Should a range still be too big at that level it becomes one larger leaf, up to 255 spheres.)
//
// PADDING.  The device's sphere test (check_hit's: tca = l.d, d2 = l.l - tca^2, x = r^2 - d2, t = tca - sqrt x) is a float
// computation that can ACCEPT a ray which in exact arithmetic passes just outside the sphere, and a box that did not contain that
// ray's point would prune a hit the linear fold finds.  The bound is split in two (DESIGN.md "BVH scenes" has the derivation):
//   * what scales with the sphere -- the rounding of r^2, and |d|^2 != 1 acting on r^2 (|(|d|^2 - 1)| <= 2^-12 for every ray the
//     hierarchy serves) -- is a RELATIVE pad of the radius here: |r| 2^-8, and an absolute 2^-20 max(|centre|, |r|) for the
//     rounding of centre - origin and of the box itself;
//   * what scales with the distance P from the ray origin to the scene (the cancellation in l.l - tca^2) is a margin the traversal
//     adds per ray (check_hit_bvh), using the smallest radius under each child (ptmi_bvh_node.inv_2r).
#include "ptmi_bvh.h"
#include "ptmi_bvh_box.h"
#include "ptmi_bvh_spatial.h"
#include "ptmi_mesh_morton.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <numeric>

namespace ptmi {

namespace {

constexpr int kLeafCap = 255;                    // what a leaf reference can encode
                                                 // (the box arithmetic is ptmi_bvh_box.h's, shared with the refit and the device)

struct Builder {
    const ptmi_sphere *s;
    std::vector<int32_t> idx;
    std::vector<ptmi_bvh_node> nodes;

    // child c of node `nd` is inner node `inner`: its box is the union of that node's two boxes as STORED (so that boxes nest exactly)
    void set_box_of_node(ptmi_bvh_node &nd, int c, int inner) const
    {
        const ptmi_bvh_node &in = nodes[(size_t)inner];
        double lo[3], hi[3];
        bvh_inner_box(lo, hi, in.center, in.half, in.ref[0], in.ref[1]);
        bvh_store(nd.center[c], nd.half[c], lo, hi);
        nd.inv_2r[c] = bvh_inner_inv_2r(in.inv_2r[0], in.inv_2r[1], in.ref[0], in.ref[1]);
    }

    // child c of node `nd` is the leaf idx[b, e)
    void set_box(ptmi_bvh_node &nd, int c, int b, int e) const
    {
        if (b == e) {
            bvh_empty_child(nd.center[c], nd.half[c], nd.inv_2r[c]);
            return;
        }
        double lo[3], hi[3];
        box_empty(lo, hi);
        double r_min = std::numeric_limits<double>::infinity();
        for (int k = b; k < e; ++k) bvh_leaf_join(lo, hi, r_min, s[idx[k]].position, s[idx[k]].radius);
        bvh_store(nd.center[c], nd.half[c], lo, hi);
        nd.inv_2r[c] = bvh_leaf_inv_2r(r_min);
    }

    // the reference to a child holding idx[b, e) at `level` (the level the child would have as an inner node)
    bool child(int b, int e, int level, int32_t &ref)
    {
        const int n = e - b;
        if (n <= PTMI_BVH_LEAF_MAX || level >= PTMI_BVH_MAX_DEPTH) {
            if (n > kLeafCap) return false;
            ref = n == 0 ? -1 : -1 - (int32_t)(((uint32_t)b << 8) | (uint32_t)n);      // (-1: an empty child)
            return true;
        }
        ref = (int32_t)nodes.size();
        nodes.emplace_back();
        return fill(ref, b, e, level);
    }

    bool fill(int id, int b, int e, int level)
    {
        const int n = e - b;
        int mid = e;                                 // (n <= leaf size: everything in child 0, child 1 empty -- the root of a small scene)
        if (n > PTMI_BVH_LEAF_MAX) {
            float lo[3], hi[3];
            for (int a = 0; a < 3; ++a) { lo[a] = std::numeric_limits<float>::infinity(); hi[a] = -lo[a]; }
            for (int k = b; k < e; ++k)
                for (int a = 0; a < 3; ++a) { lo[a] = std::min(lo[a], s[idx[k]].position[a]); hi[a] = std::max(hi[a], s[idx[k]].position[a]); }
            int axis = 0;
            for (int a = 1; a < 3; ++a)
                if ((double)hi[a] - lo[a] > (double)hi[axis] - lo[axis]) axis = a;
            mid = b + n / 2;
            const ptmi_sphere *sp = s;
            std::nth_element(idx.begin() + b, idx.begin() + mid, idx.begin() + e, [sp, axis](int32_t x, int32_t y) {
                const float px = sp[x].position[axis], py = sp[y].position[axis];
                return px < py || (px == py && x < y);
            });
        }
        int32_t r0 = 0, r1 = 0;
        if (!child(b, mid, level + 1, r0) || !child(mid, e, level + 1, r1)) return false;
        ptmi_bvh_node nd;                            // (after the recursion, whose nodes it reads: `nodes` may have moved)
        std::memset(&nd, 0, sizeof nd);
        nd.ref[0] = r0; nd.ref[1] = r1;
        if (r0 >= 0) set_box_of_node(nd, 0, r0); else set_box(nd, 0, b, mid);
        if (r1 >= 0) set_box_of_node(nd, 1, r1); else set_box(nd, 1, mid, e);
        nodes[(size_t)id] = nd;
        return true;
    }
};

}  // namespace

int bvh_build(const ptmi_sphere *spheres, int n, BvhBuild &out, std::string *why)
{
    auto refuse = [&](int code, const char *msg) { if (why) *why = msg; return code; };
    if (n < 0 || (n > 0 && !spheres)) return refuse(PTMI_EINVAL, "bad sphere arguments");
    if (n > PTMI_MAX_BVH_SPHERES) return refuse(PTMI_ELIMIT, "more spheres than PTMI_MAX_BVH_SPHERES");
    for (int i = 0; i < n; ++i)
        if (bvh_sphere_refusal(spheres[i])) return refuse(PTMI_EINVAL, "a sphere's position, radius or radius^2 is not finite: a box cannot bound it");
    Builder bd;
    bd.s = spheres;
    bd.idx.resize((size_t)n);
    std::iota(bd.idx.begin(), bd.idx.end(), 0);
    bd.nodes.reserve((size_t)std::max(1, n / 2));
    bd.nodes.emplace_back();
    if (!bd.fill(0, 0, n, 0)) return refuse(PTMI_ELIMIT, "a leaf at the depth limit would hold more than 255 spheres");
    for (int a = 0; a < 3; ++a) { out.lo[a] = 0.0f; out.hi[a] = 0.0f; }
    if (n > 0) {
        for (int a = 0; a < 3; ++a) { out.lo[a] = std::numeric_limits<float>::infinity(); out.hi[a] = -out.lo[a]; }
        for (int i = 0; i < n; ++i)
            for (int a = 0; a < 3; ++a) { out.lo[a] = std::min(out.lo[a], spheres[i].position[a]); out.hi[a] = std::max(out.hi[a], spheres[i].position[a]); }
    }
    out.nodes = std::move(bd.nodes);
    out.order = std::move(bd.idx);
    return PTMI_OK;
}

void bvh_level_plan(const std::vector<ptmi_bvh_node> &nodes, BvhLevelPlan &out)
{
    // children have larger ids than their parent (child() appends before it fills): one ascending pass gives every level
    const size_t n = nodes.size();
    std::vector<int32_t> level(n, 0);
    int deepest = 0;
    for (size_t id = 0; id < n; ++id)
        for (int c = 0; c < 2; ++c)
            if (nodes[id].ref[c] >= 0) {
                level[(size_t)nodes[id].ref[c]] = level[id] + 1;
                deepest = std::max(deepest, level[id] + 1);
            }
    std::vector<int32_t> count((size_t)deepest + 2, 0);
    for (size_t id = 0; id < n; ++id) ++count[(size_t)(deepest - level[id]) + 1];
    for (size_t k = 1; k < count.size(); ++k) count[k] += count[k - 1];
    out.level_first = count;
    out.level_nodes.assign(n, 0);
    for (size_t id = 0; id < n; ++id) out.level_nodes[(size_t)count[(size_t)(deepest - level[id])]++] = (int32_t)id;
}

const char *bvh_sphere_refusal(const ptmi_sphere &sp)
{
    const float r2 = sp.radius * sp.radius;     // what the device tests against (pack_scene)
    if (!std::isfinite(sp.position[0]) || !std::isfinite(sp.position[1]) || !std::isfinite(sp.position[2]) || !std::isfinite(sp.radius) ||
        !std::isfinite(r2))
        return "its position, radius or radius^2 is not finite: a box cannot bound it";
    return nullptr;
}

int bvh_refit(const ptmi_sphere *spheres, int n, ptmi_bvh_node *nodes, int n_nodes, const int32_t *order, std::string *why)
{
    auto refuse = [&](const std::string &msg) { if (why) *why = msg; return (int)PTMI_EINVAL; };
    if (n < 0 || n_nodes < 1 || !nodes || (n > 0 && (!spheres || !order))) return refuse("bad refit arguments");
    // the topology must be one ptmi_bvh_layout can have made: every node but the root referred to once, by a node before it; the
    // leaves a partition of the leaf order; the leaf order a permutation of the spheres
    long long inner = 0, in_leaves = 0;
    for (int id = 0; id < n_nodes; ++id)
        for (int c = 0; c < 2; ++c) {
            const int32_t ref = nodes[id].ref[c];
            if (ref >= 0) {
                if (ref <= id || ref >= n_nodes) return refuse("the nodes are not a hierarchy of ptmi_bvh_layout (a child reference out of range: wrong n_nodes?)");
                ++inner;
            } else if (ref != -1) {
                const uint32_t v = (uint32_t)(-1 - ref);
                if ((long long)(v >> 8) + (v & 255u) > n) return refuse("a leaf lies beyond the leaf order (wrong n_spheres?)");
                in_leaves += v & 255u;
            }
        }
    if (inner != n_nodes - 1 || in_leaves != n) return refuse("the nodes and the leaf order do not belong together (wrong n_nodes or n_spheres?)");
    std::vector<char> seen((size_t)n, 0);
    for (int k = 0; k < n; ++k) {
        if (order[k] < 0 || order[k] >= n || seen[(size_t)order[k]]) return refuse("the leaf order is not a permutation of the spheres");
        seen[(size_t)order[k]] = 1;
    }
    for (int i = 0; i < n; ++i)
        if (const char *bad = bvh_sphere_refusal(spheres[i])) return refuse("sphere " + std::to_string(i) + ": " + bad);
    for (int id = n_nodes - 1; id >= 0; --id) {
        ptmi_bvh_node &nd = nodes[id];
        for (int c = 0; c < 2; ++c) {
            const int32_t ref = nd.ref[c];
            if (ref == -1) { bvh_empty_child(nd.center[c], nd.half[c], nd.inv_2r[c]); continue; }
            double lo[3], hi[3];
            if (ref >= 0) {
                const ptmi_bvh_node &in = nodes[ref];
                bvh_inner_box(lo, hi, in.center, in.half, in.ref[0], in.ref[1]);
                nd.inv_2r[c] = bvh_inner_inv_2r(in.inv_2r[0], in.inv_2r[1], in.ref[0], in.ref[1]);
            } else {
                const uint32_t v = (uint32_t)(-1 - ref);
                double r_min = std::numeric_limits<double>::infinity();
                box_empty(lo, hi);
                for (uint32_t k = v >> 8; k < (v >> 8) + (v & 255u); ++k) bvh_leaf_join(lo, hi, r_min, spheres[order[k]].position, spheres[order[k]].radius);
                nd.inv_2r[c] = bvh_leaf_inv_2r(r_min);
            }
            bvh_store(nd.center[c], nd.half[c], lo, hi);
        }
    }
    return PTMI_OK;
}

// ptmi_bvh_layout_morton / the specification of ptmi_set_bvh_spheres: bvh_build's and the scene calls' refusals; the leaf order by
// (Morton key of the centre, index) and the topology of the count (ptmi_mesh_morton.h); the boxes by the refit over that topology.
// what both device builds refuse, and the box of the centres
static int device_build_front(const ptmi_sphere *spheres, int n, BvhBuild &out, std::string *why)
{
    auto refuse = [&](int code, const std::string &msg) { if (why) *why = msg; return code; };
    if (n < 0 || (n > 0 && !spheres)) return refuse(PTMI_EINVAL, "bad sphere arguments");
    if (n > PTMI_MAX_BVH_SPHERES) return refuse(PTMI_ELIMIT, "more spheres than PTMI_MAX_BVH_SPHERES");
    for (int i = 0; i < n; ++i) {
        const ptmi_sphere &sp = spheres[i];
        const std::string who = "sphere " + std::to_string(i) + ": ";
        if (const char *bad = bvh_sphere_refusal(sp)) return refuse(PTMI_EINVAL, who + bad);
        if (!std::isfinite(sp.color[0]) || !std::isfinite(sp.color[1]) || !std::isfinite(sp.color[2]) || !std::isfinite(sp.illuminance) ||
            !std::isfinite(sp.brdf_param))
            return refuse(PTMI_EINVAL, who + "its colour, illuminance or brdf_param is not finite");
        if (sp.brdf_tag < PTMI_MATTE || sp.brdf_tag > PTMI_GLASS) return refuse(PTMI_EINVAL, who + "unknown brdf_tag");
    }
    for (int a = 0; a < 3; ++a) { out.lo[a] = 0.0f; out.hi[a] = 0.0f; }
    if (n > 0) {
        for (int a = 0; a < 3; ++a) { out.lo[a] = std::numeric_limits<float>::infinity(); out.hi[a] = -out.lo[a]; }
        for (int i = 0; i < n; ++i)
            for (int a = 0; a < 3; ++a) { out.lo[a] = std::min(out.lo[a], spheres[i].position[a]); out.hi[a] = std::max(out.hi[a], spheres[i].position[a]); }
    }
    return PTMI_OK;
}

int bvh_build_morton(const ptmi_sphere *spheres, int n, BvhBuild &out, std::string *why)
{
    if (int rc = device_build_front(spheres, n, out, why)) return rc;
    std::vector<uint64_t> key((size_t)n, 0);
    for (int i = 0; i < n; ++i) key[(size_t)i] = morton_key(spheres[i].position, spheres[i].position, spheres[i].position, out.lo, out.hi);
    out.order.resize((size_t)n);
    std::iota(out.order.begin(), out.order.end(), 0);
    const uint64_t *kp = key.data();
    std::sort(out.order.begin(), out.order.end(), [kp](int32_t x, int32_t y) { return kp[x] < kp[y] || (kp[x] == kp[y] && x < y); });
    morton_topology(n, out.nodes);
    return bvh_refit(spheres, n, out.nodes.data(), (int)out.nodes.size(), out.order.data(), why);
}

// ptmi_bvh_layout_spatial / the specification of ptmi_set_bvh_spheres under PTMI_BVH_BUILD_SPATIAL (ptmi_bvh_spatial.h): the same
// refusals; the leaf order by (key in cubic cells, index); spatial splits with the depth guard, numbered breadth-first; the refit's boxes.
int bvh_build_spatial(const ptmi_sphere *spheres, int n, BvhBuild &out, std::string *why, int *fallbacks)
{
    if (int rc = device_build_front(spheres, n, out, why)) return rc;
    const double den = spatial_den(out.lo, out.hi);
    std::vector<uint64_t> key((size_t)n, 0);
    for (int i = 0; i < n; ++i) key[(size_t)i] = spatial_key(spheres[i].position, out.lo, den);
    out.order.resize((size_t)n);
    std::iota(out.order.begin(), out.order.end(), 0);
    const uint64_t *kp = key.data();
    std::sort(out.order.begin(), out.order.end(), [kp](int32_t x, int32_t y) { return kp[x] < kp[y] || (kp[x] == kp[y] && x < y); });
    std::vector<uint64_t> sorted((size_t)n, 0);
    for (int k = 0; k < n; ++k) sorted[(size_t)k] = key[(size_t)out.order[(size_t)k]];
    struct Range { int b, e; };
    std::vector<Range> level{{0, n}}, next;
    out.nodes.assign(1, ptmi_bvh_node{});
    int taken = 0;
    for (int lv = 0, first = 0; !level.empty(); ++lv, first += (int)level.size(), level.swap(next)) {
        next.clear();
        const int next_first = first + (int)level.size();
        for (size_t k = 0; k < level.size(); ++k) {
            const int b = level[k].b, e = level[k].e;
            int fell = 0;
            const int m = e - b > PTMI_BVH_LEAF_MAX ? spatial_split(sorted.data(), b, e, lv, &fell) : e;   // (a small root: all in child 0)
            taken += fell;
            const Range child[2] = {{b, m}, {m, e}};
            int32_t ref[2];
            for (int c = 0; c < 2; ++c) {
                if (child[c].e - child[c].b > PTMI_BVH_LEAF_MAX) {
                    ref[c] = next_first + (int32_t)next.size();
                    next.push_back(child[c]);
                } else {
                    ref[c] = spatial_leaf_ref(child[c].b, child[c].e);
                }
            }
            out.nodes[(size_t)first + k].ref[0] = ref[0];
            out.nodes[(size_t)first + k].ref[1] = ref[1];
        }
        out.nodes.resize((size_t)next_first + next.size(), ptmi_bvh_node{});
    }
    if (fallbacks) *fallbacks = taken;
    return bvh_refit(spheres, n, out.nodes.data(), (int)out.nodes.size(), out.order.data(), why);
}

}  // namespace ptmi

extern "C" int ptmi_bvh_layout(const ptmi_sphere *spheres, int n_spheres, ptmi_bvh_node *nodes, int node_capacity, int32_t *order)
{
    if (n_spheres < 0 || !nodes || (n_spheres > 0 && (!spheres || !order))) return PTMI_EINVAL;
    if (n_spheres > PTMI_MAX_BVH_SPHERES) return PTMI_ELIMIT;
    ptmi::BvhBuild b;
    if (int rc = ptmi::bvh_build(spheres, n_spheres, b, nullptr)) return rc;
    if ((size_t)node_capacity < b.nodes.size()) return PTMI_ELIMIT;
    std::memcpy(nodes, b.nodes.data(), b.nodes.size() * sizeof(ptmi_bvh_node));
    if (n_spheres > 0) std::memcpy(order, b.order.data(), (size_t)n_spheres * sizeof(int32_t));
    return (int)b.nodes.size();
}

extern "C" int ptmi_bvh_layout_morton(const ptmi_sphere *spheres, int n_spheres, ptmi_bvh_node *nodes, int node_capacity, int32_t *order)
{
    if (n_spheres < 0 || !nodes || (n_spheres > 0 && (!spheres || !order))) return PTMI_EINVAL;
    if (n_spheres > PTMI_MAX_BVH_SPHERES) return PTMI_ELIMIT;
    ptmi::BvhBuild b;
    if (int rc = ptmi::bvh_build_morton(spheres, n_spheres, b, nullptr)) return rc;
    if (node_capacity < 0 || (size_t)node_capacity < b.nodes.size()) return PTMI_ELIMIT;
    std::memcpy(nodes, b.nodes.data(), b.nodes.size() * sizeof(ptmi_bvh_node));
    if (n_spheres > 0) std::memcpy(order, b.order.data(), (size_t)n_spheres * sizeof(int32_t));
    return (int)b.nodes.size();
}

extern "C" int ptmi_bvh_layout_spatial(const ptmi_sphere *spheres, int n_spheres, ptmi_bvh_node *nodes, int node_capacity, int32_t *order)
{
    if (n_spheres < 0 || !nodes || (n_spheres > 0 && (!spheres || !order))) return PTMI_EINVAL;
    if (n_spheres > PTMI_MAX_BVH_SPHERES) return PTMI_ELIMIT;
    ptmi::BvhBuild b;
    if (int rc = ptmi::bvh_build_spatial(spheres, n_spheres, b, nullptr, nullptr)) return rc;
    if (node_capacity < 0 || (size_t)node_capacity < b.nodes.size()) return PTMI_ELIMIT;
    std::memcpy(nodes, b.nodes.data(), b.nodes.size() * sizeof(ptmi_bvh_node));
    if (n_spheres > 0) std::memcpy(order, b.order.data(), (size_t)n_spheres * sizeof(int32_t));
    return (int)b.nodes.size();
}

extern "C" int ptmi_bvh_refit_layout(const ptmi_sphere *spheres, int n_spheres, ptmi_bvh_node *nodes, int n_nodes, const int32_t *order)
{
    if (n_spheres < 0 || n_nodes < 1 || !nodes) return PTMI_EINVAL;
    // refitted aside: a refusal writes nothing
    std::vector<ptmi_bvh_node> work(nodes, nodes + n_nodes);
    if (int rc = ptmi::bvh_refit(spheres, n_spheres, work.data(), n_nodes, order, nullptr)) return rc;
    std::memcpy(nodes, work.data(), work.size() * sizeof(ptmi_bvh_node));
    return PTMI_OK;
}
