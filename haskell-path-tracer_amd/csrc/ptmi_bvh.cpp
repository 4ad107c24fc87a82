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

#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <numeric>

namespace ptmi {

namespace {

constexpr double kRelPad = 1.0 / 256.0, kAbsPad = 1.0 / 1048576.0;
constexpr int kLeafCap = 255;                    // what a leaf reference can encode

double pad_of(const ptmi_sphere &s)
{
    const double r = std::fabs((double)s.radius);
    const double m = std::max({std::fabs((double)s.position[0]), std::fabs((double)s.position[1]), std::fabs((double)s.position[2]), r});
    return r * (1.0 + kRelPad) + kAbsPad * m;
}

float round_up(double v)
{
    float f = (float)v;
    if ((double)f < v) f = std::nextafter(f, std::numeric_limits<float>::infinity());
    return f;
}

struct Builder {
    const ptmi_sphere *s;
    std::vector<double> pad;
    std::vector<int32_t> idx;
    std::vector<ptmi_bvh_node> nodes;

    // the stored (centre, half) of a box holding [lo, hi], rounded outwards
    static void store(ptmi_bvh_node &nd, int c, const double lo[3], const double hi[3])
    {
        for (int a = 0; a < 3; ++a) {
            const float cf = (float)(0.5 * (lo[a] + hi[a]));
            nd.center[c][a] = cf;
            nd.half[c][a] = round_up(std::max(hi[a] - (double)cf, (double)cf - lo[a]));
        }
    }

    // child c of node `nd` is inner node `inner`: its box is the union of that node's two boxes as STORED (so that boxes nest exactly)
    void set_box_of_node(ptmi_bvh_node &nd, int c, int inner) const
    {
        const ptmi_bvh_node &in = nodes[(size_t)inner];
        double lo[3], hi[3];
        for (int a = 0; a < 3; ++a) { lo[a] = std::numeric_limits<double>::infinity(); hi[a] = -lo[a]; }
        for (int k = 0; k < 2; ++k) {
            if (in.ref[k] == -1) continue;
            for (int a = 0; a < 3; ++a) {
                lo[a] = std::min(lo[a], (double)in.center[k][a] - (double)in.half[k][a]);
                hi[a] = std::max(hi[a], (double)in.center[k][a] + (double)in.half[k][a]);
            }
        }
        store(nd, c, lo, hi);
        nd.inv_2r[c] = std::max(in.ref[0] == -1 ? 0.0f : in.inv_2r[0], in.ref[1] == -1 ? 0.0f : in.inv_2r[1]);
    }

    // child c of node `nd` is the leaf idx[b, e)
    void set_box(ptmi_bvh_node &nd, int c, int b, int e) const
    {
        if (b == e) {
            for (int a = 0; a < 3; ++a) { nd.center[c][a] = 0.0f; nd.half[c][a] = -1.0f; }
            nd.inv_2r[c] = 0.0f;
            return;
        }
        double lo[3], hi[3];
        for (int a = 0; a < 3; ++a) { lo[a] = std::numeric_limits<double>::infinity(); hi[a] = -lo[a]; }
        double r_min = std::numeric_limits<double>::infinity();
        for (int k = b; k < e; ++k) {
            const ptmi_sphere &sp = s[idx[k]];
            for (int a = 0; a < 3; ++a) {
                lo[a] = std::min(lo[a], (double)sp.position[a] - pad[idx[k]]);
                hi[a] = std::max(hi[a], (double)sp.position[a] + pad[idx[k]]);
            }
            r_min = std::min(r_min, std::fabs((double)sp.radius));
        }
        store(nd, c, lo, hi);
        nd.inv_2r[c] = r_min > 0.0 ? round_up(1.0 / (2.0 * r_min)) : std::numeric_limits<float>::infinity();
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
    for (int i = 0; i < n; ++i) {
        const ptmi_sphere &sp = spheres[i];
        const float r2 = sp.radius * sp.radius;     // what the device tests against (pack_scene)
        if (!std::isfinite(sp.position[0]) || !std::isfinite(sp.position[1]) || !std::isfinite(sp.position[2]) || !std::isfinite(sp.radius) ||
            !std::isfinite(r2))
            return refuse(PTMI_EINVAL, "a sphere's position, radius or radius^2 is not finite: a box cannot bound it");
    }
    Builder bd;
    bd.s = spheres;
    bd.pad.resize((size_t)n);
    for (int i = 0; i < n; ++i) bd.pad[(size_t)i] = pad_of(spheres[i]);
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
