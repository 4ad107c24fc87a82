// ptmi_mesh.cpp -- the triangle hierarchy of a mesh scene (ptmi_set_scene_mesh, ptmi_mesh_layout), host code.
//
// The triangles' derived quantities are computed here once, with the device's f32 operations each rounded on its own (the library is
// compiled without contraction): n = cross(v1 - v0, v2 - v0) (linear's component order), n / sqrt(dot(n, n)) per component.  A
// triangle with !(dot(n, n) > 0) has zero area: it keeps its index and material but is in no leaf, and its stored normal is NaN.
//
// The hierarchy is ptmi_bvh.cpp's over the sphere centres, over the triangles' CENTROIDS: median splits along the longest axis of
// their bounds (ties by original index), leaves of at most PTMI_BVH_LEAF_MAX triangles, the same node format and nesting.  Each
// triangle's box is its vertices' box padded by 2^-16 (max |coordinate| + extent) for the rounding of the hit point and the edge
// functions (the derivation is at check_hit_mesh, ptmi_mesh_device.h).
#include "ptmi_mesh.h"
#include "ptmi_mesh_box.h"
#include "ptmi_mesh_morton.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <numeric>

namespace ptmi {

namespace {

constexpr int kLeafCap = 255;                    // what a leaf reference can encode

struct Builder {
    const ptmi_triangle *tri;
    std::vector<double> lo, hi;                  // padded box per triangle, 3 each
    std::vector<double> centroid;                // 3 each
    std::vector<int32_t> idx;
    std::vector<ptmi_bvh_node> nodes;

    static void store(ptmi_bvh_node &nd, int c, const double l[3], const double h[3]) { box_store(nd.center[c], nd.half[c], l, h); }

    void set_box_of_node(ptmi_bvh_node &nd, int c, int inner) const
    {
        const ptmi_bvh_node &in = nodes[(size_t)inner];
        double l[3], h[3];
        box_empty(l, h);
        for (int k = 0; k < 2; ++k)
            if (in.ref[k] != -1) box_join_stored(l, h, in.center[k], in.half[k]);
        store(nd, c, l, h);
        nd.inv_2r[c] = 0.0f;
    }

    void set_box(ptmi_bvh_node &nd, int c, int b, int e) const
    {
        nd.inv_2r[c] = 0.0f;
        if (b == e) {
            for (int a = 0; a < 3; ++a) { nd.center[c][a] = 0.0f; nd.half[c][a] = -1.0f; }
            return;
        }
        double l[3], h[3];
        box_empty(l, h);
        for (int k = b; k < e; ++k) box_join(l, h, &lo[3 * (size_t)idx[k]], &hi[3 * (size_t)idx[k]]);
        store(nd, c, l, h);
    }

    bool child(int b, int e, int level, int32_t &ref)
    {
        const int n = e - b;
        if (n <= PTMI_BVH_LEAF_MAX || level >= PTMI_BVH_MAX_DEPTH) {
            if (n > kLeafCap) return false;
            ref = n == 0 ? -1 : -1 - (int32_t)(((uint32_t)b << 8) | (uint32_t)n);
            return true;
        }
        ref = (int32_t)nodes.size();
        nodes.emplace_back();
        return fill(ref, b, e, level);
    }

    bool fill(int id, int b, int e, int level)
    {
        const int n = e - b;
        int mid = e;
        if (n > PTMI_BVH_LEAF_MAX) {
            double l[3], h[3];
            for (int a = 0; a < 3; ++a) { l[a] = std::numeric_limits<double>::infinity(); h[a] = -l[a]; }
            for (int k = b; k < e; ++k)
                for (int a = 0; a < 3; ++a) {
                    l[a] = std::min(l[a], centroid[3 * (size_t)idx[k] + a]);
                    h[a] = std::max(h[a], centroid[3 * (size_t)idx[k] + a]);
                }
            int axis = 0;
            for (int a = 1; a < 3; ++a)
                if (h[a] - l[a] > h[axis] - l[axis]) axis = a;
            mid = b + n / 2;
            const double *cen = centroid.data();
            std::nth_element(idx.begin() + b, idx.begin() + mid, idx.begin() + e, [cen, axis](int32_t x, int32_t y) {
                const double px = cen[3 * (size_t)x + axis], py = cen[3 * (size_t)y + axis];
                return px < py || (px == py && x < y);
            });
        }
        int32_t r0 = 0, r1 = 0;
        if (!child(b, mid, level + 1, r0) || !child(mid, e, level + 1, r1)) return false;
        ptmi_bvh_node nd;
        std::memset(&nd, 0, sizeof nd);
        nd.ref[0] = r0; nd.ref[1] = r1;
        if (r0 >= 0) set_box_of_node(nd, 0, r0); else set_box(nd, 0, b, mid);
        if (r1 >= 0) set_box_of_node(nd, 1, r1); else set_box(nd, 1, mid, e);
        nodes[(size_t)id] = nd;
        return true;
    }
};

bool finite3(const float v[3]) { return std::isfinite(v[0]) && std::isfinite(v[1]) && std::isfinite(v[2]); }

}  // namespace

int mesh_build(const ptmi_triangle *tris, int n, MeshBuild &out, std::string *why)
{
    auto refuse = [&](int code, const char *msg) { if (why) *why = msg; return code; };
    if (n < 0 || (n > 0 && !tris)) return refuse(PTMI_EINVAL, "bad triangle arguments");
    if (n > PTMI_MAX_MESH_TRIANGLES) return refuse(PTMI_ELIMIT, "more triangles than PTMI_MAX_MESH_TRIANGLES");
    out.records.assign((size_t)n * 12, 0.0f);
    Builder bd;
    bd.tri = tris;
    bd.lo.resize((size_t)n * 3); bd.hi.resize((size_t)n * 3); bd.centroid.resize((size_t)n * 3);
    bd.idx.clear();
    bd.idx.reserve((size_t)n);
    for (int i = 0; i < n; ++i) {
        const ptmi_triangle &t = tris[i];
        if (!finite3(t.v0) || !finite3(t.v1) || !finite3(t.v2))
            return refuse(PTMI_EINVAL, "a triangle's vertex is not finite: a box cannot bound it");
        if (!finite3(t.color) || !std::isfinite(t.illuminance) || !std::isfinite(t.brdf_param))
            return refuse(PTMI_EINVAL, "a triangle's colour, illuminance or brdf_param is not finite");
        // the derived normal, by the device's operations (ptmi_mesh_box.h): e1 = v1 - v0, e2 = v2 - v0, n = cross(e1, e2)
        const TriangleNormal tn = triangle_normal(t.v0, t.v1, t.v2);
        const float *nv = tn.n;
        const float nn = tn.nn;
        if (!tn.finite) return refuse(PTMI_EINVAL, "a triangle's edges, normal or normal^2 are not finite");
        float *r = &out.records[(size_t)i * 12];
        const float *v[3] = {t.v0, t.v1, t.v2};
        for (int k = 0; k < 3; ++k) { r[4 * k] = v[k][0]; r[4 * k + 1] = v[k][1]; r[4 * k + 2] = v[k][2]; }
        if (!(nn > 0.0f)) {                                      // zero area: never hit
            r[3] = r[7] = r[11] = std::numeric_limits<float>::quiet_NaN();
            continue;
        }
        const float len = std::sqrt(nn);
        r[3] = nv[0] / len; r[7] = nv[1] / len; r[11] = nv[2] / len;
        triangle_box(t.v0, t.v1, t.v2, &bd.lo[3 * (size_t)i], &bd.hi[3 * (size_t)i]);
        for (int a = 0; a < 3; ++a) bd.centroid[3 * (size_t)i + a] = ((double)t.v0[a] + (double)t.v1[a] + (double)t.v2[a]) / 3.0;
        bd.idx.push_back(i);
    }
    const int kept = (int)bd.idx.size();
    bd.nodes.reserve((size_t)std::max(1, kept / 2));
    bd.nodes.emplace_back();
    if (!bd.fill(0, 0, kept, 0)) return refuse(PTMI_ELIMIT, "a leaf at the depth limit would hold more than 255 triangles");
    for (int a = 0; a < 3; ++a) { out.lo[a] = 0.0f; out.hi[a] = 0.0f; }
    if (kept > 0) {
        for (int a = 0; a < 3; ++a) { out.lo[a] = std::numeric_limits<float>::infinity(); out.hi[a] = -out.lo[a]; }
        for (int i : bd.idx) {
            const float *v[3] = {tris[i].v0, tris[i].v1, tris[i].v2};
            for (int k = 0; k < 3; ++k)
                for (int a = 0; a < 3; ++a) { out.lo[a] = std::min(out.lo[a], v[k][a]); out.hi[a] = std::max(out.hi[a], v[k][a]); }
        }
    }
    out.nodes = std::move(bd.nodes);
    out.order = std::move(bd.idx);
    return PTMI_OK;
}

void mesh_refit_plan(const MeshBuild &built, int n_triangles, MeshRefitPlan &out)
{
    out.leaf_pos.assign((size_t)n_triangles, -1);
    for (size_t k = 0; k < built.order.size(); ++k) out.leaf_pos[(size_t)built.order[k]] = (int32_t)k;
    // children have larger ids than their parent (child() appends before it fills): one ascending pass gives every level
    const size_t n = built.nodes.size();
    std::vector<int32_t> level(n, 0);
    int deepest = 0;
    for (size_t id = 0; id < n; ++id)
        for (int c = 0; c < 2; ++c)
            if (built.nodes[id].ref[c] >= 0) {
                level[(size_t)built.nodes[id].ref[c]] = level[id] + 1;
                deepest = std::max(deepest, level[id] + 1);
            }
    std::vector<int32_t> count((size_t)deepest + 2, 0);
    for (size_t id = 0; id < n; ++id) ++count[(size_t)(deepest - level[id]) + 1];
    for (size_t k = 1; k < count.size(); ++k) count[k] += count[k - 1];
    out.level_first = count;
    out.level_nodes.assign(n, 0);
    for (size_t id = 0; id < n; ++id) out.level_nodes[(size_t)count[(size_t)(deepest - level[id])]++] = (int32_t)id;
}

int mesh_refit(const ptmi_triangle *tris, int n, ptmi_bvh_node *nodes, int n_nodes, const int32_t *order, int n_kept, std::string *why)
{
    auto refuse = [&](const std::string &msg) { if (why) *why = msg; return (int)PTMI_EINVAL; };
    if (n < 0 || n_nodes < 1 || n_kept < 0 || n_kept > n || !nodes || (n > 0 && !tris) || (n_kept > 0 && !order)) return refuse("bad refit arguments");
    // the topology must be one ptmi_mesh_layout can have made: every node but the root referred to once, by a node before it; the
    // leaves a partition of the leaf order; the leaf order distinct triangles
    long long inner = 0, in_leaves = 0;
    for (int id = 0; id < n_nodes; ++id)
        for (int c = 0; c < 2; ++c) {
            const int32_t ref = nodes[id].ref[c];
            if (ref >= 0) {
                if (ref <= id || ref >= n_nodes) return refuse("the nodes are not a hierarchy of ptmi_mesh_layout (a child reference out of range: wrong n_nodes?)");
                ++inner;
            } else if (ref != -1) {
                const uint32_t v = (uint32_t)(-1 - ref);
                if ((long long)(v >> 8) + (v & 255u) > n_kept) return refuse("a leaf lies beyond the leaf order (wrong n_kept?)");
                in_leaves += v & 255u;
            }
        }
    if (inner != n_nodes - 1 || in_leaves != n_kept) return refuse("the nodes and the leaf order do not belong together (wrong n_nodes or n_kept?)");
    std::vector<char> in_leaf((size_t)n, 0);
    for (int k = 0; k < n_kept; ++k) {
        if (order[k] < 0 || order[k] >= n || in_leaf[(size_t)order[k]]) return refuse("the leaf order does not name distinct triangles");
        in_leaf[(size_t)order[k]] = 1;
    }
    for (int i = 0; i < n; ++i) {
        const TriangleNormal tn = triangle_normal(tris[i].v0, tris[i].v1, tris[i].v2);
        if (!tn.vertices_finite) return refuse("triangle " + std::to_string(i) + ": a vertex is not finite: a box cannot bound it");
        if (!tn.finite) return refuse("triangle " + std::to_string(i) + ": its edges, normal or normal^2 are not finite");
        if (!in_leaf[(size_t)i] && tn.nn > 0.0f)
            return refuse("triangle " + std::to_string(i) + " had zero area when the scene was set and is in no leaf: it cannot gain area, set the scene again (ptmi_set_scene_mesh)");
    }
    for (int id = n_nodes - 1; id >= 0; --id) {
        ptmi_bvh_node &nd = nodes[id];
        for (int c = 0; c < 2; ++c) {
            const int32_t ref = nd.ref[c];
            if (ref == -1) continue;
            double l[3], h[3];
            box_empty(l, h);
            if (ref >= 0) {
                const ptmi_bvh_node &in = nodes[ref];
                for (int k = 0; k < 2; ++k)
                    if (in.ref[k] != -1) box_join_stored(l, h, in.center[k], in.half[k]);
            } else {
                const uint32_t v = (uint32_t)(-1 - ref);
                for (uint32_t k = v >> 8; k < (v >> 8) + (v & 255u); ++k) {
                    const ptmi_triangle &t = tris[order[k]];
                    double tl[3], th[3];
                    triangle_box(t.v0, t.v1, t.v2, tl, th);
                    box_join(l, h, tl, th);
                }
            }
            box_store(nd.center[c], nd.half[c], l, h);
        }
    }
    return PTMI_OK;
}

// ptmi_mesh_layout_morton / the specification of ptmi_set_mesh_triangles: mesh_build's refusals, records and box; the leaf order by
// (Morton key, index) and the topology of the kept count (ptmi_mesh_morton.h); the boxes by the refit over that topology.
int mesh_build_morton(const ptmi_triangle *tris, int n, MeshBuild &out, std::string *why)
{
    auto refuse = [&](int code, const std::string &msg) { if (why) *why = msg; return code; };
    if (n < 0 || (n > 0 && !tris)) return refuse(PTMI_EINVAL, "bad triangle arguments");
    if (n > PTMI_MAX_MESH_TRIANGLES) return refuse(PTMI_ELIMIT, "more triangles than PTMI_MAX_MESH_TRIANGLES");
    out.records.assign((size_t)n * 12, 0.0f);
    out.order.clear();
    for (int a = 0; a < 3; ++a) { out.lo[a] = std::numeric_limits<float>::infinity(); out.hi[a] = -out.lo[a]; }
    for (int i = 0; i < n; ++i) {
        const ptmi_triangle &t = tris[i];
        const std::string who = "triangle " + std::to_string(i);
        if (!finite3(t.v0) || !finite3(t.v1) || !finite3(t.v2)) return refuse(PTMI_EINVAL, who + ": a vertex is not finite: a box cannot bound it");
        if (!finite3(t.color) || !std::isfinite(t.illuminance) || !std::isfinite(t.brdf_param))
            return refuse(PTMI_EINVAL, who + ": its colour, illuminance or brdf_param is not finite");
        const TriangleNormal tn = triangle_normal(t.v0, t.v1, t.v2);
        if (!tn.finite) return refuse(PTMI_EINVAL, who + ": its edges, normal or normal^2 are not finite");
        float *r = &out.records[(size_t)i * 12];
        const float *v[3] = {t.v0, t.v1, t.v2};
        for (int k = 0; k < 3; ++k) { r[4 * k] = v[k][0]; r[4 * k + 1] = v[k][1]; r[4 * k + 2] = v[k][2]; }
        if (!(tn.nn > 0.0f)) {
            r[3] = r[7] = r[11] = std::numeric_limits<float>::quiet_NaN();
            continue;
        }
        const float len = std::sqrt(tn.nn);
        r[3] = tn.n[0] / len; r[7] = tn.n[1] / len; r[11] = tn.n[2] / len;
        for (int k = 0; k < 3; ++k)
            for (int a = 0; a < 3; ++a) { out.lo[a] = std::min(out.lo[a], v[k][a]); out.hi[a] = std::max(out.hi[a], v[k][a]); }
        out.order.push_back(i);
    }
    if (out.order.empty())
        for (int a = 0; a < 3; ++a) { out.lo[a] = 0.0f; out.hi[a] = 0.0f; }
    std::vector<uint64_t> key((size_t)n, 0);
    for (int i : out.order) key[(size_t)i] = morton_key(tris[i].v0, tris[i].v1, tris[i].v2, out.lo, out.hi);
    const uint64_t *kp = key.data();
    std::sort(out.order.begin(), out.order.end(), [kp](int32_t x, int32_t y) { return kp[x] < kp[y] || (kp[x] == kp[y] && x < y); });
    morton_topology((int)out.order.size(), out.nodes);
    return mesh_refit(tris, n, out.nodes.data(), (int)out.nodes.size(), out.order.data(), (int)out.order.size(), why);
}

}  // namespace ptmi

extern "C" int ptmi_mesh_layout_morton(const ptmi_triangle *triangles, int n_triangles, ptmi_bvh_node *nodes, int node_capacity, int32_t *order, int *n_kept)
{
    if (n_triangles < 0 || !nodes || (n_triangles > 0 && (!triangles || !order))) return PTMI_EINVAL;
    if (n_triangles > PTMI_MAX_MESH_TRIANGLES) return PTMI_ELIMIT;
    ptmi::MeshBuild b;
    if (int rc = ptmi::mesh_build_morton(triangles, n_triangles, b, nullptr)) return rc;
    if ((size_t)node_capacity < b.nodes.size()) return PTMI_ELIMIT;
    std::memcpy(nodes, b.nodes.data(), b.nodes.size() * sizeof(ptmi_bvh_node));
    if (!b.order.empty()) std::memcpy(order, b.order.data(), b.order.size() * sizeof(int32_t));
    if (n_kept) *n_kept = (int)b.order.size();
    return (int)b.nodes.size();
}

extern "C" int ptmi_mesh_refit_layout(const ptmi_triangle *triangles, int n_triangles, ptmi_bvh_node *nodes, int n_nodes, const int32_t *order, int n_kept)
{
    return ptmi::mesh_refit(triangles, n_triangles, nodes, n_nodes, order, n_kept, nullptr);
}

extern "C" int ptmi_mesh_layout(const ptmi_triangle *triangles, int n_triangles, ptmi_bvh_node *nodes, int node_capacity, int32_t *order, int *n_kept)
{
    if (n_triangles < 0 || !nodes || (n_triangles > 0 && (!triangles || !order))) return PTMI_EINVAL;
    if (n_triangles > PTMI_MAX_MESH_TRIANGLES) return PTMI_ELIMIT;
    ptmi::MeshBuild b;
    if (int rc = ptmi::mesh_build(triangles, n_triangles, b, nullptr)) return rc;
    if ((size_t)node_capacity < b.nodes.size()) return PTMI_ELIMIT;
    std::memcpy(nodes, b.nodes.data(), b.nodes.size() * sizeof(ptmi_bvh_node));
    if (!b.order.empty()) std::memcpy(order, b.order.data(), b.order.size() * sizeof(int32_t));
    if (n_kept) *n_kept = (int)b.order.size();
    return (int)b.nodes.size();
}
