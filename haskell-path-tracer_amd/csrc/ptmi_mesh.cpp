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

#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <numeric>

namespace ptmi {

namespace {

constexpr double kPadFactor = 1.0 / 65536.0;
constexpr int kLeafCap = 255;                    // what a leaf reference can encode

float round_up(double v)
{
    float f = (float)v;
    if ((double)f < v) f = std::nextafter(f, std::numeric_limits<float>::infinity());
    return f;
}

struct Builder {
    const ptmi_triangle *tri;
    std::vector<double> lo, hi;                  // padded box per triangle, 3 each
    std::vector<double> centroid;                // 3 each
    std::vector<int32_t> idx;
    std::vector<ptmi_bvh_node> nodes;

    static void store(ptmi_bvh_node &nd, int c, const double l[3], const double h[3])
    {
        for (int a = 0; a < 3; ++a) {
            const float cf = (float)(0.5 * (l[a] + h[a]));
            nd.center[c][a] = cf;
            nd.half[c][a] = round_up(std::max(h[a] - (double)cf, (double)cf - l[a]));
        }
    }

    void set_box_of_node(ptmi_bvh_node &nd, int c, int inner) const
    {
        const ptmi_bvh_node &in = nodes[(size_t)inner];
        double l[3], h[3];
        for (int a = 0; a < 3; ++a) { l[a] = std::numeric_limits<double>::infinity(); h[a] = -l[a]; }
        for (int k = 0; k < 2; ++k) {
            if (in.ref[k] == -1) continue;
            for (int a = 0; a < 3; ++a) {
                l[a] = std::min(l[a], (double)in.center[k][a] - (double)in.half[k][a]);
                h[a] = std::max(h[a], (double)in.center[k][a] + (double)in.half[k][a]);
            }
        }
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
        for (int a = 0; a < 3; ++a) { l[a] = std::numeric_limits<double>::infinity(); h[a] = -l[a]; }
        for (int k = b; k < e; ++k)
            for (int a = 0; a < 3; ++a) {
                l[a] = std::min(l[a], lo[3 * (size_t)idx[k] + a]);
                h[a] = std::max(h[a], hi[3 * (size_t)idx[k] + a]);
            }
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
        // the derived normal, by the device's operations (ptmi_mesh_device.h): e1 = v1 - v0, e2 = v2 - v0, n = cross(e1, e2)
        const float e1[3] = {t.v1[0] - t.v0[0], t.v1[1] - t.v0[1], t.v1[2] - t.v0[2]};
        const float e2[3] = {t.v2[0] - t.v0[0], t.v2[1] - t.v0[1], t.v2[2] - t.v0[2]};
        const float nv[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};
        const float nn = (nv[0] * nv[0] + nv[1] * nv[1]) + nv[2] * nv[2];
        if (!finite3(e1) || !finite3(e2) || !finite3(nv) || !std::isfinite(nn))
            return refuse(PTMI_EINVAL, "a triangle's edges, normal or normal^2 are not finite");
        float *r = &out.records[(size_t)i * 12];
        const float *v[3] = {t.v0, t.v1, t.v2};
        for (int k = 0; k < 3; ++k) { r[4 * k] = v[k][0]; r[4 * k + 1] = v[k][1]; r[4 * k + 2] = v[k][2]; }
        if (!(nn > 0.0f)) {                                      // zero area: never hit
            r[3] = r[7] = r[11] = std::numeric_limits<float>::quiet_NaN();
            continue;
        }
        const float len = std::sqrt(nn);
        r[3] = nv[0] / len; r[7] = nv[1] / len; r[11] = nv[2] / len;
        double m = 0.0, ext = 0.0;
        for (int a = 0; a < 3; ++a) {
            const double l = std::min({(double)t.v0[a], (double)t.v1[a], (double)t.v2[a]});
            const double h = std::max({(double)t.v0[a], (double)t.v1[a], (double)t.v2[a]});
            m = std::max({m, std::fabs(l), std::fabs(h)});
            ext = std::max(ext, h - l);
        }
        const double pad = kPadFactor * (m + ext);
        for (int a = 0; a < 3; ++a) {
            const double l = std::min({(double)t.v0[a], (double)t.v1[a], (double)t.v2[a]});
            const double h = std::max({(double)t.v0[a], (double)t.v1[a], (double)t.v2[a]});
            bd.lo[3 * (size_t)i + a] = l - pad;
            bd.hi[3 * (size_t)i + a] = h + pad;
            bd.centroid[3 * (size_t)i + a] = ((double)t.v0[a] + (double)t.v1[a] + (double)t.v2[a]) / 3.0;
        }
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

}  // namespace ptmi

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
