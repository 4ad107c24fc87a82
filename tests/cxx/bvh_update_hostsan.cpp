// bvh_update_hostsan.cpp -- the host side of the scene's calls (csrc/ptmi_scene.cpp) under AddressSanitizer + UBSan, as a stand-alone
// program: linked against the library built with its host code instrumented and against the HIP stand-in (tests/cxx/hip_stub.cpp:
// device memory is host memory, kernels do not run), run directly by tests/test_bvh_update_host_sanitized.py.  It sets a BVH scene and a
// mesh scene, updates from host and from stand-in device memory, sets new spheres with another count, provokes every refusal, and lets
// every runtime call of ptmi_update_spheres, ptmi_set_bvh_spheres, ptmi_set_scene_bvh, ptmi_set_scene_mesh, ptmi_update_mesh_vertices and
// ptmi_set_mesh_triangles (host and device entries) fail in turn; after each failure the layouts read back are the ones before the call.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include <hip/hip_runtime_api.h>

#include "ptmi.h"

extern "C" {
void hipstub_fail(int kind, long k);
long hipstub_calls(int kind);
long hipstub_live_blocks(void);
void hipstub_poke(const char *kernel_part, long nth, unsigned long long offset, unsigned int value);
void hipstub_clear_pokes(void);
}

#define CHECK(cond)                                                                              \
    do {                                                                                         \
        if (!(cond)) { std::fprintf(stderr, "FAILED line %d: %s\n", __LINE__, #cond); std::exit(1); } \
    } while (0)

namespace {

std::vector<ptmi_sphere> spheres_of(int n, float shift)
{
    std::vector<ptmi_sphere> s((size_t)n);
    for (int i = 0; i < n; ++i) {
        ptmi_sphere &x = s[(size_t)i];
        std::memset(&x, 0, sizeof x);
        x.position[0] = shift + 0.37f * (float)(i % 17); x.position[1] = 0.11f * (float)(i % 29); x.position[2] = -6.0f - 0.05f * (float)i;
        x.radius = 0.1f + 0.01f * (float)(i % 7);
        x.color[0] = x.color[1] = x.color[2] = 0.5f;
        x.brdf_tag = PTMI_MATTE; x.brdf_param = 0.8f;
    }
    return s;
}

std::vector<float> geometry_of(const std::vector<ptmi_sphere> &s)
{
    std::vector<float> g(4 * s.size());
    for (size_t i = 0; i < s.size(); ++i) { std::memcpy(&g[4 * i], s[i].position, 12); g[4 * i + 3] = s[i].radius; }
    return g;
}

// the sphere hierarchy, and -- a mesh scene -- the triangle hierarchy (t_nodes < 0: there is none)
struct Layout {
    int n_nodes = 0, t_nodes = -1, kept = 0;
    std::vector<ptmi_bvh_node> nodes, t_node;
    std::vector<int32_t> order, t_order;
    bool operator==(const Layout &o) const
    {
        return n_nodes == o.n_nodes && order == o.order && std::memcmp(nodes.data(), o.nodes.data(), nodes.size() * sizeof(ptmi_bvh_node)) == 0 &&
               t_nodes == o.t_nodes && kept == o.kept && t_order == o.t_order &&
               (t_node.empty() || std::memcmp(t_node.data(), o.t_node.data(), t_node.size() * sizeof(ptmi_bvh_node)) == 0);
    }
};

Layout read_layout(ptmi_ctx *c, int n_spheres)
{
    Layout l;
    l.n_nodes = ptmi_bvh_read_layout(c, nullptr, 0, nullptr);
    CHECK(l.n_nodes >= 1);
    l.nodes.resize((size_t)l.n_nodes);
    l.order.resize((size_t)n_spheres);
    CHECK(ptmi_bvh_read_layout(c, l.nodes.data(), l.n_nodes, n_spheres ? l.order.data() : nullptr) == l.n_nodes);
    l.t_nodes = ptmi_mesh_read_layout(c, nullptr, 0, nullptr, &l.kept);
    if (l.t_nodes >= 0) {
        l.t_node.resize((size_t)l.t_nodes);
        l.t_order.resize((size_t)l.kept + 1);
        CHECK(ptmi_mesh_read_layout(c, l.t_node.data(), l.t_nodes, l.t_order.data(), &l.kept) == l.t_nodes);
    } else CHECK(l.t_nodes == PTMI_ESTATE);
    return l;
}

// `call` with the k-th runtime call of every kind failing, k = 1, 2, ... until the call gets through: each failure is PTMI_EHIP or
// PTMI_ENOMEM and leaves the layout of `n_before` spheres as it was; `restore` brings that state back after a call that got through.
// Returns how many failures were injected.  `same_blocks`: a failed call leaves as many live device blocks as it found (for calls whose staging
// block, if any, stands already).
template <class F, class R> int walk_failures(ptmi_ctx *c, int n_before, F &&call, R &&restore, bool same_blocks = false)
{
    int injected = 0;
    for (int kind = 0; kind < 4; ++kind)
        for (long k = 1;; ++k) {
            const Layout before = read_layout(c, n_before);
            hipstub_fail(kind, k);
            const long calls = hipstub_calls(kind), live = hipstub_live_blocks();
            const int rc = call();
            const bool hit = hipstub_calls(kind) - calls >= k;
            hipstub_fail(kind, 0);
            if (!hit) { CHECK(rc == PTMI_OK); if (kind < 3) CHECK(restore() == PTMI_OK); break; }
            if (rc == PTMI_OK) { CHECK(restore() == PTMI_OK); continue; }      // (a failure the library may absorb)
            CHECK(rc == PTMI_EHIP || rc == PTMI_ENOMEM);
            CHECK(ptmi_last_error(c) && *ptmi_last_error(c));
            CHECK(read_layout(c, n_before) == before);
            if (same_blocks) CHECK(hipstub_live_blocks() == live);
            ++injected;
        }
    return injected;
}

void scenario(bool mesh)
{
    ptmi_ctx *c = nullptr;
    CHECK(ptmi_create(&c, 0) == PTMI_OK);
    const int n = 300, n2 = 1021;
    const std::vector<ptmi_sphere> s = spheres_of(n, 0.0f), moved = spheres_of(n, 1.5f), more = spheres_of(n2, -2.0f);
    const std::vector<float> g = geometry_of(moved);
    ptmi_plane plane;
    std::memset(&plane, 0, sizeof plane);
    plane.position[1] = -3.0f; plane.direction[1] = 1.0f; plane.color[0] = 0.5f; plane.brdf_tag = PTMI_MATTE; plane.brdf_param = 1.0f;
    ptmi_triangle tri[2];
    std::memset(tri, 0, sizeof tri);
    for (int k = 0; k < 2; ++k) { tri[k].v1[0] = 1.0f + (float)k; tri[k].v2[1] = 1.0f; tri[k].v0[2] = tri[k].v1[2] = tri[k].v2[2] = -9.0f; tri[k].brdf_tag = PTMI_MATTE; tri[k].brdf_param = 1.0f; }

    // refusals of a linear and an unset scene
    CHECK(ptmi_update_spheres(c, g.data(), n) == PTMI_ESTATE);
    CHECK(ptmi_set_bvh_spheres(c, s.data(), n) == PTMI_ESTATE);
    CHECK(ptmi_bvh_read_layout(c, nullptr, 0, nullptr) == PTMI_ESTATE);
    CHECK(ptmi_set_scene(c, s.data(), 16, &plane, 1) == PTMI_OK);
    CHECK(ptmi_update_spheres(c, g.data(), 16) == PTMI_ESTATE);
    CHECK(ptmi_set_bvh_spheres_device(c, s.data(), 16) == PTMI_ESTATE);

    if (mesh) CHECK(ptmi_set_scene_mesh(c, s.data(), n, tri, 2, &plane, 1) == PTMI_OK);
    else CHECK(ptmi_set_scene_bvh(c, s.data(), n, &plane, 1) == PTMI_OK);
    const Layout as_set = read_layout(c, n);
    std::vector<ptmi_bvh_node> host_nodes((size_t)n);
    std::vector<int32_t> host_order((size_t)n);
    CHECK(ptmi_bvh_layout(s.data(), n, host_nodes.data(), n, host_order.data()) == as_set.n_nodes);
    CHECK(std::memcmp(host_nodes.data(), as_set.nodes.data(), (size_t)as_set.n_nodes * sizeof(ptmi_bvh_node)) == 0 && host_order == as_set.order);

    // argument refusals: nothing changes
    CHECK(ptmi_update_spheres(c, nullptr, n) == PTMI_EINVAL);
    CHECK(ptmi_update_spheres(c, g.data(), n - 1) == PTMI_EINVAL);
    CHECK(ptmi_update_spheres_device(c, g.data(), -1) == PTMI_EINVAL);
    CHECK(ptmi_set_bvh_spheres(c, nullptr, 3) == PTMI_EINVAL);
    CHECK(ptmi_set_bvh_spheres(c, s.data(), -1) == PTMI_EINVAL);
    CHECK(ptmi_set_bvh_spheres(c, s.data(), PTMI_MAX_BVH_SPHERES + 1) == PTMI_ELIMIT);
    CHECK(read_layout(c, n) == as_set);
    // the device's verdicts (kernels do not run on the stand-in: the words it "wrote" are placed into the read-back)
    hipstub_poke("bvh_check_kernel", 1, 0, (77u << 2) | 0u);
    CHECK(ptmi_update_spheres(c, g.data(), n) == PTMI_EINVAL && std::strstr(ptmi_last_error(c), "sphere 77"));
    hipstub_clear_pokes();
    for (unsigned code = 0; code < 3; ++code) {
        hipstub_poke("bvh_check_kernel", 1, 0, (55u << 2) | code);
        CHECK(ptmi_set_bvh_spheres(c, more.data(), n2) == PTMI_EINVAL && std::strstr(ptmi_last_error(c), "sphere 55"));
        hipstub_clear_pokes();
    }
    CHECK(read_layout(c, n) == as_set);

    // a whole new scene of either kind over the one that stands, each with every runtime call failing in turn: the old scene stays whole
    std::vector<ptmi_triangle> many40(40), few7(7);
    for (size_t k = 0; k < many40.size(); ++k) { many40[k] = tri[k % 2]; many40[k].v0[2] -= (float)k; many40[k].v1[2] -= (float)k; many40[k].v2[2] -= (float)k; }
    for (size_t k = 0; k < few7.size(); ++k) few7[k] = many40[3 * k];
    auto set_again = [&] { return mesh ? ptmi_set_scene_mesh(c, s.data(), n, tri, 2, &plane, 1) : ptmi_set_scene_bvh(c, s.data(), n, &plane, 1); };
    auto set_more_bvh = [&] { return ptmi_set_scene_bvh(c, more.data(), n2, &plane, 1); };
    int injected = walk_failures(c, n, set_more_bvh, set_again, true);
    injected += walk_failures(c, n2, [&] { return ptmi_set_scene_mesh(c, s.data(), n, many40.data(), 40, &plane, 1); }, set_more_bvh, true);
    CHECK(read_layout(c, n).t_nodes >= 1);
    CHECK(set_again() == PTMI_OK);
    CHECK(read_layout(c, n) == as_set);

    // updates from host memory and from (stand-in) device memory, each with every runtime call failing in turn
    auto nothing = [] { return (int)PTMI_OK; };
    injected += walk_failures(c, n, [&] { return ptmi_update_spheres(c, g.data(), n); }, nothing);
    void *d_g = nullptr;
    CHECK(hipMalloc(&d_g, g.size() * sizeof(float)) == hipSuccess);
    std::memcpy(d_g, g.data(), g.size() * sizeof(float));
    injected += walk_failures(c, n, [&] { return ptmi_update_spheres_device(c, static_cast<const float *>(d_g), n); }, nothing);
    CHECK(read_layout(c, n).n_nodes == as_set.n_nodes);

    // new spheres with another count: up, then to none (the plane stays), then back
    injected += walk_failures(c, n, [&] { return ptmi_set_bvh_spheres(c, more.data(), n2); }, [&] { return ptmi_set_bvh_spheres(c, s.data(), n); });
    const Layout built = read_layout(c, n2);
    std::vector<ptmi_bvh_node> twin((size_t)n2);
    std::vector<int32_t> twin_order((size_t)n2);
    CHECK(ptmi_bvh_layout_morton(more.data(), n2, twin.data(), n2, twin_order.data()) == built.n_nodes);
    for (int k = 0; k < built.n_nodes; ++k) CHECK(built.nodes[(size_t)k].ref[0] == twin[(size_t)k].ref[0] && built.nodes[(size_t)k].ref[1] == twin[(size_t)k].ref[1]);
    CHECK(ptmi_update_spheres(c, g.data(), n) == PTMI_EINVAL);                     // the count is the new one now
    void *d_s = nullptr;
    CHECK(hipMalloc(&d_s, s.size() * sizeof(ptmi_sphere)) == hipSuccess);
    std::memcpy(d_s, s.data(), s.size() * sizeof(ptmi_sphere));
    injected += walk_failures(c, n2, [&] { return ptmi_set_bvh_spheres_device(c, static_cast<const ptmi_sphere *>(d_s), n); },
                              [&] { return ptmi_set_bvh_spheres(c, more.data(), n2); });
    CHECK(read_layout(c, n).n_nodes == as_set.n_nodes);
    injected += walk_failures(c, n, [&] { return ptmi_set_bvh_spheres(c, nullptr, 0); }, [&] { return ptmi_set_bvh_spheres(c, s.data(), n); });
    CHECK(read_layout(c, 0).n_nodes == 1);
    CHECK(ptmi_update_spheres(c, nullptr, 0) == PTMI_OK);
    injected += walk_failures(c, 0, [&] { return ptmi_set_bvh_spheres(c, s.data(), n); }, [&] { return ptmi_set_bvh_spheres(c, nullptr, 0); });
    if (mesh) {
        // new triangles of another count between two updates: the second update makes its second scene block afresh (the first one's was
        // a copy of the block that went, of another size: a copy or a read past its end is a heap overflow here)
        CHECK(ptmi_update_spheres(c, g.data(), n) == PTMI_OK);
        ptmi_triangle many[5];
        for (int k = 0; k < 5; ++k) { many[k] = tri[k % 2]; many[k].v0[2] -= (float)k; many[k].v1[2] -= (float)k; many[k].v2[2] -= (float)k; }
        hipstub_poke("mesh_build_check_kernel", 1, 7 * sizeof(unsigned int), 5u);   // (kBuildKept: all five have area)
        CHECK(ptmi_set_mesh_triangles(c, many, 5) == PTMI_OK);
        hipstub_clear_pokes();
        injected += walk_failures(c, n, [&] { return ptmi_update_spheres(c, g.data(), n); }, nothing);
        CHECK(ptmi_set_mesh_triangles(c, tri, 1) == PTMI_OK);
        CHECK(ptmi_update_spheres(c, g.data(), n) == PTMI_OK);
        CHECK(ptmi_set_bvh_spheres(c, more.data(), n2) == PTMI_OK);                 // (copies the materials of planes and triangles out of the scene block)
        CHECK(ptmi_set_bvh_spheres(c, s.data(), n) == PTMI_OK);

        // new triangles of another count, from host and stand-in device memory, with every runtime call failing in turn.  Kernels do not
        // run: the check kernel's kept count is placed into its read-back, so that the sort, the scatter and every level are launched
        void *d_t = nullptr;
        CHECK(hipMalloc(&d_t, many40.size() * sizeof(ptmi_triangle)) == hipSuccess);
        std::memcpy(d_t, many40.data(), many40.size() * sizeof(ptmi_triangle));
        auto set_triangles = [&](const ptmi_triangle *t, int count, bool device) {
            hipstub_poke("mesh_build_check_kernel", 1, 7 * sizeof(unsigned int), (unsigned int)count);   // (kBuildKept: all of them have area)
            const int rc = device ? ptmi_set_mesh_triangles_device(c, t, count) : ptmi_set_mesh_triangles(c, t, count);
            hipstub_clear_pokes();
            return rc;
        };
        CHECK(set_triangles(many40.data(), 40, false) == PTMI_OK);                  // (the staging block stands from here on)
        CHECK(read_layout(c, n).kept == 40);
        injected += walk_failures(c, n, [&] { return set_triangles(few7.data(), 7, false); }, [&] { return set_triangles(many40.data(), 40, false); }, true);
        CHECK(read_layout(c, n).kept == 7);
        injected += walk_failures(c, n, [&] { return set_triangles(static_cast<const ptmi_triangle *>(d_t), 40, true); }, [&] { return set_triangles(few7.data(), 7, false); }, true);
        const Layout forty = read_layout(c, n);
        CHECK(forty.kept == 40 && forty.t_nodes > 7);                                // (several levels)
        // ... and their vertices moved, over the plan the device call made
        std::vector<float> v(40 * 9);
        for (size_t k = 0; k < many40.size(); ++k) { std::memcpy(&v[9 * k], many40[k].v0, 12); std::memcpy(&v[9 * k + 3], many40[k].v1, 12); std::memcpy(&v[9 * k + 6], many40[k].v2, 12); }
        CHECK(ptmi_update_mesh_vertices(c, v.data(), 39) == PTMI_EINVAL);
        hipstub_poke("mesh_refit_check_kernel", 1, 0, (33u << 2) | 2u);
        CHECK(ptmi_update_mesh_vertices(c, v.data(), 40) == PTMI_EINVAL && std::strstr(ptmi_last_error(c), "triangle 33"));
        hipstub_clear_pokes();
        injected += walk_failures(c, n, [&] { return ptmi_update_mesh_vertices(c, v.data(), 40); }, nothing, true);
        std::memcpy(d_t, v.data(), v.size() * sizeof(float));
        injected += walk_failures(c, n, [&] { return ptmi_update_mesh_vertices_device(c, static_cast<const float *>(d_t), 40); }, nothing, true);
        CHECK(read_layout(c, n) == forty);
        CHECK(hipFree(d_t) == hipSuccess);
    }
    CHECK(injected >= 20);
    std::printf("%s scene: %d injected failures\n", mesh ? "mesh" : "bvh", injected);

    // 0 spheres in a scene with nothing else
    if (!mesh) {
        CHECK(ptmi_set_scene_bvh(c, s.data(), 9, nullptr, 0) == PTMI_OK);
        CHECK(ptmi_set_bvh_spheres(c, nullptr, 0) == PTMI_EINVAL);
        CHECK(read_layout(c, 9).n_nodes == 2);
    }
    CHECK(hipFree(d_g) == hipSuccess && hipFree(d_s) == hipSuccess);
    ptmi_destroy(c);
}

}  // namespace

int main()
{
    scenario(false);
    scenario(true);
    CHECK(hipstub_live_blocks() == 0);
    std::printf("BVH_UPDATE_HOSTSAN_OK\n");
    return 0;
}
