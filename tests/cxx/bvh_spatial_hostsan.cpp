// bvh_spatial_hostsan.cpp -- ptmi_bvh_layout_spatial, the host twin of the spatial sphere build, under AddressSanitizer + UBSan, as a
// stand-alone program: compiled together with csrc/ptmi_bvh.cpp (pure host code, no device, no runtime) and run directly by
// tests/test_bvh_spatial_host_sanitized.py.  It drives the twin over every count at which it takes another path and over the families of
// tests/bvh_spatial_scenes.py -- a field, all centres equal, flat in one and in two axes, duplicate keys, the chain the depth guard acts
// on -- with exactly fitting buffers (an access one element beyond is an error here), checks what every tree must satisfy, and provokes
// every refusal, after which nothing may have been written.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "ptmi.h"

#define CHECK(cond)                                                                              \
    do {                                                                                         \
        if (!(cond)) { std::fprintf(stderr, "FAILED line %d: %s\n", __LINE__, #cond); std::exit(1); } \
    } while (0)

namespace {

uint32_t lcg(uint32_t &state) { state = state * 1664525u + 1013904223u; return state >> 8; }
float unit(uint32_t &state) { return (float)lcg(state) / 16777216.0f; }

std::vector<ptmi_sphere> blank(int n)
{
    std::vector<ptmi_sphere> s((size_t)n);
    for (int i = 0; i < n; ++i) {
        ptmi_sphere &x = s[(size_t)i];
        std::memset(&x, 0, sizeof x);
        x.radius = 0.05f + 0.01f * (float)(i % 7);
        x.color[0] = x.color[1] = x.color[2] = 0.5f;
        x.brdf_tag = i % 3 == 0 ? PTMI_GLOSSY : PTMI_MATTE; x.brdf_param = 0.8f;
    }
    return s;
}

// a flat field like world.sphere_field's: wide in x and z, thin in y
std::vector<ptmi_sphere> field(int n, uint32_t seed)
{
    std::vector<ptmi_sphere> s = blank(n);
    const float width = 2.0f + std::sqrt((float)n);
    for (auto &x : s) { x.position[0] = width * (unit(seed) - 0.5f); x.position[1] = 3.0f * unit(seed); x.position[2] = -5.0f - width * unit(seed); }
    return s;
}

std::vector<ptmi_sphere> all_equal(int n)
{
    std::vector<ptmi_sphere> s = blank(n);
    for (auto &x : s) { x.position[0] = 1.25f; x.position[1] = -3.5f; x.position[2] = 7.0f; }
    return s;
}

std::vector<ptmi_sphere> flat(int n, int axes, uint32_t seed)
{
    std::vector<ptmi_sphere> s = field(n, seed);
    for (auto &x : s) { x.position[1] = 1.5f; if (axes > 1) x.position[0] = -2.25f; }
    return s;
}

std::vector<ptmi_sphere> duplicates(int n, uint32_t seed)
{
    std::vector<ptmi_sphere> s = field(n, seed);
    for (int i = 0; i < n; ++i) std::memcpy(s[(size_t)i].position, s[(size_t)(i % (n / 3 + 1))].position, sizeof s[0].position);
    return s;
}

// tests/bvh_spatial_scenes.py's chain: per octave three centres that drop to the next octave one axis after another, four spheres on
// each, and a cluster in the cell at the origin
std::vector<ptmi_sphere> chain()
{
    std::vector<ptmi_sphere> s = blank(14 * 3 * 4 + 100);
    size_t k = 0;
    for (int i = 0; i < 14; ++i) {
        const float hi = std::ldexp(1.0f, -i), lo = std::ldexp(1.0f, -i - 1);
        const float c[3][3] = {{hi, hi, hi}, {lo, hi, hi}, {lo, lo, hi}};
        for (int j = 0; j < 3; ++j)
            for (int d = 0; d < 4; ++d, ++k) std::memcpy(s[k].position, c[j], sizeof c[j]);
    }
    uint32_t seed = 5;
    for (int j = 0; j < 100; ++j, ++k)
        for (int a = 0; a < 3; ++a) s[k].position[a] = j == 0 ? 0.0f : std::ldexp(unit(seed), -16);
    CHECK(k == s.size());
    return s;
}

// what every tree of the twin satisfies; returns the deepest level of an inner node
int check_tree(const std::vector<ptmi_sphere> &s)
{
    const int n = (int)s.size();
    const int capacity = n > PTMI_BVH_LEAF_MAX + 1 ? n - PTMI_BVH_LEAF_MAX : 1;      // the most nodes a tree of n spheres can have
    std::vector<ptmi_bvh_node> nodes((size_t)capacity);
    std::vector<int32_t> order((size_t)n);
    const int n_nodes = ptmi_bvh_layout_spatial(n ? s.data() : nullptr, n, nodes.data(), capacity, n ? order.data() : nullptr);
    CHECK(n_nodes >= 1 && n_nodes <= capacity);
    std::vector<char> seen((size_t)n, 0);
    for (int k = 0; k < n; ++k) { CHECK(order[(size_t)k] >= 0 && order[(size_t)k] < n && !seen[(size_t)order[(size_t)k]]); seen[(size_t)order[(size_t)k]] = 1; }
    std::vector<int> level((size_t)n_nodes, 0), referred((size_t)n_nodes, 0);
    long long in_leaves = 0, next_leaf = 0;
    int deepest = 0;
    for (int id = 0; id < n_nodes; ++id) {
        CHECK(id == 0 || level[(size_t)id] >= level[(size_t)id - 1]);                 // levels are contiguous id ranges
        for (int c = 0; c < 2; ++c) {
            const int32_t ref = nodes[(size_t)id].ref[c];
            if (ref >= 0) {
                CHECK(ref > id && ref < n_nodes && !referred[(size_t)ref]);
                referred[(size_t)ref] = 1;
                level[(size_t)ref] = level[(size_t)id] + 1;
                if (level[(size_t)ref] > deepest) deepest = level[(size_t)ref];
            } else if (ref != -1) {
                const uint32_t v = (uint32_t)(-1 - ref);
                CHECK((v & 255u) >= 1 && (v & 255u) <= PTMI_BVH_LEAF_MAX && (long long)(v >> 8) + (v & 255u) <= n);
                in_leaves += v & 255u;
            } else {
                CHECK(nodes[(size_t)id].half[c][0] == -1.0f && nodes[(size_t)id].inv_2r[c] == 0.0f);
            }
        }
    }
    (void)next_leaf;
    CHECK(in_leaves == n && deepest < PTMI_BVH_MAX_DEPTH);
    // the twin again gives the same bytes, and the refit leaves them as they are
    std::vector<ptmi_bvh_node> again((size_t)n_nodes);
    std::vector<int32_t> order2((size_t)n);
    CHECK(ptmi_bvh_layout_spatial(n ? s.data() : nullptr, n, again.data(), n_nodes, n ? order2.data() : nullptr) == n_nodes);
    CHECK(std::memcmp(again.data(), nodes.data(), (size_t)n_nodes * sizeof(ptmi_bvh_node)) == 0 && order2 == order);
    CHECK(ptmi_bvh_refit_layout(n ? s.data() : nullptr, n, again.data(), n_nodes, n ? order.data() : nullptr) == PTMI_OK);
    CHECK(std::memcmp(again.data(), nodes.data(), (size_t)n_nodes * sizeof(ptmi_bvh_node)) == 0);
    if (n_nodes > 1) CHECK(ptmi_bvh_layout_spatial(s.data(), n, again.data(), n_nodes - 1, order2.data()) == PTMI_ELIMIT);
    return deepest;
}

void refusals()
{
    const std::vector<ptmi_sphere> good = field(300, 77);
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    for (int what = 0; what < 6; ++what) {
        std::vector<ptmi_sphere> bad = good;
        int n = (int)bad.size(), capacity = n, want = PTMI_EINVAL;
        switch (what) {
        case 0: bad[5].position[0] = inf; break;
        case 1: bad[5].radius = -1e30f; break;                                        // radius^2 overflows
        case 2: bad[5].color[1] = nan; break;
        case 3: bad[5].brdf_tag = -1; break;
        case 4: capacity = 3; want = PTMI_ELIMIT; break;
        default: n = PTMI_MAX_BVH_SPHERES + 1; want = PTMI_ELIMIT; break;             // (refused before a sphere is read)
        }
        std::vector<ptmi_bvh_node> nodes(good.size());
        std::vector<int32_t> order(good.size(), -7);
        std::memset(nodes.data(), 7, nodes.size() * sizeof(ptmi_bvh_node));
        const std::vector<ptmi_bvh_node> before = nodes;
        CHECK(ptmi_bvh_layout_spatial(bad.data(), n, nodes.data(), capacity, order.data()) == want);
        CHECK(ptmi_bvh_layout_morton(bad.data(), n, nodes.data(), capacity, order.data()) == want);
        CHECK(std::memcmp(nodes.data(), before.data(), nodes.size() * sizeof(ptmi_bvh_node)) == 0);
        for (int32_t o : order) CHECK(o == -7);
    }
    ptmi_bvh_node one;
    std::vector<int32_t> order(good.size());
    CHECK(ptmi_bvh_layout_spatial(nullptr, 3, nullptr, 0, nullptr) == PTMI_EINVAL);
    CHECK(ptmi_bvh_layout_spatial(nullptr, 3, &one, 1, order.data()) == PTMI_EINVAL);
    CHECK(ptmi_bvh_layout_spatial(good.data(), 3, &one, 1, nullptr) == PTMI_EINVAL);
    CHECK(ptmi_bvh_layout_spatial(nullptr, -1, &one, 1, nullptr) == PTMI_EINVAL);
    CHECK(ptmi_bvh_layout_spatial(good.data(), (int)good.size(), &one, -1, order.data()) == PTMI_ELIMIT);
}

}  // namespace

int main()
{
    const int counts[] = {0, 1, 4, 5, 9, 64, 1020, 20000};
    for (int n : counts) {
        const int deepest = check_tree(field(n, 24u + (uint32_t)n));
        std::printf("field of %d: the deepest inner node at level %d\n", n, deepest);
    }
    check_tree(all_equal(300));
    check_tree(flat(600, 1, 34));
    check_tree(flat(300, 2, 33));
    check_tree(duplicates(600, 35));
    const int deepest = check_tree(chain());
    std::printf("chain: the deepest inner node at level %d\n", deepest);
    CHECK(deepest == PTMI_BVH_MAX_DEPTH - 1);                                         // the guard acted, at the limit
    refusals();
    std::printf("BVH_SPATIAL_HOSTSAN_OK\n");
    return 0;
}
