"""ptmi_mesh_refit_layout (host code, no device): the specification of the device refit behind ptmi_update_mesh_vertices.  The topology
of ptmi_mesh_layout is kept (`ref`, the leaf order) and the boxes are recomputed for moved vertices with the build's own arithmetic:
unchanged vertices give the build's nodes back byte for byte, moving away and back too; after a deformation every child box holds the
padded box of every triangle under it; and tests/cxx/mesh_traverse.c, walking the REFITTED nodes as the device's check_hit_mesh does,
picks the hit the literal fold over the moved triangles picks (t bit for bit, the primitive, Just / Nothing) on 10^6 adversarial rays
aimed at the moved triangles -- under a smooth wave and under per-vertex noise of the order of the icosphere's radius, which makes a bad
tree that must still be right."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import mesh_rays  # noqa: E402

pkg = mesh_rays.pkg
binding, world = pkg.binding, pkg.world


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return mesh_rays.traverse_lib(tmp_path_factory.mktemp("meshrefit"))


def moved(t, amount, kind, seed=0):
    return world.with_vertices(t, world.displaced(world.triangle_vertices(t), amount, kind, seed=seed))


@pytest.mark.parametrize("subdivisions", [3, 6])
def test_unchanged_vertices_give_the_builds_nodes_byte_for_byte(subdivisions):
    _, t, _ = mesh_rays.adversarial_scene(subdivisions, seed=subdivisions)
    nodes, order = binding.mesh_layout(t)
    again = binding.mesh_refit_layout(t, nodes, order)
    assert again.tobytes() == nodes.tobytes()


def children(nodes):
    """(node, child, first, count) of every leaf child and (node, child, inner) of every inner child"""
    for k in range(len(nodes)):
        for c in range(2):
            ref = int(nodes[k]["ref"][c])
            if ref >= 0:
                yield k, c, ref, None
            elif ref != -1:
                yield k, c, (-1 - ref) >> 8, (-1 - ref) & 255


@pytest.mark.parametrize("kind, amount", [("wave", 0.1), ("noise", 1.0)])
def test_after_a_deformation_the_topology_stands_and_every_box_holds_what_lies_under_it(kind, amount):
    _, t, _ = mesh_rays.adversarial_scene(4, seed=4)
    nodes, order = binding.mesh_layout(t)
    t2 = moved(t, amount, kind)
    assert not np.array_equal(t2["v0"], t["v0"])
    order_before = order.copy()
    got = binding.mesh_refit_layout(t2, nodes, order)
    assert np.array_equal(order, order_before)
    assert np.array_equal(got["ref"], nodes["ref"]) and np.all(got["inv_2r"] == 0)
    assert got.tobytes() != nodes.tobytes()
    # the padded boxes by ptmi_mesh.cpp's rule, in float64: the vertices' box padded by 2^-16 (max |coordinate| + extent)
    v = world.triangle_vertices(t2).astype(np.float64)
    vlo, vhi = v.min(1), v.max(1)
    pad = 2.0 ** -16 * (np.abs(v).max((1, 2)) + (vhi - vlo).max(1))
    tlo, thi = vlo - pad[:, None], vhi + pad[:, None]
    lo = got["center"].astype(np.float64) - got["half"].astype(np.float64)
    hi = got["center"].astype(np.float64) + got["half"].astype(np.float64)
    # bottom-up: what lies under a child is its leaf's triangles, or the union of what lies under the inner node's children
    under_lo, under_hi = {}, {}
    for k in range(len(got) - 1, -1, -1):
        l, h = np.full(3, np.inf), np.full(3, -np.inf)
        for kk, c, first, count in [x for x in children(got[k:k + 1])]:
            if count is None:
                cl, ch = under_lo[first], under_hi[first]
            else:
                idx = order[first:first + count]
                cl, ch = tlo[idx].min(0), thi[idx].max(0)
            assert np.all(lo[k, c] <= cl) and np.all(ch <= hi[k, c]), (k, c)
            l, h = np.minimum(l, cl), np.maximum(h, ch)
        under_lo[k], under_hi[k] = l, h


def test_moving_away_and_back_restores_the_original_bytes():
    _, t, _ = mesh_rays.adversarial_scene(5, seed=2)
    nodes, order = binding.mesh_layout(t)
    away = binding.mesh_refit_layout(moved(t, 0.5, "noise"), nodes, order)
    assert away.tobytes() != nodes.tobytes()
    back = binding.mesh_refit_layout(t, away, order)
    assert back.tobytes() == nodes.tobytes()


def walk_refitted(lib, s, t_set, t_moved, p, rays):
    """mesh_traverse.c's walk over the nodes of the scene AS SET refitted to the moved triangles -> (t, idx, just)"""
    import oracle as ora
    nodes, order = binding.mesh_layout(t_set)
    nodes = binding.mesh_refit_layout(t_moved, nodes, order)
    sp, pl = np.ascontiguousarray(s, ora.SPHERE_DTYPE), np.ascontiguousarray(p, ora.PLANE_DTYPE)
    rec = mesh_rays.records(lib, t_moved)
    kept = t_moved[order]
    allv = np.concatenate([kept["v0"], kept["v1"], kept["v2"]]).astype(np.float32)
    lo, hi = np.ascontiguousarray(allv.min(0)), np.ascontiguousarray(allv.max(0))
    n = len(rays)
    tt, idx, just = np.zeros(n, np.float32), np.zeros(n, np.int32), np.zeros(n, np.int32)
    _p = mesh_rays._p
    lib.mesh_walk_check_hit(_p(nodes), _p(order), len(order), _p(lo), _p(hi), _p(sp), len(sp), _p(pl), len(pl), _p(rec), len(rec),
                            _p(rays), n, _p(tt), _p(idx), _p(just))
    return tt, idx, just


@pytest.mark.parametrize("subdivisions, kind, amount", [(3, "wave", 0.1), (3, "noise", 1.0), (6, "wave", 0.1), (6, "noise", 1.0)])
def test_the_walk_over_refitted_nodes_picks_the_linear_folds_hit(lib, subdivisions, kind, amount):
    """OBSERVED (rays the fold alone puts on icosphere triangles, of 10^6; the demand is more than 10^5):
    1 310 triangles: wave 0.1 206 833, noise 1.0 429 054; 82 757 triangles: wave 0.1 217 133, noise 1.0 525 969"""
    n_rays = 1_000_000
    s, t, p = mesh_rays.adversarial_scene(subdivisions, seed=subdivisions)
    t2 = moved(t, amount, kind, seed=subdivisions)
    rays = mesh_rays.adversarial_rays(t2, n_rays, seed=subdivisions + 10)
    want = mesh_rays.linear_fold(lib, s, t2, p, rays)
    got = walk_refitted(lib, s, t, t2, p, rays)
    first = len(s) + len(p)
    on_icosphere = int(np.sum(want[2].astype(bool) & (want[1] >= first + 13)))
    print("refit walk: %d triangles, %s %.2f: %d of %d rays on icosphere triangles" % (len(t), kind, amount, on_icosphere, n_rays))
    assert not np.any(got[2] == -2), "the traversal stack would overflow"
    bad = np.flatnonzero((got[0].view(np.uint32) != want[0].view(np.uint32)) | (got[1] != want[1]) | (got[2] != want[2]))
    assert bad.size == 0, "%d of %d rays differ, e.g. ray %d: walk (%r, %d, %d) fold (%r, %d, %d)" % (
        bad.size, n_rays, bad[0], got[0][bad[0]], got[1][bad[0]], got[2][bad[0]], want[0][bad[0]], want[1][bad[0]], want[2][bad[0]])
    assert on_icosphere > n_rays // 10, on_icosphere


def test_refusals_and_a_collapsed_triangle(lib):
    s, t, p = mesh_rays.adversarial_scene(3, seed=3)
    nodes, order = binding.mesh_layout(t)
    L = binding.load_library()

    def rc(tri, nd, n_nodes, od, n_kept):
        tri = np.ascontiguousarray(tri, world.TRIANGLE_DTYPE)
        nd, before = nd.copy(), nd.tobytes()
        got = L.ptmi_mesh_refit_layout(mesh_rays._p(tri), len(tri), mesh_rays._p(nd), n_nodes, mesh_rays._p(od), n_kept)
        if got != binding.PTMI_OK:
            assert nd.tobytes() == before, "a refused refit wrote into the nodes"
        return got
    assert rc(t, nodes, len(nodes), order, len(order)) == binding.PTMI_OK
    assert rc(t, nodes, len(nodes) - 1, order, len(order)) == binding.PTMI_EINVAL
    assert rc(t, np.concatenate([nodes, nodes[:1]]), len(nodes) + 1, order, len(order)) == binding.PTMI_EINVAL
    assert rc(t, nodes, len(nodes), order, len(order) - 1) == binding.PTMI_EINVAL
    assert rc(t, nodes, len(nodes), np.concatenate([order, order[:1]]), len(order) + 1) == binding.PTMI_EINVAL
    for value in (np.nan, np.inf, 1e25):
        bad = t.copy()
        bad["v1"][40, 2] = value
        assert rc(bad, nodes, len(nodes), order, len(order)) == binding.PTMI_EINVAL, value
    # one of the scene's five triangles of zero area (the last five) given area: it is in no leaf
    flat = len(t) - 3
    assert flat not in order.tolist()
    bad = t.copy()
    bad["v2"][flat] += np.float32(0.5)
    assert rc(bad, nodes, len(nodes), order, len(order)) == binding.PTMI_EINVAL
    moved_flat = t.copy()                                     # ... moved while staying flat: accepted
    for k in ("v0", "v1", "v2"):
        moved_flat[k][flat] += np.float32(0.25)
    assert rc(moved_flat, nodes, len(nodes), order, len(order)) == binding.PTMI_OK
    # a kept triangle collapsed to a point is accepted, stays in its leaf, and is never hit
    k = int(order[len(order) // 2])
    col = t.copy()
    col["v1"][k] = col["v0"][k]
    col["v2"][k] = col["v0"][k]
    assert rc(col, nodes, len(nodes), order, len(order)) == binding.PTMI_OK
    rays = mesh_rays.adversarial_rays(t[k:k + 1], 20000, seed=9)         # aimed at where it was, and at the point it is now
    rays2 = mesh_rays.adversarial_rays(col[k:k + 1], 20000, seed=9)
    rays = np.concatenate([rays, rays2])
    want = mesh_rays.linear_fold(lib, s, col, p, rays)
    got = walk_refitted(lib, s, t, col, p, rays)
    prim = len(s) + len(p) + k
    assert not np.any(want[1] == prim) and not np.any(got[1] == prim)
    assert np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32)) and np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])
    assert want[2].sum() > 1000
