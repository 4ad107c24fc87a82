"""The nearest-primitive query's walk held to its specification, on the CPU: tests/cxx/nearest_traverse.cpp includes csrc/ptmi_nearest.h
and restates nearest_search (csrc/ptmi_nearest_device.h) over layouts from the binding, and its (dist, idx, point) must equal the host twin
(binding.nearest, the specification by enumeration) BIT FOR BIT, without r_max and with every family of r_max aimed at the winner's key
(nearest_points.aimed_r_max), on
  * sphere hierarchies: every scene of any_hit_rays.sphere_scenes() over the trees of bvh_layout, bvh_layout_morton and
    bvh_layout_spatial, and a bvh_refit_layout tree after a wave displacement;
  * triangle hierarchies: every family of mesh_rays.SWEPT and needles_1e7 at every placement, a mesh_layout_morton tree, a
    mesh_refit_layout tree of the room, and one after forty kept triangles collapsed to zero area (still in their leaves: no candidates).
In every case at least half the points are served by the walk and at least one is not (a point with a non-finite word, or one beyond
2^40) -- but for a scene whose own box of centres is beyond 2^40 (any_hit_rays.beyond_reach): there the admission rule refuses every point,
and that is what is checked.  Measured and printed (pytest -s; HISTORY.md records them): primitive tests per served point beside the enumeration's, and the
answers the walk gets wrong with its margin at 0 -- the far points are built to outrun the boxes' own padding.  Whether margin 0 is wrong
anywhere is asserted only for the kind it was seen wrong on when this was written (HISTORY.md says which)."""
import os
import sys
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import any_hit_rays as A  # noqa: E402
import bvh_rays  # noqa: E402
import mesh_rays  # noqa: E402
import nearest_points as N  # noqa: E402

B = N.B
N_SPHERE_POINTS, N_MESH_POINTS = 3000, 1500
WRONG = {"bvh": {}, "mesh": {}}                     # case -> answers the margin-0 walk gets wrong, over both r_max families


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return N.traverse_lib(tmp_path_factory.mktemp("nearest"))


def hold(lib, name, kind, spheres, planes, points, sphere_tree, triangles=None, triangle_tree=None):
    """One scene over one pair of trees: the restated walk is the host twin, with and without r_max; the margin-0 walk's wrong answers
    are counted -> primitive tests per served point without r_max"""
    want0 = B.nearest(spheres, planes, triangles, points, None, point=True)
    n_prims = len(spheres) + (0 if triangles is None else len(triangles))
    wrong, per_point = 0, None
    for r_max in (None, N.aimed_r_max(want0[0], want0[1])):
        want = want0 if r_max is None else B.nearest(spheres, planes, triangles, points, r_max, point=True)
        got = N.walk(lib, spheres, planes, triangles, points, r_max, sphere_tree, triangle_tree)
        bad = N.same_bits((got.dist, got.idx, got.point), want)
        assert bad.size == 0, "%s, %s: %d points differ, e.g. point %d %r: walk %r %r %r, twin %r %r %r" % (
            name, "no r_max" if r_max is None else "aimed r_max", bad.size, bad[0], points[bad[0]], got.dist[bad[0]], got.idx[bad[0]], got.point[bad[0]],
            want[0][bad[0]], want[1][bad[0]], want[2][bad[0]])
        served = got.served != 0
        # "at least half served, at least one not" holds for every case but ONE scene (field x 4096 + ..., on its three builders): its giant
        # sphere puts the box of centres itself beyond 2^40, so the admission rule refuses every point wherever it lies -- no choice of
        # points could have half of them served.  That scene stays among the cases for what it does check (the walk equals the twin through
        # the enumeration, and nothing is served); the tests-per-point figure has no served point to be taken over
        beyond = A.beyond_reach(types.SimpleNamespace(kind=kind, spheres=spheres))
        if beyond:
            assert not served.any(), name
        else:
            assert 2 * served.sum() >= len(points) and (~served).sum() >= 1, (name, int(served.sum()))
        zero = N.walk(lib, spheres, planes, triangles, points, r_max, sphere_tree, triangle_tree, margin=0.0)
        wrong += N.same_bits((zero.dist, zero.idx, zero.point), want).size
        if r_max is None:
            per_point = got.tests[served].sum() / max(1, served.sum())
            assert beyond or per_point < n_prims, (name, per_point, n_prims)
            assert (want[1] >= 0).sum() >= len(points) // 2, name       # the answers are answers
        else:
            assert (want[1] != want0[1]).sum() >= len(points) // 8, name           # the aimed r_max moves answers
    WRONG[kind][name] = wrong
    print("\n%s: %d points, %d served; primitive tests per served point %.2f of %d; margin 0 wrong on %d answers" % (
        name, len(points), int(served.sum()), per_point, n_prims, wrong))
    return per_point


# ---- sphere hierarchies ----------------------------------------------------------------------------------------------------------

SPHERE_CASES = [name for name, _ in A.sphere_scenes()]


@pytest.mark.parametrize("name", SPHERE_CASES)
def test_the_sphere_walk_is_the_twin_on_every_builders_tree(lib, name):
    s, p = dict(A.sphere_scenes())[name]
    pts = N.points(s, p, None, N_SPHERE_POINTS, seed=1)
    for what, layout in (("bvh_layout", B.bvh_layout), ("bvh_layout_morton", B.bvh_layout_morton), ("bvh_layout_spatial", B.bvh_layout_spatial)):
        hold(lib, "%s, %s" % (name, what), "bvh", s, p, pts, layout(s))


def test_the_sphere_walk_is_the_twin_on_a_refitted_tree(lib):
    s, p = bvh_rays.adversarial_scene(1500, seed=4)
    nodes, order = B.bvh_layout(s)
    _, moved = A.moved_spheres(s)
    refit = B.bvh_refit_layout(moved, nodes, order)
    assert refit.tobytes() != B.bvh_layout(moved)[0].tobytes()
    hold(lib, "field after a wave of 0.5, bvh_refit_layout", "bvh", moved, p, N.points(moved, p, None, N_SPHERE_POINTS, seed=2), (refit, order))


# ---- triangle hierarchies --------------------------------------------------------------------------------------------------------

def mesh_hold(lib, name, scene, seed, tree=None):
    s, t, p = scene
    t = np.ascontiguousarray(t, B.TRIANGLE_DTYPE)
    return hold(lib, name, "mesh", s, p, N.points(s, p, t, N_MESH_POINTS, seed=seed), B.bvh_layout(s), triangles=t,
                triangle_tree=tree if tree is not None else B.mesh_layout(t))


@pytest.mark.parametrize("placement", list(mesh_rays.PLACEMENTS))
@pytest.mark.parametrize("family", A.MESH_FAMILIES)
def test_the_triangle_walk_is_the_twin_on_every_family_and_placement(lib, family, placement):
    mesh_hold(lib, "%s, %s" % (family, placement), mesh_rays.placed(family, placement, seed=1), 5)


def test_the_triangle_walk_is_the_twin_on_a_morton_and_a_refitted_tree(lib):
    s, t, p = mesh_rays.placed("room", "room", seed=1)
    mesh_hold(lib, "room, mesh_layout_morton", (s, t, p), 3, tree=B.mesh_layout_morton(t))
    t2 = mesh_rays.placed("room", "moved", seed=1)[1]
    nodes, order = B.mesh_layout(t)
    mesh_hold(lib, "room refitted to moved, mesh_refit_layout", (s, t2, p), 11, tree=(B.mesh_refit_layout(t2, nodes, order), order))


def test_the_triangle_walk_skips_triangles_a_refit_collapsed(lib):
    """ptmi_update_mesh_vertices accepts a kept triangle that collapses to zero area: it stays in its leaf with a NaN normal, its vertices
    still count for its box.  Such a triangle is no candidate -- the twin of the NEW triangles never had it in a leaf -- though its three
    edges are still there to be measured: the walk over the refitted tree must skip it in the leaf"""
    s, t, p = mesh_rays.placed("room", "room", seed=1)
    t = np.ascontiguousarray(t, B.TRIANGLE_DTYPE)
    nodes, order = B.mesh_layout(t)
    pts = N.points(s, p, t, N_MESH_POINTS, seed=13)
    before = B.nearest(s, p, t, pts)[1] - len(s) - len(p)
    named = np.bincount(before[before >= 0], minlength=len(t))
    collapsed = np.argsort(-named, kind="stable")[:40]                   # the forty triangles most often the answer: all kept
    assert np.isin(collapsed, order).all() and named[collapsed].sum() >= 100
    t2 = t.copy()
    t2["v2"][collapsed] = t2["v1"][collapsed]
    refit = B.mesh_refit_layout(t2, nodes, order)
    hold(lib, "room with forty kept triangles collapsed, mesh_refit_layout", "mesh", s, p, pts, B.bvh_layout(s), triangles=t2, triangle_tree=(refit, order))
    after = B.nearest(s, p, t2, pts)[1] - len(s) - len(p)
    assert not np.isin(after, collapsed).any() and (after != before).sum() >= 100


# ---- over the kinds as a whole (after the cases above: pytest runs a module's tests in order) ---------------------------------------

@pytest.mark.parametrize("kind", ["bvh", "mesh"])
def test_over_a_hierarchy_kind_the_margin_is_measured(kind):
    assert WRONG[kind], "the cases of this kind come first: run the whole module"
    zero = sum(WRONG[kind].values())
    print("\n%s cases as a whole: margin 0 wrong on %d answers over %d cases" % (kind, zero, len(WRONG[kind])))
    if kind == "mesh":                               # seen wrong when this was written; among the sphere cases no such input was found
        assert zero >= 1, "the walk with its margin at 0 is wrong on no answer: the points do not reach the margin"
