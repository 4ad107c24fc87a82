"""ptmi_occluded_device's any-hit walks held to the closest hit, on the CPU: tests/cxx/any_hit_traverse.c restates occluded_linear,
occluded_bvh and occluded_mesh (csrc/ptmi_query_device.h) with the box tests and margins of the closest-hit restatements, and its answers
must equal the specification `just && t < t_max` of the literal fold (bvh_rays.linear_fold, mesh_rays.linear_fold), exactly, for every
family of t_max (any_hit_rays.t_max_for), on
  * sphere hierarchies: every scene of test_mesh_exact.bvh_cases() over the trees of bvh_layout, bvh_layout_morton and bvh_layout_spatial,
    and a bvh_refit_layout tree after a wave displacement;
  * triangle hierarchies: every family of mesh_rays.SWEPT and needles_1e7 at every placement, the room at every scale and offset, its
    mesh_layout_morton trees, and mesh_refit_layout onto moved, far and squashed;
  * linear scenes: mainScene, the bench scene, and a field whose radii reach 2^20 on either side of sphere_reach's limit.
Each case asserts what keeps it from passing vacuously (any_hit_rays.assert_conditions).  The walk with its margin set to 0 must be wrong
somewhere among the sphere cases and among the mesh cases: the rays do reach the margins.  Measured and printed (pytest -s; HISTORY.md
records them): the shares of the paths, primitive tests per ray beside the closest walk's, what the margin-0, half-margin and strict-bound
variants get wrong.  tests/test_gpu_any_hit.py is the device half."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import any_hit_rays as A  # noqa: E402
import bvh_rays  # noqa: E402
import mesh_rays  # noqa: E402

B, W = A.B, A.W
N_SPHERE_RAYS, N_MESH_RAYS = 20_000, 6000
TOTALS = {"bvh": [0, 0], "mesh": [0, 0]}            # (any-hit tests, closest-walk tests) over the served rays of every case of the kind
WRONG = {"bvh": {}, "mesh": {}}                     # case -> rays the variants get wrong: (margin 0, half margin, strict bound)


@pytest.fixture(scope="module")
def libs(tmp_path_factory):
    d = tmp_path_factory.mktemp("anyhit")
    return bvh_rays.traverse_lib(d), mesh_rays.traverse_lib(d)


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return A.any_hit_lib(tmp_path_factory.mktemp("anyhitlib"))


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def closest_sphere_tests(blib, case, tree, rows):
    """sphere tests of the closest-hit walk (bvh_traverse.c) over this tree on the rays `rows`"""
    nodes, order = tree
    rays = np.ascontiguousarray(case.rays[rows])
    n = len(rays)
    lo, hi = A._box(case.spheres["position"])
    t, idx, just = np.zeros(n, np.float32), np.zeros(n, np.int32), np.zeros(n, np.int32)
    return blib.bvh_check_hit(_p(np.ascontiguousarray(nodes)), _p(np.ascontiguousarray(order, np.int32)), _p(lo), _p(hi), _p(case.spheres), len(case.spheres),
                              _p(case.planes), len(case.planes), _p(rays), n, _p(t), _p(idx), _p(just))


def closest_triangle_tests(mlib, case, tree, rows):
    """triangle tests of the closest-hit walk (mesh_traverse.c) over this tree on the rays `rows`"""
    nodes, order = tree
    rays = np.ascontiguousarray(case.rays[rows])
    n = len(rays)
    kept = case.triangles[order]
    lo, hi = A._box(np.concatenate([kept["v0"], kept["v1"], kept["v2"]]))
    t, idx, just = np.zeros(n, np.float32), np.zeros(n, np.int32), np.zeros(n, np.int32)
    return mlib.mesh_walk_check_hit(_p(np.ascontiguousarray(nodes)), _p(np.ascontiguousarray(order, np.int32)), len(order), _p(lo), _p(hi), _p(case.spheres),
                                    len(case.spheres), _p(case.planes), len(case.planes), _p(case.records), len(case.records), _p(rays), n, _p(t), _p(idx), _p(just))


def hold(lib, libs, case, what, sphere_tree=None, triangle_tree=None, conditions=True):
    """One case over one pair of trees: the restatement is the specification, the conditions hold, the figures are printed and kept"""
    name = "%s, %s" % (case.name, what)
    answer, path, tests = case.walk(lib, sphere_tree, triangle_tree)
    bad = case.wrong(answer)
    assert bad.size == 0, "%s: %d rays differ, e.g. %s" % (what, bad.size, case.describe(bad[0], answer[bad[0]]))
    assert ((path == A.NOT_SERVED) | (path == A.NO_LIMIT) | (tests >= 0)).all()
    if conditions:
        A.assert_conditions(case, path)
    served = path != A.NOT_SERVED
    built = case.trees()
    if case.kind == "bvh":
        closest = closest_sphere_tests(libs[0], case, sphere_tree or built[0], served)
    else:
        closest = closest_triangle_tests(libs[1], case, triangle_tree or built[1], served)
    fig = A.figures(case, path, tests, closest)
    TOTALS[case.kind][0] += fig["tests"]
    TOTALS[case.kind][1] += fig["closest_tests"]
    variants = tuple(int(case.wrong(case.walk(lib, sphere_tree, triangle_tree, widen=w, strict=s)[0]).size) for w, s in ((0.0, 0), (0.5, 0), (1.0, 1)))
    WRONG[case.kind][name] = variants
    print("\n%s; half margin wrong on %d, strict bound on %d" % (A.show(name, fig, variants[0]), variants[1], variants[2]))


# ---- sphere hierarchies ----------------------------------------------------------------------------------------------------------

SPHERE_CASES = [name for name, _ in A.sphere_scenes()]


@pytest.fixture(scope="module")
def sphere_cases(libs):
    return {name: A.Case(name, "bvh", s, p, A.sphere_rays(s, N_SPHERE_RAYS), libs) for name, (s, p) in A.sphere_scenes()}


@pytest.mark.parametrize("name", SPHERE_CASES)
def test_the_sphere_any_hit_walk_is_the_specification_on_every_builders_tree(lib, libs, sphere_cases, name):
    case = sphere_cases[name]
    for what, layout in (("bvh_layout", B.bvh_layout), ("bvh_layout_morton", B.bvh_layout_morton), ("bvh_layout_spatial", B.bvh_layout_spatial)):
        hold(lib, libs, case, what, sphere_tree=layout(case.spheres))


def test_the_sphere_any_hit_walk_is_the_specification_on_a_refitted_tree(lib, libs):
    """Boxes no build produced: the field's tree refitted to its spheres after a wave of 0.5"""
    s, p = bvh_rays.adversarial_scene(1500, seed=4)
    nodes, order = B.bvh_layout(s)
    _, moved = A.moved_spheres(s)
    case = A.Case("field after a wave of 0.5", "bvh", moved, p, A.sphere_rays(moved, N_SPHERE_RAYS), libs)
    refit = B.bvh_refit_layout(moved, nodes, order)
    assert refit.tobytes() != B.bvh_layout(moved)[0].tobytes()
    hold(lib, libs, case, "bvh_refit_layout", sphere_tree=(refit, order))


# ---- triangle hierarchies --------------------------------------------------------------------------------------------------------

def mesh_case(libs, name, scene, family, seed):
    s, t, p = scene
    return A.Case(name, "mesh", s, p, A.mesh_case_rays(family, scene, N_MESH_RAYS, seed, libs[1]), libs, triangles=t)


@pytest.mark.parametrize("placement", list(mesh_rays.PLACEMENTS))
@pytest.mark.parametrize("family", A.MESH_FAMILIES)
def test_the_triangle_any_hit_walk_is_the_specification_on_every_family_and_placement(lib, libs, family, placement):
    case = mesh_case(libs, "%s, %s" % (family, placement), mesh_rays.placed(family, placement, seed=1), "needles" if family == "needles_1e7" else family, 5)
    hold(lib, libs, case, "mesh_layout")


@pytest.mark.parametrize("scale", mesh_rays.SCALES)
def test_the_triangle_any_hit_walk_is_the_specification_on_the_room_at_every_scale_and_offset(lib, libs, scale):
    base = mesh_rays.adversarial_scene(4, seed=2)
    for offset in mesh_rays.OFFSETS:
        case = mesh_case(libs, "room x %g + %r" % (scale, offset), mesh_rays.transformed(base, scale, offset), None, 3)
        hold(lib, libs, case, "mesh_layout")
        if offset in (mesh_rays.OFFSETS[0], mesh_rays.OFFSETS[3]):
            hold(lib, libs, case, "mesh_layout_morton", triangle_tree=B.mesh_layout_morton(case.triangles))


@pytest.mark.parametrize("target", ["moved", "far", "squashed"])
def test_the_triangle_any_hit_walk_is_the_specification_on_a_refitted_tree(lib, libs, target):
    """Boxes no build produced: the room's tree refitted onto a placement and onto a squashed copy"""
    s, t, p = mesh_rays.placed("room", "room", seed=1)
    t2 = A.squashed(t) if target == "squashed" else mesh_rays.placed("room", target, seed=1)[1]
    nodes, order = B.mesh_layout(t)
    case = mesh_case(libs, "room refitted to " + target, (s, t2, p), "room", 11)
    hold(lib, libs, case, "mesh_refit_layout", triangle_tree=(B.mesh_refit_layout(t2, nodes, order), order))


# ---- linear scenes ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", [x[0] for x in A.linear_scenes()])
def test_the_linear_any_hit_walk_is_the_specification(lib, libs, name):
    _, s, p, served_at_all = next(x for x in A.linear_scenes() if x[0] == name)
    rays = np.concatenate([bvh_rays.adversarial_rays(s, N_SPHERE_RAYS // 2, seed=8), bvh_rays.admission_rays(s, N_SPHERE_RAYS // 2, seed=8)])
    case = A.Case(name, "linear", s, p, rays, libs)
    answer, path, tests = case.walk(lib)
    bad = case.wrong(answer)
    assert bad.size == 0, "%d rays differ, e.g. %s" % (bad.size, case.describe(bad[0], answer[bad[0]]))
    reach = lib.any_sphere_reach(_p(case.spheres), len(case.spheres))
    if served_at_all:
        assert reach <= 2.0 ** 40
        A.assert_conditions(case, path)
    else:
        # sphere_reach on the far side of its limit: the scene serves no ray, whatever the ray (the near side is the case before it)
        assert reach > 2.0 ** 40 and (path == A.NOT_SERVED).all() and case.want.sum() >= len(rays) // 100
    lin_tests = int((path != A.NOT_SERVED).sum()) * len(case.spheres)
    print("\n" + A.show(name, A.figures(case, path, tests, lin_tests)) + " (the fold's), sphere_reach %r" % reach)


# ---- over the kinds as a whole (after the cases above: pytest runs a module's tests in order) ---------------------------------------

@pytest.mark.parametrize("kind", ["bvh", "mesh"])
def test_over_a_hierarchy_kind_the_any_hit_walk_tests_no_more_than_the_closest_walk_and_margin_0_is_wrong_somewhere(kind):
    assert WRONG[kind], "the cases of this kind come first: run the whole module"
    mine, closest = TOTALS[kind]
    zero, half, strict = (sum(v[k] for v in WRONG[kind].values()) for k in range(3))
    print("\n%s cases as a whole: %d primitive tests against the closest walk's %d over the same served rays; wrong rays over %d cases: margin 0 %d, "
          "half margin %d, strict bound %d" % (kind, mine, closest, len(WRONG[kind]), zero, half, strict))
    assert mine <= closest, (kind, mine, closest)
    assert zero >= 1, "%s: the walk with unwidened boxes is wrong on no ray: the rays do not reach the margins" % kind
    # Half the margin: the sphere margin is the sphere test's rounding bound with no factor to spare (ptmi_bvh_device.h), and the silhouette
    # rays of the small-scale fields come within half of it -- a margin half as large in any_hit_spheres fails here.  The triangle margin is
    # 2^8 times its bound (ptmi_mesh_device.h): half of it still covers every ray, and what it gets wrong is printed, not asserted.  The
    # strict bound (t_near < lim) can differ from the device's only where a box is entered exactly at lim, which a sufficient margin
    # excludes for every occluder: likewise printed.
    if kind == "bvh":
        assert half >= 1, "the sphere walk with half its margin is wrong on no ray: the rays do not come within half a margin"
