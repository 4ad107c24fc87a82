"""ptmi_trace_rays_multi_device's k-bounded walk held to its specification, on the CPU: tests/cxx/multi_hit_traverse.c restates
multi_hit_search (csrc/ptmi_multi_hit_device.h) over the box tests and margins of traverse_slabs.h, and its rows must equal the
specification by enumeration (tests/cxx/multi_hit_reference.c) exactly, for k in {1, 2, 4, 5, 16}, without t_max and with every family of
t_max aimed at the 1st, the k-th and the (k+1)-th hit (multi_hit_rays.aimed_t_max), on
  * sphere hierarchies: every scene of any_hit_rays.sphere_scenes() over the trees of bvh_layout, bvh_layout_morton and
    bvh_layout_spatial, a bvh_refit_layout tree after a wave displacement, and the device test's BVH scene with its stack;
  * triangle hierarchies: every family of mesh_rays.SWEPT and needles_1e7 at every placement, a mesh_layout_morton tree and a
    mesh_refit_layout tree of the room, and the device test's mesh scene with its stack.
The walk with its margin set to 0 must be wrong somewhere among the sphere cases and among the mesh cases.  The strict bound (a child
entered at t_near < bound) is run on the two stack scenes, whose ties reach the bound.  Measured and printed (pytest -s; HISTORY.md records
them): primitive tests per served ray at k = 1, 4 and 16 beside the closest walk's and the enumeration's."""
import ctypes as C
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
import multi_hit_rays as M  # noqa: E402

B = M.B
KS = (1, 2, 4, 5, 16)
N_SPHERE_RAYS, N_MESH_RAYS = 6000, 3000
WRONG = {"bvh": {}, "mesh": {}}                     # case -> rays the margin-0 walk gets wrong, over every k


@pytest.fixture(scope="module")
def libs(tmp_path_factory):
    d = tmp_path_factory.mktemp("multihit")
    return M.multi_hit_lib(d), bvh_rays.traverse_lib(d), mesh_rays.traverse_lib(d)


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def hold(libs, name, kind, spheres, planes, rays, sphere_tree, triangles=None, triangle_tree=None, strict=False):
    """One scene over one pair of trees: the restated walk is the specification for every k, with and without t_max; the margin-0 walk's
    wrong rays are counted -> {k: primitive tests per served ray without t_max}"""
    lib, _, mlib = libs
    rec = mesh_rays.records(mlib, triangles) if triangles is not None else None
    wrong_unwidened = wrong_strict = 0
    per_ray = {}
    for k in KS:
        aimed = M.aimed_t_max(M.reference(lib, spheres, planes, rec, rays, None, k + 1), k)
        for t_max in (None, aimed):
            want = M.reference(lib, spheres, planes, rec, rays, t_max, k)
            got = M.walk(lib, spheres, planes, triangles, rec, rays, t_max, k, sphere_tree, triangle_tree)
            bad = M.rows_differ((got.t, got.idx, got.count), want)
            assert bad.size == 0, "%s, k = %d, %s: %d rays differ, e.g. ray %d: walk %r %r, specification %r %r" % (
                name, k, "no t_max" if t_max is None else "aimed t_max", bad.size, bad[0], got.t[bad[0]], got.idx[bad[0]], want.t[bad[0]], want.idx[bad[0]])
            served = got.served != 0
            if A.beyond_reach(types.SimpleNamespace(kind=kind, spheres=spheres)):      # the scene's own box refuses every ray: the enumeration alone
                assert not served.any(), name
            else:
                assert 2 * served.sum() >= len(rays) and (~served).sum() >= 1, (name, int(served.sum()))
            zero = M.walk(lib, spheres, planes, triangles, rec, rays, t_max, k, sphere_tree, triangle_tree, widen=0.0)
            wrong_unwidened += M.rows_differ((zero.t, zero.idx, zero.count), want).size
            if strict:
                st = M.walk(lib, spheres, planes, triangles, rec, rays, t_max, k, sphere_tree, triangle_tree, strict=1)
                wrong_strict += M.rows_differ((st.t, st.idx, st.count), want).size
            if t_max is None:
                per_ray[k] = got.tests[served].sum() / max(1, served.sum())
                if k in (1, 4, 16):
                    assert (want.count[served] == np.minimum(want.total[served], k)).all()
    WRONG[kind][name] = wrong_unwidened
    print("\n%s: %d rays; primitive tests per served ray %s; margin 0 wrong on %d rows%s" % (
        name, len(rays), ", ".join("k = %d: %.2f" % (k, per_ray[k]) for k in (1, 4, 16)), wrong_unwidened,
        "; strict bound wrong on %d rows" % wrong_strict if strict else ""))
    return per_ray, wrong_strict


# ---- sphere hierarchies ----------------------------------------------------------------------------------------------------------

SPHERE_CASES = [name for name, _ in A.sphere_scenes()]


@pytest.mark.parametrize("name", SPHERE_CASES)
def test_the_sphere_walk_is_the_specification_on_every_builders_tree(libs, name):
    s, p = dict(A.sphere_scenes())[name]
    rays = A.sphere_rays(s, N_SPHERE_RAYS)
    for what, layout in (("bvh_layout", B.bvh_layout), ("bvh_layout_morton", B.bvh_layout_morton), ("bvh_layout_spatial", B.bvh_layout_spatial)):
        hold(libs, "%s, %s" % (name, what), "bvh", s, p, rays, layout(s))


def test_the_sphere_walk_is_the_specification_on_a_refitted_tree(libs):
    s, p = bvh_rays.adversarial_scene(1500, seed=4)
    nodes, order = B.bvh_layout(s)
    _, moved = A.moved_spheres(s)
    refit = B.bvh_refit_layout(moved, nodes, order)
    assert refit.tobytes() != B.bvh_layout(moved)[0].tobytes()
    hold(libs, "field after a wave of 0.5, bvh_refit_layout", "bvh", moved, p, A.sphere_rays(moved, N_SPHERE_RAYS), (refit, order))


def test_the_sphere_walk_on_the_stack_scene_and_its_cost_beside_the_closest_walk(libs):
    """The device test's BVH scene: rays down the stack have 27 hits and ties at every eighth.  At k = 1 without t_max the walk tests no
    more spheres than the closest walk (bvh_traverse.c) plus what the ties cost: a leaf of at most PTMI_BVH_LEAF_MAX for each ray whose
    first two hits tie"""
    lib, blib, _ = libs
    s, _, p, rays = M.driver_scene("bvh")
    tree = B.bvh_layout(s)
    per_ray, wrong_strict = hold(libs, "the device test's BVH scene with its stack", "bvh", s, p, rays, tree, strict=True)
    got = M.walk(lib, s, p, None, None, rays, None, 1, tree)
    served = got.served != 0
    sub = np.ascontiguousarray(rays[served])
    n = len(sub)
    lo, hi = M._box(np.ascontiguousarray(s, np.dtype(s.dtype))["position"])
    import oracle as ora
    so, po = np.ascontiguousarray(s, ora.SPHERE_DTYPE), np.ascontiguousarray(p, ora.PLANE_DTYPE)
    t, idx, just = np.zeros(n, np.float32), np.zeros(n, np.int32), np.zeros(n, np.int32)
    closest = blib.bvh_check_hit(_p(np.ascontiguousarray(tree[0])), _p(np.ascontiguousarray(tree[1], np.int32)), _p(lo), _p(hi), _p(so), len(so), _p(po), len(po),
                                 _p(sub), n, _p(t), _p(idx), _p(just))
    ref2 = M.reference(lib, s, p, None, rays, None, 2)
    ties = int((served & (ref2.tie != 0)).sum())
    mine = int(got.tests[served].sum())
    print("\nk = 1 without t_max: %d sphere tests over %d served rays (%.2f a ray), the closest walk %d (%.2f), the enumeration %d a ray; %d rays tie at the first hit; "
          "strict bound wrong on %d rows" % (mine, n, mine / n, closest, closest / n, len(s), ties, wrong_strict))
    assert mine <= closest + B.BVH_LEAF_MAX * ties, (mine, closest, ties)
    assert per_ray[1] <= per_ray[4] <= per_ray[16] < len(s)


# ---- triangle hierarchies --------------------------------------------------------------------------------------------------------

def mesh_hold(libs, name, scene, family, seed, tree=None, strict=False):
    s, t, p = scene
    rays = A.mesh_case_rays(family, scene, N_MESH_RAYS, seed, libs[2])
    return hold(libs, name, "mesh", s, p, rays, B.bvh_layout(s), triangles=np.ascontiguousarray(t, M.W.TRIANGLE_DTYPE),
                triangle_tree=tree if tree is not None else B.mesh_layout(t), strict=strict)


@pytest.mark.parametrize("placement", list(mesh_rays.PLACEMENTS))
@pytest.mark.parametrize("family", A.MESH_FAMILIES)
def test_the_triangle_walk_is_the_specification_on_every_family_and_placement(libs, family, placement):
    mesh_hold(libs, "%s, %s" % (family, placement), mesh_rays.placed(family, placement, seed=1), "needles" if family == "needles_1e7" else family, 5)


def test_the_triangle_walk_is_the_specification_on_a_morton_and_a_refitted_tree(libs):
    s, t, p = mesh_rays.placed("room", "room", seed=1)
    mesh_hold(libs, "room, mesh_layout_morton", (s, t, p), "room", 3, tree=B.mesh_layout_morton(t))
    t2 = mesh_rays.placed("room", "moved", seed=1)[1]
    nodes, order = B.mesh_layout(t)
    mesh_hold(libs, "room refitted to moved, mesh_refit_layout", (s, t2, p), "room", 11, tree=(B.mesh_refit_layout(t2, nodes, order), order))


def test_the_triangle_walk_on_the_stack_scene(libs):
    s, t, p, rays = M.driver_scene("mesh")
    per_ray, wrong_strict = hold(libs, "the device test's mesh scene with its stack", "mesh", s, p, rays, B.bvh_layout(s), triangles=t,
                                 triangle_tree=B.mesh_layout(t), strict=True)
    print("\nthe mesh stack scene: %d spheres and %d triangles a ray by enumeration; strict bound wrong on %d rows" % (len(s), len(t), wrong_strict))
    assert per_ray[1] <= per_ray[4] <= per_ray[16] < len(s) + len(t)


# ---- over the kinds as a whole (after the cases above: pytest runs a module's tests in order) ---------------------------------------

@pytest.mark.parametrize("kind", ["bvh", "mesh"])
def test_over_a_hierarchy_kind_the_walk_with_unwidened_boxes_is_wrong_somewhere(kind):
    assert WRONG[kind], "the cases of this kind come first: run the whole module"
    zero = sum(WRONG[kind].values())
    print("\n%s cases as a whole: margin 0 wrong on %d rows over %d cases" % (kind, zero, len(WRONG[kind])))
    assert zero >= 1, "%s: the walk with unwidened boxes is wrong on no ray: the rays do not reach the margins" % kind
