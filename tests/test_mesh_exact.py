"""The triangle test against exact geometry, and the walks against their folds beyond the room, on the CPU.  tests/exact_mesh.py is
checkHit on triangles in float64 with a derived bound on what f32 may answer; the restatement of the device's triangle test
(tests/cxx/mesh_traverse.c, mesh_lin_check_hit) is held to its rules 1 to 4 on every shape family of tests/mesh_rays.py at three
placements, with the shares that keep the check from passing vacuously asserted.  The walk of the triangle hierarchy equals the literal fold
bit for bit on the same inputs and on the room at every scale and offset of mesh_rays.SCALES x OFFSETS; the sphere hierarchy's walk equals
its fold on transformed fields, on radii of every size and on the admission test's brackets.  Existing seeded rays are unchanged.
Each sweep prints its figures (pytest -s); DESIGN.md 5.8 records them."""
import hashlib
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import bvh_rays  # noqa: E402
import exact_mesh  # noqa: E402
import mesh_rays  # noqa: E402
from test_bvh_traversal import assert_same as bvh_assert_same, run_both as bvh_run_both  # noqa: E402
from test_mesh_traversal import assert_same  # noqa: E402

W = mesh_rays.world
N_RAYS = 6000


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return mesh_rays.traverse_lib(tmp_path_factory.mktemp("meshexact"))


@pytest.fixture(scope="module")
def bvh_lib(tmp_path_factory):
    return bvh_rays.traverse_lib(tmp_path_factory.mktemp("bvhexact"))


def figures(fig):
    return ", ".join("%s %.4g" % (k, fig[k]) for k in ("rays", "share_d", "share_p_not_d", "share_nothing", "t_ratio", "edge_ratio", "unique", "resolved"))


def test_existing_seeds_give_the_rays_they_always_gave():
    """adversarial_rays with its default box is what it was before it took a box: the digests are of the rays the earlier version made"""
    for sub, seed, n, want in ((3, 3, 100000, "b18ea9a610dc1f1668f5783b93090fd54a232617a2fc96604832b9242d58fba5"),
                               (6, 31, 20000, "b5de10dfe14703f867f07eeb6b73774b34e564c8260deef6dbec1d7573dbfd4d"),
                               (4, 0, 5000, "14eafa3c68a920db34f9a4b67f05b7e66a5a99facb8ecdb4b6602ba81d865ff3")):
        _, t, _ = mesh_rays.adversarial_scene(sub, seed=seed)
        with np.errstate(invalid="ignore"):
            rays = mesh_rays.adversarial_rays(t, n, seed=seed)
        assert hashlib.sha256(rays.tobytes()).hexdigest() == want, (sub, seed, n)


def test_the_rational_pair_agrees_with_float64_and_decides_what_float64_cannot():
    _, t, _ = mesh_rays.closed_room(2)
    v = W.triangle_vertices(t)
    rays = mesh_rays.family_rays(t, 400, seed=9)
    tr = exact_mesh.Triangles(v)
    rng = np.random.default_rng(0)
    for i, j in zip(rng.integers(0, len(rays), 60), rng.integers(0, 13, 60)):
        dN, tt, Wk, N = exact_mesh.exact_pair(rays[i], v[j])
        if tt is None:
            continue
        o, d = rays[i, :3].astype(np.float64), rays[i, 3:].astype(np.float64)
        t64 = (tr.v0n[j] - o @ tr.nhat[j]) / (d @ tr.nhat[j])
        assert abs(float(tt) - t64) <= 1e-9 * (abs(t64) + 1e-30) / max(abs(d @ tr.nhat[j]), 1e-9)
    # a ray through a vertex, exactly: every edge function is exactly 0 in rationals
    dN, tt, Wk, N = exact_mesh.exact_pair(np.array([1, 5, 2, 0, -1, 0], np.float32), np.array([[1, 0, 2], [3, 0, 2], [1, 0, -4]], np.float32))
    assert tt == 5 and Wk[0] == 0 and Wk[2] == 0 and Wk[1] > 0


@pytest.mark.parametrize("placement", list(mesh_rays.PLACEMENTS))
@pytest.mark.parametrize("family", mesh_rays.SWEPT)
def test_the_restated_triangle_test_answers_within_the_exact_bounds_and_the_walk_is_the_fold(lib, family, placement):
    s, t, p = mesh_rays.placed(family, placement, seed=1)
    rays = mesh_rays.sweep_rays(family, t, N_RAYS, seed=5)
    what = "%s, %s, %d triangles" % (family, placement, len(t))
    want = mesh_rays.linear_fold(lib, s, t, p, rays)
    got, tests = mesh_rays.walk(lib, s, t, p, rays)
    assert_same(got, want, what)
    served = mesh_rays.admitted(t, rays) if len(s) == 0 else None
    if served is not None:
        # both paths are taken: the hierarchy, and the literal fold for |d|^2 - 1 beyond 2^-12 and reaches beyond 2^40 (special_rays b, c)
        assert served.sum() > len(rays) // 2 and (~served).sum() > len(rays) // 100, (what, served.sum())
    if family not in ("room", "mixed", "multiscale"):
        # large enough to prune (3 000 triangles and more; multiscale's huge triangles cover everything).  Over the rays the hierarchy
        # serves that start in the scene's box: a ray from 10^4 .. 10^7 scene lengths away widens every box by 2^-16 of its distance,
        # more than the scene, and a ray that takes the fold counts no test at all
        box, _ = mesh_rays.scene_box(t)
        near = served & np.all([(rays[:, a] >= box[a][0]) & (rays[:, a] <= box[a][0] + box[a][1]) for a in range(3)], 0)
        _, near_tests = mesh_rays.walk(lib, s, t, p, np.ascontiguousarray(rays[near]))
        print("\n%s: %d served rays start in the scene's box, triangle tests per ray %.0f" % (what, near.sum(), near_tests / near.sum()))
        assert near.sum() > len(rays) // 2 and near_tests < int(near.sum()) * len(t) // 20, (what, near_tests)
    fig = exact_mesh.check_answers(W.triangle_vertices(t), rays, want, len(s) + len(p), what)
    print("\n%s: %s, triangle tests per ray %.0f" % (what, figures(fig), tests / len(rays)))
    exact_mesh.assert_shares(fig, what)


@pytest.mark.parametrize("family", list(mesh_rays.FAMILIES))
def test_stored_normals_are_the_true_normals_within_the_bound(lib, family):
    """Rule 4, and how the error grows with the shape: per family at its three placements, the largest error and error / bound"""
    for placement in mesh_rays.PLACEMENTS:
        _, t, _ = mesh_rays.placed(family, placement, seed=1)
        rec = mesh_rays.records(lib, t)
        err, bound, constrained, tr = exact_mesh.normal_errors(W.triangle_vertices(t), rec[:, 9:12])
        assert np.all(np.isnan(rec[tr.zero_area, 9])), "a triangle of zero area has a normal"
        live = ~tr.zero_area & np.isfinite(err)
        print("\n%s %s: %d constrained of %d; error %.3g (bound %.3g), error / bound %.3g; unconstrained: error up to %.3g" % (
            family, placement, constrained.sum(), len(t), err[constrained].max(initial=0), bound[constrained].max(initial=0),
            (err[constrained] / bound[constrained]).max(initial=0), err[live & ~constrained].max(initial=0)))
        bad = np.flatnonzero(constrained & ~(err <= bound))
        assert bad.size == 0, "%s %s: triangle %d's normal is off by %g, bound %g" % (family, placement, bad[0], err[bad[0]], bound[bad[0]])


def test_needles_of_1e7_walk_as_they_fold(lib):
    for placement in mesh_rays.PLACEMENTS:
        s, t, p = mesh_rays.placed("needles_1e7", placement, seed=1)
        rays = mesh_rays.sweep_rays("needles", t, 20000, seed=6)
        want = mesh_rays.linear_fold(lib, s, t, p, rays)
        got, _ = mesh_rays.walk(lib, s, t, p, rays)
        assert_same(got, want, "needles 1e7, " + placement)
        exact_mesh.check_answers(W.triangle_vertices(t), rays, want, 0, "needles 1e7, " + placement)


def cracks(family, placement, answer_of, n_rays=20000):
    """Rays from inside a closed mesh that faces inward, aimed at its edges and vertices, answered Nothing while P is not empty (D is then
    empty by rule 2) -> (count, edge-aimed rays).  "icosphere": the icosphere with its winding reversed; "room": the room's twelve wall
    triangles, seen past the icosphere (a ray that slips through the icosphere's own edges meets a wall, and cannot be told from one that
    passes its silhouette: not counted)."""
    s, t, p = mesh_rays.placed(family, placement, seed=1)
    if family == "icosphere":
        t = W.with_vertices(t, W.triangle_vertices(t)[:, [0, 2, 1]])
    centre, radius = mesh_rays.placed_point(family, placement, *mesh_rays.INSIDE[family])
    rays = mesh_rays.inside_edge_rays(t[:12] if family == "room" else t, centre, radius, n_rays, seed=7)
    ans = answer_of(s, t, p, rays)
    c = exact_mesh.check_answers(W.triangle_vertices(t), rays, ans, 0, "cracks, %s %s" % (family, placement))["classes"]
    assert np.mean(c["p_not_d"]) > 0.9                              # the rays do run along edges
    return int(np.sum((ans[2] == 0) & (c["n_p"] > 0) & (c["n_d"] == 0))), len(rays)


@pytest.mark.parametrize("family", ["icosphere", "room"])
def test_cracks_are_counted(lib, family):
    """Measured, not asserted: a ray through a shared edge can be refused by both neighbours"""
    for placement in mesh_rays.PLACEMENTS:
        n, of = cracks(family, placement, lambda s, t, p, rays: mesh_rays.linear_fold(lib, s, t, p, rays))
        print("\ncracks, %s from inside, %s: %d of %d edge-aimed rays (%.0f per million)" % (family, placement, n, of, 1e6 * n / of))


@pytest.mark.parametrize("scale", mesh_rays.SCALES)
def test_the_walk_is_the_fold_on_the_room_at_every_scale_and_offset(lib, scale):
    base = mesh_rays.adversarial_scene(4, seed=2)
    for offset in mesh_rays.OFFSETS:
        s, t, p = mesh_rays.transformed(base, scale, offset)
        rays = mesh_rays.family_rays(t, 40000, seed=3)
        want = mesh_rays.linear_fold(lib, s, t, p, rays)
        got, tests = mesh_rays.walk(lib, s, t, p, rays)
        assert_same(got, want, "room x %g + %r" % (scale, offset))


def bvh_cases():
    field = bvh_rays.adversarial_scene(1500, seed=4)
    for scale, offset in ((2.0 ** -20, bvh_rays.OFFSETS[0]), (2.0 ** -12, bvh_rays.OFFSETS[1]), (3.0, bvh_rays.OFFSETS[1]),
                          (2.0 ** 12, bvh_rays.OFFSETS[2]), (2.0 ** 20, bvh_rays.OFFSETS[0]), (1.0, bvh_rays.OFFSETS[3])):
        yield "field x %g + %r" % (scale, offset), bvh_rays.transformed(field, scale, offset)
    yield "radii 2^-20 .. 2^20", bvh_rays.multiscale_field(3000, seed=4)


def bvh_case_rays(spheres, n):
    return np.ascontiguousarray(np.concatenate([bvh_rays.adversarial_rays(spheres, n // 2, seed=8), bvh_rays.admission_rays(spheres, n // 2, seed=8)]))


def test_the_sphere_walk_is_its_fold_beyond_the_field(bvh_lib):
    for what, (spheres, planes) in bvh_cases():
        rays = bvh_case_rays(spheres, 100_000)
        lin, bvh = bvh_run_both(bvh_lib, spheres, planes, rays)
        bvh_assert_same(lin, bvh)
        assert lin[2].sum() > len(rays) // 20, what
