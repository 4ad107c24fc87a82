"""The device's checkHit on mesh scenes against exact geometry (tests/exact_mesh.py) and against the literal fold, on the shape families
and placements of tests/mesh_rays.py; the same after ptmi_update_mesh_vertices to a placement and to a squashed copy (a walk on boxes no
build produced); renders of the room moved by (1e3, -2e3, 5e2) with its camera against the mesh reference in the three kernel families;
the sphere hierarchy on transformed fields, radii of every size and the admission brackets; and the crack counts, equal to the
restatement's.  tests/test_mesh_exact.py is the CPU half."""
import os
import sys

import numpy as np
import pytest

from conftest import assert_planes_equal, initial_planes

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bvh_rays  # noqa: E402
import exact_mesh  # noqa: E402
import mesh_rays  # noqa: E402
from test_gpu_mesh_renders import scene as room_scene  # noqa: E402
from test_mesh_exact import N_RAYS, bvh_case_rays, bvh_cases, cracks, figures  # noqa: E402

pytestmark = pytest.mark.gpu
CAP = 1 << 16
THREADS = max(1, min(16, os.cpu_count() or 1))
W = mesh_rays.world
MOVE = (1e3, -2e3, 5e2)


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return mesh_rays.traverse_lib(tmp_path_factory.mktemp("gpumeshexact"))


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return mesh_rays.reference_lib(tmp_path_factory.mktemp("gpumeshexactref"))


@pytest.fixture(scope="module")
def bvh_lib(tmp_path_factory):
    return bvh_rays.traverse_lib(tmp_path_factory.mktemp("gpubvhexact"))


def same_bits(got, want, what):
    for a, b, name in zip(got, want, ("t", "idx", "just")):
        bad = np.flatnonzero(np.asarray(a).view(np.uint32) != np.asarray(b).view(np.uint32))
        assert bad.size == 0, "%s: %s differs for %d rays, first %d: device %r, fold %r" % (what, name, bad.size, bad[0], a[bad[0]], b[bad[0]])


def device_answer(ctx, rays):
    t, idx, just = (np.array(x) for x in ctx.eval_check_hit(rays))
    miss = just == 0                                                   # a miss in the fold's form: (0, -1, 0)
    return np.where(miss, np.float32(0), t), np.where(miss, -1, idx).astype(np.int32), just.astype(np.int32)


@pytest.mark.parametrize("placement", list(mesh_rays.PLACEMENTS))
@pytest.mark.parametrize("family", mesh_rays.SWEPT + ("needles_1e7",))
def test_the_device_answers_as_the_fold_and_within_the_exact_bounds(ctx, lib, family, placement):
    s, t, p = mesh_rays.placed(family, placement, seed=1)
    rays = mesh_rays.sweep_rays(family, t, N_RAYS, seed=5)
    what = "%s, %s, %d triangles" % (family, placement, len(t))
    ctx.set_scene_mesh(s, t, p)
    got = device_answer(ctx, rays)
    same_bits(got, mesh_rays.linear_fold(lib, s, t, p, rays), what)
    fig = exact_mesh.check_answers(W.triangle_vertices(t), rays, got, len(s) + len(p), what)
    print("\ndevice, %s: %s" % (what, figures(fig)))
    if family != "needles_1e7":
        exact_mesh.assert_shares(fig, what)


def squashed(t, factor=1e-3):
    """The triangles pressed flat towards a plane through the icosphere's centre, across a direction in general position: every
    triangle that was not parallel to it becomes a needle or a sliver"""
    v = W.triangle_vertices(t).astype(np.float64)
    a = np.array([0.36, 0.48, 0.8])
    rel = v - np.array([1.0, 3.0, -16.0])
    return W.with_vertices(t, (v - (1.0 - factor) * (rel @ a)[..., None] * a).astype(np.float32))


@pytest.mark.parametrize("target", ["moved", "far", "squashed"])
def test_after_an_update_the_device_answers_as_the_fold_and_within_the_exact_bounds(ctx, pkg, lib, target):
    s, t, p = mesh_rays.placed("room", "room", seed=1)
    t2 = squashed(t) if target == "squashed" else mesh_rays.placed("room", target, seed=1)[1]
    nodes, order = pkg.binding.mesh_layout(t)
    ctx.set_scene_mesh(s, t, p)
    ctx.update_mesh_vertices(W.triangle_vertices(t2))
    got_nodes, got_order = ctx.mesh_read_layout()
    assert got_nodes.tobytes() == pkg.binding.mesh_refit_layout(t2, nodes, order).tobytes() and np.array_equal(got_order, order)
    rays = mesh_rays.sweep_rays("room", t2, N_RAYS, seed=11)
    got = device_answer(ctx, rays)
    same_bits(got, mesh_rays.linear_fold(lib, s, t2, p, rays), "refit to " + target)
    fig = exact_mesh.check_answers(W.triangle_vertices(t2), rays, got, 0, "refit to " + target)
    print("\ndevice after a refit to %s: %s" % (target, figures(fig)))
    exact_mesh.assert_shares(fig, "refit to " + target)


@pytest.mark.parametrize("case", ["inline", "streams", "glass_tree"])
def test_renders_of_the_moved_room_match_the_mesh_reference(ctx, pkg, ora, ref, case):
    s, t, p = mesh_rays.transformed(room_scene(pkg, glass=case == "glass_tree"), 1.0, MOVE)
    cam = pkg.world.initial_camera()
    cam["position"] = (cam["position"].astype(np.float64) + np.array(MOVE)).astype(np.float32)
    w, h = 67, 45
    start = initial_planes(ora, w, h)
    algorithm = pkg.INLINE if case == "inline" else pkg.STREAMS

    def image(tris):
        ctx.set_scene_mesh(s, tris, p)
        ctx.resize(w, h)
        ctx.upload_state(*start)
        ctx.render(cam, 8, 2, algorithm)
        return ctx.download_state()
    got = image(t)
    with mesh_rays.MeshOracle(ref, t) as mo:
        if case == "inline":
            want, _ = mo.render_inline(s, p, cam, w, h, 8, 2, start, n_threads=THREADS)
        elif case == "glass_tree":
            want = mo.render_streams_tree(s, p, cam, w, h, CAP, 2, start, n_threads=THREADS)[0]
        else:
            want, _ = mo.render_streams(s, p, cam, w, h, CAP, 2, start, n_threads=THREADS)
    assert_planes_equal(got, want, "%s, the room moved by %r" % (case, MOVE))
    assert np.mean(np.asarray(want[0]) != 0) > 0.15
    assert not np.array_equal(np.asarray(image(t[:0])[0]), np.asarray(got[0]))          # not the image of the scene without triangles


def test_the_sphere_hierarchy_answers_as_its_fold_beyond_the_field(ctx, bvh_lib):
    for what, (spheres, planes) in bvh_cases():
        rays = bvh_case_rays(spheres, 100_000)
        ctx.set_scene_bvh(spheres, planes)
        got = device_answer(ctx, rays)
        want = bvh_rays.linear_fold(bvh_lib, spheres, planes, rays)
        (t0, i0, j0), (t1, i1, j1) = got, want
        bad = np.flatnonzero(((t0 != t1) & ~(np.isnan(t0) & np.isnan(t1))) | (i0 != i1) | (j0 != j1))
        assert bad.size == 0, "%s: %d rays differ, first %d: device (%r, %d, %d) fold (%r, %d, %d)" % (
            what, bad.size, bad[0], t0[bad[0]], i0[bad[0]], j0[bad[0]], t1[bad[0]], i1[bad[0]], j1[bad[0]])
        assert j1.sum() > len(rays) // 20, what


@pytest.mark.parametrize("family", ["icosphere", "room"])
def test_the_device_cracks_where_the_restatement_cracks(ctx, lib, family):
    def on_device(s, t, p, rays):
        ctx.set_scene_mesh(s, t, p)
        return device_answer(ctx, rays)
    for placement in mesh_rays.PLACEMENTS:
        n_dev, of = cracks(family, placement, on_device)
        n_cpu, _ = cracks(family, placement, lambda s, t, p, rays: mesh_rays.linear_fold(lib, s, t, p, rays))
        print("\ncracks, %s from inside, %s: device %d, restatement %d of %d edge-aimed rays" % (family, placement, n_dev, n_cpu, of))
        assert n_dev == n_cpu
