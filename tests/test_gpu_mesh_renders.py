"""Mesh scenes (ptmi_set_scene_mesh) rendered on the device with triangles HIT, against an independent CPU reference: the oracle's own
render loops with the mesh checkHit (tests/cxx/mesh_reference.c: the literal fold over spheres ++ planes ++ triangles, a triangle's hit
record from its unit normal and its own material).  Bit for bit on all seven planes: Inline at two bounce limits, the Streams chain under
both seed rules, the GLASS tree walk with glass triangles, ragged image sizes, render1 / render1_chained, and a partitioned context whose
stitched parts equal the whole.  Also: with no triangles, check_hit_mesh's sphere walk and plane fold answer exactly as
check_hit_bvh does."""
import os
import sys

import numpy as np
import pytest

from conftest import assert_planes_equal, initial_planes

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bvh_rays  # noqa: E402
import mesh_rays  # noqa: E402

pytestmark = pytest.mark.gpu
CAP = 1 << 16
THREADS = max(1, min(16, os.cpu_count() or 1))


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return mesh_rays.reference_lib(tmp_path_factory.mktemp("meshref"))


def scene(pkg, glass=False):
    """world.mesh_room(3) (1 293 triangles, 8 spheres) and one plane, a raised floor: triangle k is primitive 9 + k, so a material
    or normal looked up one primitive off shows.  glass: the icosphere's triangles are GLASS."""
    W = pkg.world
    s, t, _ = W.mesh_room(3, seed=7)
    p = np.array([W.plane((0.0, -2.5, 0.0), (0.0, 1.0, 0.0), (0.6, 0.8, 0.6), 0.0, W.MATTE, 0.9)], dtype=W.PLANE_DTYPE)
    if glass:
        t = t.copy()
        t["brdf_tag"][13:] = W.GLASS
        t["brdf_param"][13:] = 1.5
        t["color"][13:] = (0.95, 0.95, 0.95)
    return s, t, p


def render(c, sc, cam, w, h, limit, spp, start, algorithm):
    c.set_scene_mesh(*sc)
    c.resize(w, h)
    c.upload_state(*start)
    c.render(cam, limit, spp, algorithm)
    return c.download_state()


@pytest.mark.parametrize("limit, w, h", [(8, 67, 45), (3, 64, 16)])
def test_inline_with_triangles_hit_matches_the_mesh_reference(ctx, pkg, ora, ref, limit, w, h):
    sc = scene(pkg)
    cam = pkg.world.initial_camera()
    start = initial_planes(ora, w, h)
    got = render(ctx, sc, cam, w, h, limit, 2, start, pkg.INLINE)
    with mesh_rays.MeshOracle(ref, sc[1]) as mo:
        want, _ = mo.render_inline(sc[0], sc[2], cam, w, h, limit, 2, start, n_threads=THREADS)
    assert_planes_equal(got, want, "Inline with triangles, limit %d, %dx%d" % (limit, w, h))
    assert np.mean(np.asarray(want[0]) != 0) > 0.15                      # lit: paths meet the triangle light and the ceiling (24 % at limit 3)
    # triangles are really hit: the image differs from the one without them
    ctx.set_scene_mesh(sc[0], sc[1][:0], sc[2])
    ctx.upload_state(*start)
    ctx.render(cam, limit, 2, pkg.INLINE)
    assert not np.array_equal(np.asarray(ctx.download_state()[0]), np.asarray(got[0]))


@pytest.mark.parametrize("rule", ["keep", "from_result"])
def test_streams_chain_with_triangles_hit_matches_the_mesh_reference(ctx, pkg, ora, ref, rule):
    B = pkg.binding
    sc = scene(pkg)
    cam = pkg.world.initial_camera()
    w, h = 61, 37
    start = initial_planes(ora, w, h)
    value = {"keep": B.SEED_KEEP_ACCUMULATOR, "from_result": B.SEED_FROM_RESULT}[rule]
    ctx.set_option(B.OPT_STREAMS_SEED_RULE, value)
    try:
        got = render(ctx, sc, cam, w, h, 8, 2, start, pkg.STREAMS)
    finally:
        ctx.set_option(B.OPT_STREAMS_SEED_RULE, B.SEED_AUTO)
    ora_rule = {"keep": ora.SEED_KEEP_ACCUMULATOR, "from_result": ora.SEED_FROM_RESULT}[rule]
    with mesh_rays.MeshOracle(ref, sc[1]) as mo:
        want, _ = mo.render_streams(sc[0], sc[2], cam, w, h, CAP, 2, start, seed_rule=ora_rule, n_threads=THREADS)
    assert_planes_equal(got, want, "Streams chain with triangles, seed rule %s" % rule)


def test_glass_triangles_in_the_tree_walk_match_the_mesh_reference(ctx, pkg, ora, ref):
    sc = scene(pkg, glass=True)
    cam = pkg.world.initial_camera()
    w, h = 72, 40
    start = initial_planes(ora, w, h)
    got = render(ctx, sc, cam, w, h, 8, 2, start, pkg.STREAMS)
    with mesh_rays.MeshOracle(ref, sc[1]) as mo:
        want = mo.render_streams_tree(sc[0], sc[2], cam, w, h, CAP, 2, start, n_threads=THREADS)[0]
    assert_planes_equal(got, want, "tree walk with GLASS triangles")


def test_render1_and_render1_chained_match_the_mesh_reference(ctx, pkg, ora, ref):
    sc = scene(pkg)
    cam = pkg.world.initial_camera()
    w, h = 40, 24
    start = initial_planes(ora, w, h)
    with mesh_rays.MeshOracle(ref, sc[1]) as mo:
        want, _ = mo.render_inline(sc[0], sc[2], cam, w, h, 8, 1, start, n_threads=THREADS)
    ctx.set_scene_mesh(*sc)
    tok, fetched = ctx.render1_chained(cam, 8, w, h, 0, planes_in=start, fetch=("r", "g", "b", "sa", "sb", "sc", "sctr"))
    assert tok != 0
    assert_planes_equal([fetched[k] for k in ("r", "g", "b", "sa", "sb", "sc", "sctr")], want, "render1_chained, mesh scene")
    assert_planes_equal(ctx.render1(cam, 8, w, h, start), want, "render1, mesh scene")


def test_partitioned_context_stitches_the_mesh_reference(pkg, ora, ref):
    sc = scene(pkg)
    cam = pkg.world.initial_camera()
    w, h, n_parts, stripe = 48, 50, 3, 4
    start = initial_planes(ora, w, h)
    with mesh_rays.MeshOracle(ref, sc[1]) as mo:
        want, _ = mo.render_inline(sc[0], sc[2], cam, w, h, 8, 2, start, n_threads=THREADS)
    stitched = [np.zeros_like(p) for p in want]
    for part in range(n_parts):
        with pkg.Context(0) as c:
            c.set_scene_mesh(*sc)
            c.set_partition(stripe, n_parts, part)
            c.resize(w, h)
            rows = c.global_rows()
            c.init_output(0x5EED1234)
            c.render(cam, 8, 2)
            for dst, src in zip(stitched, c.download_state()):
                dst[rows] = src
    assert_planes_equal(stitched, want, "%d stripes, mesh scene" % n_parts)


def test_without_triangles_check_hit_mesh_answers_as_check_hit_bvh(ctx):
    """check_hit_mesh runs check_hit_bvh's sphere walk and plane fold before its triangles, behind an admission test of its own:
    the two must answer the same, bit for bit, on the BVH tests' adversarial rays."""
    spheres, planes = bvh_rays.adversarial_scene(20000, seed=51)
    rays = bvh_rays.adversarial_rays(spheres, 100_000, seed=51)
    ctx.set_scene_bvh(spheres, planes)
    want = ctx.eval_check_hit(rays)
    ctx.set_scene_mesh(spheres, np.zeros(0, mesh_rays.world.TRIANGLE_DTYPE), planes)
    got = ctx.eval_check_hit(rays)
    for a, b, name in zip(got, want, ("t", "idx", "just")):
        assert np.array_equal(np.asarray(a).view(np.uint32), np.asarray(b).view(np.uint32)), name
    assert want[2].sum() > 20_000
