"""Mesh scenes (ptmi_set_scene_mesh) on the device: checkHit through the two hierarchies picks what the literal fold over
spheres ++ planes ++ triangles picks (tests/cxx/mesh_traverse.c), a mesh scene without triangles -- or with triangles that only ever
tie with a plane, which keeps the tie -- renders bit for bit what the oracle renders for its spheres and planes in all three per-pixel kernel families, mesh renders
are deterministic and the same in a one-device group, and the context switches representations and refuses what a mesh scene cannot do."""
import os
import sys

import numpy as np
import pytest

from conftest import assert_planes_equal, initial_planes

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_rays  # noqa: E402

pytestmark = pytest.mark.gpu
CAP = 1 << 16
THREADS = max(1, min(16, os.cpu_count() or 1))


@pytest.fixture(scope="module")
def trav(tmp_path_factory):
    return mesh_rays.traverse_lib(tmp_path_factory.mktemp("mesh"))


def same_hits(got, want, what):
    (t0, i0, j0), (t1, i1, j1) = got, want
    bad = np.flatnonzero(((t0 != t1) & ~(np.isnan(t0) & np.isnan(t1))) | (i0 != i1) | (j0 != j1))
    assert bad.size == 0, "%s: %d of %d rays differ, e.g. ray %d: device (%r, %d, %d) cpu (%r, %d, %d)" % (
        what, bad.size, len(t0), bad[0], t0[bad[0]], i0[bad[0]], j0[bad[0]], t1[bad[0]], i1[bad[0]], j1[bad[0]])


def test_eval_check_hit_on_a_mesh_scene_is_the_linear_fold(ctx, trav):
    s, t, p = mesh_rays.adversarial_scene(6, seed=31)
    assert len(t) >= 50_000
    rays = mesh_rays.adversarial_rays(t, 20_000, seed=31)
    ctx.set_scene_mesh(s, t, p)
    got = ctx.eval_check_hit(rays)
    want = mesh_rays.linear_fold(trav, s, t, p, rays)
    same_hits(got, want, "mesh scene, %d triangles" % len(t))
    assert int(np.sum(want[2].astype(bool) & (want[1] >= len(s) + len(p) + 13))) > 2000


def test_eval_check_hit_on_a_million_triangles_is_the_cpu_walk(ctx, trav):
    s, t, p = mesh_rays.adversarial_scene(8, seed=32)
    assert len(t) >= 1_000_000
    rays = mesh_rays.adversarial_rays(t, 100_000, seed=32)
    ctx.set_scene_mesh(s, t, p)
    got = ctx.eval_check_hit(rays)
    want, _ = mesh_rays.walk(trav, s, t, p, rays)
    same_hits(got, want, "mesh scene, %d triangles" % len(t))
    assert int(np.sum(want[2].astype(bool) & (want[1] >= len(s) + len(p) + 13))) > 10_000


def render(c, set_scene, cam, w, h, limit, spp, start, algorithm):
    set_scene()
    c.resize(w, h)
    c.upload_state(*start)
    c.render(cam, limit, spp, algorithm)
    return c.download_state()


def plane_scene(pkg, glass=False):
    """sphere_field(2000) and its 4 planes, plus 4 triangles ON each plane, around its position and with its direction as their
    normal (exactly: axis-aligned, the derived unit normal is the plane's direction bit for bit).  A ray meets such a triangle exactly
    where it meets its plane, at the same key by the same operations, and the plane -- the earlier primitive -- keeps every tie: no
    triangle is ever selected, and the render is the spheres and planes' -> (spheres, planes, triangles)"""
    s, p = pkg.world.sphere_field(2000, seed=41, glass_fraction=0.1 if glass else 0.0)
    K = 1024.0
    tris = []
    for q in p:
        pos, n = q["position"].astype(np.float32), q["direction"].astype(np.float32)
        a = np.roll(n, 1)                                # a, b axis-aligned with a x b = n
        b = np.cross(n, a).astype(np.float32)
        for u, w in ((a, b), (b, -a), (-a, -b), (-b, a)):
            tris.append(pkg.world.triangle(tuple(pos), tuple(pos + K * u), tuple(pos + K * w), (1.0, 1.0, 1.0), 100.0, pkg.world.MATTE, 1.0))
    return s, p, np.array(tris, dtype=pkg.world.TRIANGLE_DTYPE)


@pytest.mark.parametrize("algorithm, glass, limit", [("INLINE", False, 8), ("INLINE", False, 3), ("STREAMS", False, 8), ("STREAMS", True, 8)])
def test_no_triangles_and_triangles_on_the_planes_render_what_the_oracle_renders(ctx, pkg, ora, algorithm, glass, limit):
    s, p, t = plane_scene(pkg, glass)
    cam = pkg.world.initial_camera()
    w, h, spp = 72, 40, 2
    start = initial_planes(ora, w, h)
    alg = getattr(pkg, algorithm)
    if algorithm == "INLINE":
        want, _ = ora.render_inline(s, p, cam, w, h, limit, spp, start, n_threads=THREADS)
    elif glass:
        want = ora.render_streams_tree(s, p, cam, w, h, CAP, spp, start, n_threads=THREADS)[0]
    else:
        want, _ = ora.render_streams(s, p, cam, w, h, CAP, spp, start, n_threads=THREADS)
    none = render(ctx, lambda: ctx.set_scene_mesh(s, t[:0], p), cam, w, h, limit, spp, start, alg)
    assert_planes_equal(none, want, "%s, mesh scene without triangles" % algorithm)
    far = render(ctx, lambda: ctx.set_scene_mesh(s, t, p), cam, w, h, limit, spp, start, alg)
    assert_planes_equal(far, want, "%s, triangles on the planes" % algorithm)


def mesh_image(c, pkg, scene, w, h, limit, spp, alg, seed=3):
    c.set_scene_mesh(*scene)
    c.resize(w, h)
    c.init_output(seed)
    c.render(pkg.world.initial_camera(), limit, spp, alg)
    return c.download_state()


@pytest.mark.parametrize("algorithm", ["INLINE", "STREAMS"])
def test_mesh_renders_are_deterministic_lit_and_the_same_in_a_group(pkg, algorithm):
    alg = getattr(pkg, algorithm)
    scene = pkg.world.mesh_room(4, seed=1)
    w, h = 67, 45                                        # ragged: neither rows of 64 nor whole 8 x 8 tiles
    with pkg.Context(0) as c:
        a = mesh_image(c, pkg, scene, w, h, 8, 4, alg)
        b = mesh_image(c, pkg, scene, w, h, 8, 4, alg)
        for x, y in zip(a, b):
            assert np.array_equal(np.asarray(x).view(np.uint32), np.asarray(y).view(np.uint32))
        rgb = np.stack([np.asarray(x) for x in a[:3]])
        assert np.all(np.isfinite(rgb)) and np.mean(rgb != 0) > 0.3         # the room's ceiling and light glow: most pixels see light
        without = mesh_image(c, pkg, (scene[0], scene[1][:13], scene[2]), w, h, 8, 4, alg)
        assert not np.array_equal(np.asarray(without[0]), np.asarray(a[0]))  # the icosphere is there
    with pkg.Group([0], 0) as g:                           # a one-device group renders the same image
        g.set_scene_mesh(*scene)
        g.resize(w, h)
        g.init_output(3)
        g.render(pkg.world.initial_camera(), 8, 4, alg)
        g.synchronize()
        got = g.download_color()
    assert_planes_equal(got, a[:3], "group of 1, mesh scene")


def test_glass_triangles_take_the_tree_walk(pkg):
    s, t, p = pkg.world.mesh_room(3, seed=2)
    t = t.copy()
    t["brdf_tag"][13:] = pkg.world.GLASS
    t["brdf_param"][13:] = 1.5
    with pkg.Context(0) as c:
        a = mesh_image(c, pkg, (s, t, p), 48, 32, 8, 2, pkg.STREAMS)
        b = mesh_image(c, pkg, (s, t, p), 48, 32, 8, 2, pkg.STREAMS)
        assert all(np.array_equal(np.asarray(x).view(np.uint32), np.asarray(y).view(np.uint32)) for x, y in zip(a, b))
        assert np.all(np.isfinite(np.stack([np.asarray(x) for x in a[:3]])))
        with pytest.raises(pkg.binding.PtmiError):
            c.render(pkg.world.initial_camera(), 8, 1, pkg.INLINE)               # GLASS needs Streams, as for every scene


def test_switching_failures_and_refusals(pkg, ora):
    B = pkg.binding
    s, p, t = plane_scene(pkg)
    small = pkg.world.scene16()
    cam = pkg.world.initial_camera()
    w, h = 48, 32
    start = initial_planes(ora, w, h)
    want_box, _ = ora.render_inline(s, p, cam, w, h, 8, 2, start, n_threads=THREADS)
    want_small, _ = ora.render_inline(small[0], small[1], cam, w, h, 8, 2, start)
    with pkg.Context(0) as c:
        c.resize(w, h)

        def image():
            c.upload_state(*start)
            c.render(cam, 8, 2)
            return c.download_state()
        c.set_scene_mesh(s, t, p)
        assert_planes_equal(image(), want_box, "mesh")
        c.set_scene_bvh(s, p)
        assert_planes_equal(image(), want_box, "mesh -> BVH")
        c.set_scene(*small)
        assert_planes_equal(image(), want_small, "BVH -> linear")
        c.set_scene_mesh(s, t, p)
        assert_planes_equal(image(), want_box, "linear -> mesh")
        # failures leave the mesh scene as it was
        bad = t.copy()
        bad["v1"][5, 2] = np.nan
        for args, code in (((s, bad, p), B.PTMI_EINVAL), ((s, t, np.repeat(p, 17)), B.PTMI_ELIMIT),
                           ((s[:0], t[:0], p[:0]), B.PTMI_EINVAL)):
            with pytest.raises(B.PtmiError) as e:
                c.set_scene_mesh(*args)
            assert e.value.code == code
        assert_planes_equal(image(), want_box, "after refused mesh scenes")
        with pytest.raises(B.PtmiError):
            c.set_variant(5)
        with pytest.raises(B.PtmiError):
            c.set_option(B.OPT_STREAMS_FORM, B.FORM_STREAM)
        flat = t.copy()
        flat["v2"] = flat["v0"]                          # zero area: accepted, never hit
        c.set_scene_mesh(s, flat, p)
        assert_planes_equal(image(), want_box, "zero-area triangles")
        c.set_scene(*small)
        c.set_variant(5)
        with pytest.raises(B.PtmiError) as e:
            c.set_scene_mesh(s, t, p)
        assert e.value.code == B.PTMI_EINVAL
        c.set_variant(0)
        assert_planes_equal(image(), want_small, "a refused mesh scene leaves the linear one")


def test_the_ablation_library_refuses_mesh_scenes(pkg, ablations):
    with pkg.Context(0, library=ablations) as c:
        with pytest.raises(pkg.binding.PtmiError) as e:
            c.set_scene_mesh(*pkg.world.mesh_room(0))
        assert e.value.code == pkg.binding.PTMI_EINVAL
