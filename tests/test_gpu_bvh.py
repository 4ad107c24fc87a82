"""BVH scenes (ptmi_set_scene_bvh) on the device: checkHit through the hierarchy picks what the oracle's linear fold picks, the three
per-pixel kernels render bit for bit what the oracle renders, a scene renders the same as a BVH scene and as a linear one, and the
context switches representations, keeps its scene through failures and refuses what a BVH scene cannot do."""
import os
import sys

import numpy as np
import pytest

from conftest import assert_planes_equal, initial_planes

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bvh_rays  # noqa: E402

pytestmark = pytest.mark.gpu
CAP = 1 << 16          # the default step cap of render Streams (PTMI_OPT_STREAM_STEP_CAP)
THREADS = max(1, min(16, os.cpu_count() or 1))


@pytest.fixture(scope="module")
def trav(tmp_path_factory):
    return bvh_rays.traverse_lib(tmp_path_factory.mktemp("bvh"))


def same_hits(got, want, what, bitwise=False):
    (t0, i0, j0), (t1, i1, j1) = got, want
    # t: equal as numbers -- against the oracle two encodings differ where the value cannot: a NaN key (a NaN origin: the literal
    # fold) is the host's default NaN (sign bit set) or the device's, and for a ray that starts exactly on a sphere (tca = -0, x = 0)
    # the oracle's min(t0, t1) is +0 where the device's t0 is -0 (the same hit position).  BVH against linear on the device: bit for bit.
    same_t = (t0.view(np.uint32) == t1.view(np.uint32)) if bitwise else ((t0 == t1) | (np.isnan(t0) & np.isnan(t1)))
    bad = np.flatnonzero(~same_t | (i0 != i1) | (j0 != j1))
    assert bad.size == 0, "%s: %d of %d rays differ, e.g. ray %d: device (%r, %d, %d) oracle (%r, %d, %d)" % (
        what, bad.size, len(t0), bad[0], t0[bad[0]], i0[bad[0]], j0[bad[0]], t1[bad[0]], i1[bad[0]], j1[bad[0]])


def test_eval_check_hit_on_a_bvh_scene_is_the_linear_fold(ctx, trav):
    spheres, planes = bvh_rays.adversarial_scene(50000, seed=11)
    rays = bvh_rays.adversarial_rays(spheres, 100_000, seed=11)
    ctx.set_scene_bvh(spheres, planes)
    got = ctx.eval_check_hit(rays)
    want = bvh_rays.linear_fold(trav, spheres, planes, rays)
    same_hits(got, want, "BVH scene, 50k spheres")
    assert want[2].sum() > 20_000


def test_eval_check_hit_on_a_linear_scene_is_the_linear_fold(ctx, trav):
    spheres, planes = bvh_rays.adversarial_scene(900, seed=12)
    assert len(spheres) + len(planes) <= 1024
    rays = bvh_rays.adversarial_rays(spheres, 100_000, seed=12)
    ctx.set_scene(spheres, planes)
    lin = ctx.eval_check_hit(rays)
    same_hits(lin, bvh_rays.linear_fold(trav, spheres, planes, rays), "linear scene")
    ctx.set_scene_bvh(spheres, planes)
    tree = ctx.eval_check_hit(rays)
    same_hits(tree, bvh_rays.linear_fold(trav, spheres, planes, rays), "the same scene as a BVH scene")
    same_hits(tree, lin, "BVH against linear on the device", bitwise=True)


def render(c, pkg, scene, cam, w, h, limit, spp, start, algorithm, bvh=True):
    (c.set_scene_bvh if bvh else c.set_scene)(*scene)
    c.resize(w, h)
    c.upload_state(*start)
    c.render(cam, limit, spp, algorithm)
    return c.download_state()


@pytest.mark.parametrize("n, w, h, limit, spp", [(2000, 72, 40, 8, 3), (20000, 40, 24, 8, 2), (2000, 64, 16, 0, 2), (2000, 64, 16, 8, 0)])
def test_render_inline_on_a_bvh_scene_matches_the_oracle(ctx, pkg, ora, n, w, h, limit, spp):
    scene = pkg.world.sphere_field(n, seed=n)
    cam = pkg.world.initial_camera()
    start = initial_planes(ora, w, h)
    got = render(ctx, pkg, scene, cam, w, h, limit, spp, start, pkg.INLINE)
    want, _ = ora.render_inline(scene[0], scene[1], cam, w, h, limit, spp, start, n_threads=THREADS)
    assert_planes_equal(got, want, "Inline, %d spheres, limit %d spp %d" % (n, limit, spp))


def test_render_streams_on_a_bvh_scene_matches_the_oracle(ctx, pkg, ora):
    scene = pkg.world.sphere_field(2000, seed=21)
    cam = pkg.world.initial_camera()
    w, h, spp = 72, 40, 2
    start = initial_planes(ora, w, h)
    got = render(ctx, pkg, scene, cam, w, h, 8, spp, start, pkg.STREAMS)
    want, _ = ora.render_streams(scene[0], scene[1], cam, w, h, CAP, spp, start, n_threads=THREADS)
    assert_planes_equal(got, want, "Streams, 2000 spheres")


def test_render_streams_with_glass_on_a_bvh_scene_matches_the_tree_walk_oracle(ctx, pkg, ora):
    scene = pkg.world.sphere_field(2000, seed=22, glass_fraction=0.1)
    assert np.any(scene[0]["brdf_tag"] == pkg.world.GLASS)
    cam = pkg.world.initial_camera()
    w, h, spp = 72, 40, 2
    start = initial_planes(ora, w, h)
    got = render(ctx, pkg, scene, cam, w, h, 8, spp, start, pkg.STREAMS)
    want = ora.render_streams_tree(scene[0], scene[1], cam, w, h, CAP, spp, start, n_threads=THREADS)[0]
    assert_planes_equal(got, want, "Streams with GLASS (tree walk), 2000 spheres")


def test_render1_chained_on_a_bvh_scene_matches_the_oracle(ctx, pkg, ora):
    scene = pkg.world.sphere_field(3000, seed=23)
    cam = pkg.world.initial_camera()
    w, h = 40, 24
    start = initial_planes(ora, w, h)
    ctx.set_scene_bvh(*scene)
    tok, fetched = ctx.render1_chained(cam, 8, w, h, 0, planes_in=start, fetch=("r", "g", "b", "sa", "sb", "sc", "sctr"))
    assert tok != 0
    got = [fetched[k] for k in ("r", "g", "b", "sa", "sb", "sc", "sctr")]
    want, _ = ora.render_inline(scene[0], scene[1], cam, w, h, 8, 1, start, n_threads=THREADS)
    assert_planes_equal(got, want, "render1_chained, BVH scene")
    got1 = ctx.render1(cam, 8, w, h, start)
    assert_planes_equal(got1, want, "render1, BVH scene")


def test_a_million_spheres(ctx, pkg, ora):
    scene = pkg.world.sphere_field(1_000_000, seed=24)
    cam = pkg.world.initial_camera()
    w, h = 32, 16
    start = initial_planes(ora, w, h)
    got = render(ctx, pkg, scene, cam, w, h, 4, 1, start, pkg.INLINE)
    want, _ = ora.render_inline(scene[0], scene[1], cam, w, h, 4, 1, start, n_threads=THREADS)
    assert_planes_equal(got, want, "Inline, 10^6 spheres")


def test_at_the_primitive_limit_bvh_and_linear_render_the_same(ctx, pkg, ora):
    scene = pkg.world.sphere_field(1020, seed=25)
    assert len(scene[0]) + len(scene[1]) == 1024
    cam = pkg.world.initial_camera()
    w, h = 96, 64
    start = initial_planes(ora, w, h)
    for algorithm in (pkg.INLINE, pkg.STREAMS):
        lin = render(ctx, pkg, scene, cam, w, h, 8, 3, start, algorithm, bvh=False)
        tree = render(ctx, pkg, scene, cam, w, h, 8, 3, start, algorithm, bvh=True)
        assert_planes_equal(tree, lin, "BVH against linear, 1024 primitives, algorithm %d" % algorithm)


def test_switching_failures_and_refusals(pkg, ora):
    B = pkg.binding
    small = pkg.world.scene16()
    field = pkg.world.sphere_field(3000, seed=26)
    cam = pkg.world.initial_camera()
    w, h = 48, 32
    start = initial_planes(ora, w, h)
    want_small, _ = ora.render_inline(small[0], small[1], cam, w, h, 8, 2, start)
    want_field, _ = ora.render_inline(field[0], field[1], cam, w, h, 8, 2, start, n_threads=THREADS)
    with pkg.Context(0) as c:
        c.resize(w, h)

        def image():
            c.upload_state(*start)
            c.render(cam, 8, 2)
            return c.download_state()
        c.set_scene(*small)
        assert_planes_equal(image(), want_small, "linear")
        c.set_scene_bvh(*field)
        assert_planes_equal(image(), want_field, "linear -> BVH")
        c.set_scene(*small)
        assert_planes_equal(image(), want_small, "BVH -> linear")
        c.set_scene_bvh(*field)
        # failures leave the scene as it was
        too_many_planes = np.repeat(field[1], 17)
        with pytest.raises(B.PtmiError) as e:
            c.set_scene_bvh(field[0], too_many_planes)
        assert e.value.code == B.PTMI_ELIMIT
        nan = field[0].copy()
        nan["position"][5, 2] = np.nan
        with pytest.raises(B.PtmiError) as e:
            c.set_scene_bvh(nan, field[1])
        assert e.value.code == B.PTMI_EINVAL
        assert_planes_equal(image(), want_field, "BVH after failed set_scene_bvh")
        with pytest.raises(B.PtmiError) as e:
            c.set_scene(field[0], field[1])                                # (the linear limit stands)
        assert e.value.code == B.PTMI_ELIMIT
        assert_planes_equal(image(), want_field, "BVH after a failed set_scene")
        # what a BVH scene refuses
        for call in (lambda: c.set_option(B.OPT_STREAMS_FORM, B.FORM_STREAM), lambda: c.set_variant(13)):
            with pytest.raises(B.PtmiError) as e:
                call()
            assert e.value.code == B.PTMI_EINVAL
        c.set_option(B.OPT_STREAMS_FORM, B.FORM_PIXEL)
        c.set_scene(*small)
        c.set_option(B.OPT_STREAMS_FORM, B.FORM_STREAM)
        with pytest.raises(B.PtmiError) as e:
            c.set_scene_bvh(*field)
        assert e.value.code == B.PTMI_EINVAL
        c.set_option(B.OPT_STREAMS_FORM, B.FORM_AUTO)
        c.set_variant(5)
        with pytest.raises(B.PtmiError) as e:
            c.set_scene_bvh(*field)
        assert e.value.code == B.PTMI_EINVAL
        c.set_variant(0)
        assert_planes_equal(image(), want_small, "linear after refused set_scene_bvh")


def test_the_ablation_library_refuses_bvh_scenes(pkg, ablations):
    with pkg.Context(0, library=ablations) as c:
        with pytest.raises(pkg.binding.PtmiError) as e:
            c.set_scene_bvh(*pkg.world.sphere_field(100, seed=1))
        assert e.value.code == pkg.binding.PTMI_EINVAL


def test_group_set_scene_bvh_host_readout_equals_the_ungrouped_image(pkg):
    sp, pl = pkg.world.sphere_field(5000, seed=27)
    cam = pkg.world.initial_camera()
    w, h = 133, 71
    with pkg.Context(0) as c:
        c.set_scene_bvh(sp, pl)
        c.resize(w, h)
        c.init_output(7)
        c.render(cam, 8, 3)
        want = c.download_state()
    with pkg.Group([0], 0) as g:
        g.set_scene_bvh(sp, pl)
        g.resize(w, h)
        g.init_output(7)
        g.render(cam, 8, 2)
        g.render(cam, 8, 1)
        g.synchronize()
        got = g.download_color()
    assert_planes_equal(got, want[:3], "group of 1, BVH scene")


def test_glass_tree_walk_with_hit_indices_beyond_16_bits_matches_the_oracle(ctx, pkg, ora):
    """The tree walk keeps each start hit's primitive in one word with its steps and draws; a BVH scene's primitives need more than the
    16 bits a linear scene's do.  A field of 72 000 spheres ordered far to near, so that every sphere the camera sees has an index above
    65 535, a quarter of the near ones GLASS (glass primary hits: the start record's children), against the oracle's tree walk."""
    spheres, planes = pkg.world.sphere_field(72000, seed=28)
    cam = pkg.world.initial_camera()
    far_to_near = np.argsort(-np.linalg.norm(spheres["position"] - cam["position"], axis=1), kind="stable")
    spheres = spheres[far_to_near].copy()
    near = np.arange(len(spheres)) >= 65536
    glass = near & (np.random.default_rng(28).random(len(spheres)) < 0.25)
    spheres["brdf_tag"][glass] = pkg.world.GLASS
    spheres["brdf_param"][glass] = 1.5
    spheres["color"][glass] = (0.95, 0.95, 0.95)
    spheres["illuminance"][glass] = 0.0
    w, h, spp = 40, 24, 2
    start = initial_planes(ora, w, h)
    ctx.set_scene_bvh(spheres, planes)
    # the camera's rays do hit spheres beyond index 65535, GLASS ones among them
    rng = np.random.default_rng(1)
    dirs = rng.normal(size=(4096, 3)) * (1.0, 0.5, 1.0) + (0.0, 0.0, -2.0)
    dirs = (dirs / np.linalg.norm(dirs, axis=1, keepdims=True)).astype(np.float32)
    rays = np.hstack([np.repeat(cam["position"][None, :], len(dirs), 0), dirs]).astype(np.float32)
    _, idx, just = ctx.eval_check_hit(rays)
    hit = idx[(just == 1) & (idx < len(spheres))]
    assert np.sum(hit >= 65536) > 500 and np.sum(glass[hit]) > 50, (np.sum(hit >= 65536), np.sum(glass[hit]))
    got = render(ctx, pkg, (spheres, planes), cam, w, h, 8, spp, start, pkg.STREAMS)
    want = ora.render_streams_tree(spheres, planes, cam, w, h, CAP, spp, start, n_threads=THREADS)[0]
    assert_planes_equal(got, want, "Streams with GLASS (tree walk), hit indices beyond 65535")
