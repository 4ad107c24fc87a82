"""The x-y terms of check_hit's sphere test, kept across spheres that share cx and cy (csrc/ptmi_device.h, SphereShare::kXY; the scene's
mask: csrc/ptmi_share.h).  A sphere whose centre has its predecessor's cx and cy BITS takes the predecessor's lx dx + ly dy and
lx lx + ly ly and makes the rest of the test as every sphere does: the same operations on the same operands, so every case compares
with the oracle bit for bit -- (t, index, Just) of hand-made rays through ctx.eval_check_hit (the plain walk, two spheres a trip)
against the oracle's fold, and all seven planes of a render of 64 x 48 pixels, 4 spp, limit 8 (the staged walk, four spheres a trip;
past the LDS limit the plain walk) through every kernel family that shares (FORMS): render Inline (profiles/shared_xy_ab.txt).  A scene
without runs (a run of 1 below) goes to the kernels that share nothing (render_inline_kernel_plain, the point query's kNone form).  The
Streams chain, the tree walk and the stream form run the whole test at every sphere (experiments/shared_xy/) and are held to the oracle
by tests/test_gpu_sphere_pass.py."""
import numpy as np
import pytest

from conftest import assert_planes_equal, initial_planes
from test_gpu_sphere_pass import check_rays, check_render, colour_of, render_gpu, skewer, skewer_rays

pytestmark = pytest.mark.gpu
W_, H_, SPP, LIMIT = 64, 48, 4, 8
FORMS = (("inline", "INLINE"),)    # check_render's name and the package's algorithm of every form that shares


def spheres_of(pkg, centres, radii=None):
    """Spheres at `centres`, colours distinct by index, every third one glowing, matte and glossy in turns"""
    W = pkg.world
    return np.array([W.sphere(tuple(c), (radii[i] if radii is not None else 1.0), colour_of(i), 4.0 if i % 3 == 0 else 0.0,
                              W.GLOSSY if i % 2 else W.MATTE, 0.8) for i, c in enumerate(centres)], dtype=W.SPHERE_DTYPE)


def row_scene(pkg, n, start, length, run_xy=(0.5, -0.25)):
    """n spheres, one behind the other in z and spread in x and y, except those of [start, start + length): they stand at run_xy, the
    farther the larger, so that each shows around the one in front of it.  mainScene's planes around them."""
    centres, radii = [], []
    for i in range(n):
        in_run = start <= i < start + length
        centres.append((run_xy[0], run_xy[1], -7.0 - 1.5 * i) if in_run else (-5.5 + 1.4 * i, 1.1 * (i % 3 - 1), -7.0 - 1.5 * i))
        radii.append(0.5 + 0.2 * (i - start) if in_run else 0.8)
    return spheres_of(pkg, centres, radii), pkg.world.main_scene()[1]


def query_rays(ora, cam, scene):
    """The 8 x 8 primary rays, then rays from the camera at and beside every sphere in turn (64 of them)"""
    rays = [np.concatenate(ora.primary_ray(cam, 8, 8, x, y)) for y in range(8) for x in range(8)]
    ns = len(scene[0])
    for n in range(64 if ns else 0):
        s, m = scene[0][n % ns], n // ns
        aim = s["position"].astype(np.float64) + 0.6 * float(s["radius"]) * np.array([m % 3 - 1, (m // 3) % 3 - 1, 0.0])
        d = aim - cam["position"]
        rays.append(np.concatenate([cam["position"], (d / np.linalg.norm(d)).astype(np.float32)]))
    return np.array(rays, np.float32)


def check_scene(ctx, pkg, ora, scene, what, cam=None, w=W_, h=H_):
    cam = pkg.world.initial_camera() if cam is None else cam
    check_rays(ctx, ora, scene, query_rays(ora, cam, scene), what)
    return render_forms(ctx, pkg, ora, scene, cam, w, h, SPP, what)


def render_forms(ctx, pkg, ora, scene, cam, w, h, spp, what):
    """Every sharing form against the oracle; render Inline's planes"""
    return [check_render(ctx, pkg, ora, scene, cam, w, h, spp, how, what, LIMIT) for how, _ in FORMS][0]


# ---- 1. the benchmark's scene

def test_s16_as_it_is(ctx, pkg, ora):
    spheres, planes = pkg.world.scene16()
    xy = spheres["position"][:, :2].copy().view(np.uint32)
    shared = [i for i in range(1, len(spheres)) if np.array_equal(xy[i], xy[i - 1])]
    assert shared == [6, 7, 9, 10, 12, 13]                  # three runs of three behind mainScene's five
    got = check_scene(ctx, pkg, ora, (spheres, planes), "S16")
    assert np.any(got[0] != 0.0)


# ---- 2. runs against every unroll tail of both walks

@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 6, 7, 8, 9])
def test_runs_at_every_index_and_every_unroll_tail(ctx, pkg, ora, n):
    """Runs of 1 to 5 spheres from every index on (so every index modulo 4, index 0 and the last sphere included) in scenes of n
    spheres: the staged walk takes four spheres a trip, then two, then one, the plain walk two and one, and each trip shifts the mask
    by its spheres -- a run begins, continues and ends in every position of every trip."""
    cam = pkg.world.initial_camera()
    for start in range(n):
        for length in range(1, 6):
            if start + length > n:
                break
            scene = row_scene(pkg, n, start, length)
            check_scene(ctx, pkg, ora, scene, "%d spheres, run of %d at %d" % (n, length, start), cam)


def test_two_runs_back_to_back(ctx, pkg, ora):
    """... and a run that ends where the next begins: sphere 3 must compute its own terms, not keep sphere 2's"""
    centres = [(-1.5, 0.5, -8.0), (-1.5, 0.5, -10.0), (-1.5, 0.5, -12.5), (1.5, -0.5, -8.0), (1.5, -0.5, -10.0), (1.5, -0.5, -12.5), (0.0, 2.0, -9.0)]
    scene = (spheres_of(pkg, centres, [0.6, 0.9, 1.3, 0.6, 0.9, 1.3, 0.7]), pkg.world.main_scene()[1])
    check_scene(ctx, pkg, ora, scene, "two runs")


# ---- 3. what must not share

@pytest.mark.parametrize("which", ["cx", "cy"])
def test_neighbours_equal_in_one_coordinate_only_do_not_share(ctx, pkg, ora, which):
    centres = [(1.0, -1.0 + 1.3 * i, -8.0 - 1.5 * i) if which == "cx" else (-3.0 + 2.0 * i, 0.5, -8.0 - 1.5 * i) for i in range(4)]
    scene = (spheres_of(pkg, centres, [0.9] * 4), pkg.world.main_scene()[1])
    check_scene(ctx, pkg, ora, scene, "equal in %s only" % which)


@pytest.mark.parametrize("first", [0.0, -0.0])
def test_zeros_of_either_sign_do_not_share(ctx, pkg, ora, first):
    """cx = +0 and cx = -0 are equal values with different bits: (+0) - ox and (-0) - ox differ for ox = +-0, so the second sphere
    computes its own lx.  Rays from ox = +0 and ox = -0, along the axis and oblique; the render's camera stands at x = +0.
    This case holds the RESULT to the oracle; it could not tell a mask that compares values from one that compares bits: in these rays
    the shared terms differ at most in the sign of a zero, which the nonzero lz dz absorbs.  That the mask compares bits is what the
    host program checks (tests/cxx/shared_xy_mask_main.cpp, tests/test_shared_xy_mask_host.py)."""
    zeros = [np.float32(first), -np.float32(first), np.float32(first)]
    centres = [(zeros[i], 0.0, -8.0 - 2.0 * i) for i in range(3)]
    spheres = spheres_of(pkg, centres, [0.6, 0.9, 1.3])
    assert [bool(np.signbit(c)) for c in spheres["position"][:, 0]] == [bool(np.signbit(z)) for z in zeros]
    scene = (spheres, pkg.world.main_scene()[1])
    oblique = np.array([0.02, 0.05, -1.0]) / np.linalg.norm([0.02, 0.05, -1.0])
    rays = []
    for ox in (0.0, -0.0):
        for oy in (0.0, 0.3, 0.7, 1.0):
            rays.append((ox, oy, 0.0, 0.0, 0.0, -1.0))
            rays.append((ox, oy, 0.0, -0.0, -0.0, -1.0))
            rays.append((ox, oy, 0.0) + tuple(oblique))
            rays.append((ox, oy, -20.0, 0.0, 0.0, 1.0))
    rays = np.array(rays, np.float32)
    assert np.signbit(rays[len(rays) // 2:, 0]).all() and not np.signbit(rays[:len(rays) // 2, 0]).any()
    check_rays(ctx, ora, scene, rays, "zeros of either sign")
    check_scene(ctx, pkg, ora, scene, "zeros of either sign", pkg.world.camera((0.0, 0.0, 0.0), (0.0, 0.0, 0.0), 90))


# ---- 4. ties

def test_the_first_of_two_coincident_spheres_wins(ctx, pkg, ora):
    """Fully coincident: the second shares everything there is to share and is the same candidate at the same t; the fold keeps the first"""
    W = pkg.world
    spheres = np.array([W.sphere((0.5, 0.25, -9.0), 1.0, (0.3, 0.3, 0.3), 0.0, W.MATTE, 0.8),
                        W.sphere((0.5, 0.25, -10.0), 2.0, (1.0, 0.2, 0.2), 5.0, W.MATTE, 0.8),
                        W.sphere((0.5, 0.25, -10.0), 2.0, (0.2, 0.2, 1.0), 9.0, W.GLOSSY, 0.9)], dtype=W.SPHERE_DTYPE)
    scene = (spheres, W.main_scene()[1])
    rays = np.array([(0.5, 1.5, 0.0, 0.0, 0.0, -1.0), (2.0, 0.25, 0.0, 0.0, 0.0, -1.0)], np.float32)     # past the small sphere in front
    for r in rays:
        t0, t1, t2 = (ora.distance_to_sphere(r[:3], r[3:], s) for s in spheres)
        assert t0 is None and t1 is not None and t1 == t2
    ctx.set_scene(*scene)
    t, idx, just = ctx.eval_check_hit(rays)
    assert list(just) == [1, 1] and list(idx) == [1, 1]
    check_scene(ctx, pkg, ora, scene, "coincident spheres", W.camera((0.0, 0.0, 0.0), (0.0, 0.0, 0.0), 90))


# ---- 5. non-finite input

def test_a_run_with_a_nan_cx_shares_and_takes_the_literal_fold(ctx, pkg, ora):
    """Three spheres with ONE NaN pattern in cx and equal cy: the same bits, so the second and third share -- NaN terms, as they would
    compute -- every ray gets a NaN key, and the wave must fall back to the literal fold and agree with the oracle on every plane
    (colour planes: NaN == NaN by position)."""
    spheres, planes = pkg.world.main_scene()
    spheres = spheres.copy()
    for i in (1, 2, 3):
        spheres["position"][i] = (np.nan, 1.0, -9.0 - i)
    assert len({c.tobytes() for c in spheres["position"][1:4, :2]}) == 1
    cam = pkg.world.initial_camera()
    start = initial_planes(ora, W_, H_)
    got = render_gpu(ctx, pkg, (spheres, planes), cam, W_, H_, LIMIT, SPP, start, pkg.INLINE)
    with np.errstate(all="ignore"):
        want, _ = ora.render_inline(spheres, planes, cam, W_, H_, LIMIT, SPP, start)
    for a, b in zip(got[:3], want[:3]):
        assert np.array_equal(np.isnan(a), np.isnan(b))
        assert np.array_equal(a[~np.isnan(a)].view(np.uint32), b[~np.isnan(b)].view(np.uint32))
    for a, b in zip(got[3:], want[3:]):
        assert np.array_equal(a, b)


# ---- 6. a run whose candidates are stashed and folded in several passes

@pytest.mark.parametrize("order", ["nearest_first", "nearest_last", "shuffled"])
@pytest.mark.parametrize("k", [2, 3, 5, 9])
def test_a_skewered_run_takes_several_passes(ctx, pkg, ora, k, order):
    """k spheres on the z axis: ONE run (every sphere after the first shares), and a ray down the axis is a candidate of each in front
    of it, so its lane's stash is taken at every shared sphere and a pass runs there: the case the sharing makes common."""
    scene = skewer(pkg, k, order)
    xy = scene[0]["position"][:, :2].copy().view(np.uint32)
    assert all(np.array_equal(xy[i], xy[0]) for i in range(k))
    rays = skewer_rays(k)
    assert max(sum(ora.distance_to_sphere(r[:3], r[3:], s) is not None for s in scene[0]) for r in rays) >= min(k, 3)
    check_rays(ctx, ora, scene, rays, "skewered run of %d, %s" % (k, order))
    got = render_forms(ctx, pkg, ora, scene, pkg.world.camera((0.0, 0.0, 0.0), (0.0, 0.0, 0.0), 90), W_, H_, SPP, "skewered run of %d, %s" % (k, order))
    assert np.any(got[0] != 0.0)


# ---- 7. a scene the kernel reads from global memory, with more spheres than the mask has bits

def test_runs_in_a_scene_past_the_lds_limit(ctx, pkg, ora):
    """200 small spheres in runs of three along z (and a run across index 63 | 64, where the mask ends: sphere 64 runs the whole test
    although its predecessor has its cx and cy): the plain walk on scalar loads, in render Inline and in the point queries."""
    centres = [(-9.0 + 1.0 * ((j // 3) % 19), -2.0 + 0.9 * ((j // 3) // 19), -9.0 - 0.8 * (j % 3)) for j in range(200)]
    radii = [0.3 + 0.05 * (j % 3) for j in range(200)]
    assert centres[63][:2] == centres[64][:2] and centres[62][:2] != centres[63][:2]
    scene = (spheres_of(pkg, centres, radii), pkg.world.main_scene()[1])
    assert 16 * len(scene[0]) > 3 * 1024
    cam = pkg.world.initial_camera()
    got = render_forms(ctx, pkg, ora, scene, cam, W_, H_, 1, "200 spheres in runs")
    assert np.any(got[0] != 0.0)
    check_rays(ctx, ora, scene, query_rays(ora, cam, (scene[0][60:68], scene[1])), "200 spheres in runs")


# ---- 8. the mask is the scene's: no context keeps a stale one

def test_a_context_goes_from_runs_to_none_and_back(ctx, pkg, ora):
    """set_scene with runs, then without, then with again on ONE context: each render is the render of a fresh context (and the
    oracle's).  The scene without runs has the first one's count and z, so a mask left behind would share where nothing repeats."""
    cam = pkg.world.initial_camera()
    with_runs = row_scene(pkg, 7, 1, 4)
    without = row_scene(pkg, 7, 0, 1)
    other_runs = row_scene(pkg, 7, 3, 4, run_xy=(-1.0, 0.5))
    start = initial_planes(ora, W_, H_)
    for n, scene in enumerate((with_runs, without, other_runs, with_runs)):
        with pkg.Context(0) as fresh:
            for how, algorithm in FORMS:
                got = check_render(ctx, pkg, ora, scene, cam, W_, H_, SPP, how, "scene %d of the sequence" % n, LIMIT)
                want = render_gpu(fresh, pkg, scene, cam, W_, H_, LIMIT, SPP, start, getattr(pkg, algorithm))
                assert_planes_equal(got, want, "scene %d of the sequence against a fresh context, %s" % (n, how))
        check_rays(ctx, ora, scene, query_rays(ora, cam, scene), "scene %d of the sequence" % n)


# ---- 9. lanes that hold no pixel

@pytest.mark.parametrize("w,h", [(5, 48), (64, 44), (20, 12)])
def test_s16_with_lanes_that_hold_no_pixel(ctx, pkg, ora, w, h):
    """An image narrower than a tile, one with a ragged last tile row, one with part-filled tiles both ways"""
    render_forms(ctx, pkg, ora, pkg.world.scene16(), pkg.world.initial_camera(), w, h, SPP, "S16 at %d x %d" % (w, h))
