"""The candidates of check_hit's sphere test as a wave mask from two compares (csrc/ptmi_device.h, fold_sphere): !(tca < 0) and
!(d2 > r^2), joined by a scalar and, with x = r^2 - d2 formed only where a lane is a candidate -- instead of x for every lane and one
compare of min(tca, x).  d2 > r^2 and r^2 - d2 < 0 are the same predicate, so every hit stays what it was: the cases below sit on that
predicate's edges and compare with the oracle bit for bit -- (Just, index, t) of hand-made rays through ctx.eval_check_hit against the
oracle's fold, 64 rays a wave with the edge lanes among ordinary ones, and all seven planes of 8 x 8 renders whose explicit `screen`
sends half the pixels down the -z axis.  The finite cases run through a BVH scene too (its walk keeps PTMI_SPHERE_TEST whole and must
give the linear fold's hits); a hierarchy refuses spheres that are not finite."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from conftest import assert_planes_equal, initial_planes  # noqa: E402
from test_gpu_sphere_pass import colour_of, fold, skewer, skewer_rays  # noqa: E402

pytestmark = pytest.mark.gpu
F = np.float32
ONE_DN, ONE_UP = np.nextafter(F(1), F(0)), np.nextafter(F(1), F(2))


def spheres_of(pkg, centres, radii):
    W = pkg.world
    return np.array([W.sphere(tuple(c), radii[i], colour_of(i), 4.0 if i % 2 == 0 else 0.0, W.GLOSSY if i % 2 else W.MATTE, 0.8)
                     for i, c in enumerate(centres)], dtype=W.SPHERE_DTYPE)


def terms(ray, sphere):
    """tca, d2 and r^2 in binary32, operation for operation as PTMI_SPHERE_TEST forms them (dot = (x x + y y) + z z)"""
    with np.errstate(all="ignore"):
        o, d = ray[:3].astype(F), ray[3:].astype(F)
        l = sphere["position"].astype(F) - o
        tca = F(F(F(l[0] * d[0]) + F(l[1] * d[1])) + F(l[2] * d[2]))
        ll = F(F(F(l[0] * l[0]) + F(l[1] * l[1])) + F(l[2] * l[2]))
        return tca, F(ll - F(tca * tca)), F(sphere["radius"] * sphere["radius"])


def ordinary_rays(n, seed):
    """rays from near the origin into the half space the scenes stand in"""
    r = np.random.default_rng(seed)
    d = np.stack([r.uniform(-0.5, 0.5, n), r.uniform(-0.3, 0.3, n), -np.ones(n)], axis=1)
    d /= np.linalg.norm(d, axis=1)[:, None]
    o = np.stack([r.uniform(-0.2, 0.2, n), r.uniform(-0.2, 0.2, n), np.zeros(n)], axis=1)
    return np.concatenate([o, d], axis=1).astype(F)


def in_waves(special, seed):
    """every special ray in lane 0, lane 63 and a middle lane of a wave of 64 whose other lanes hold ordinary rays, then all of them together"""
    waves = []
    for k, ray in enumerate(special):
        w = ordinary_rays(64, seed + k)
        w[(0, 63, 29)[k % 3]] = ray
        waves.append(w)
    w = ordinary_rays(64, seed + 1000)
    w[:min(len(special), 64)] = special[:64]
    waves.append(w)
    return np.concatenate(waves)


def check(ctx, ora, scene, rays, what, bvh=False):
    """ctx.eval_check_hit against the oracle's fold, ray by ray: Just, index and the bits of t"""
    (ctx.set_scene_bvh if bvh else ctx.set_scene)(*scene)
    rays = np.ascontiguousarray(rays, F)
    t, idx, just = ctx.eval_check_hit(rays)
    for n, r in enumerate(rays):
        w_just, w_t, w_idx = fold(ora, scene, r[:3], r[3:])
        assert bool(just[n]) == w_just, (what, n)
        if w_just:
            assert idx[n] == w_idx and F(t[n]).view(np.uint32) == F(w_t).view(np.uint32), (what, n, idx[n], w_idx, t[n], w_t)


def grazing_scene(pkg):
    """unit spheres whose centres stand 1 and its two neighbours off the -z axis, at z = -5 (tca = 5: cx^2 is absorbed, d2 = 1 = r^2 for
    all three) and at z = -0.5 (tca = 0.5: d2 is r^2 and a step either side); a small one behind them all that every axis ray does hit"""
    centres = [(cx, 0.0, z) for z in (-5.0, -0.5) for cx in (F(1), ONE_DN, ONE_UP)] + [(0.0, 0.0, -9.0)]
    return spheres_of(pkg, centres, [1.0] * 6 + [0.5]), np.array([], dtype=pkg.world.PLANE_DTYPE)


AXIS = (0.0, 0.0, 0.0, 0.0, 0.0, -1.0)


@pytest.mark.parametrize("bvh", [False, True], ids=["linear", "bvh"])
def test_d2_equal_to_r2_and_one_step_either_side(ctx, pkg, ora, bvh):
    scene = grazing_scene(pkg)
    axis = np.array(AXIS, F)
    rel = []
    for s in scene[0][:6]:
        tca, d2, r2 = terms(axis, s)
        rel.append("=" if d2 == r2 else ("<" if d2 < r2 else ">"))
        assert tca > 0
    assert rel[:3] == ["=", "=", "="] and sorted(rel[3:]) == ["<", "=", ">"], rel      # the construction does sit on the edge
    # each sphere alone in the scene, then all together
    special = [axis] + [np.array((0.0, 0.0, 0.0, 0.0, 0.0, 1.0), F)]
    for k in range(6):
        one = (scene[0][k:k + 1], scene[1])
        check(ctx, ora, one, in_waves([axis], 300 + k), "d2 %s r2, sphere %d alone" % (rel[k], k), bvh)
    hits = [ora.distance_to_sphere(axis[:3], axis[3:], s) is not None for s in scene[0][:6]]
    assert hits == [r != ">" for r in rel]                  # d2 == r2 is a hit (x = 0), one step beyond is none
    check(ctx, ora, scene, in_waves(special, 310), "grazing spheres together", bvh)


@pytest.mark.parametrize("bvh", [False, True], ids=["linear", "bvh"])
def test_tca_of_either_zero_with_the_origin_inside(ctx, pkg, ora, bvh):
    """The origin inside a sphere whose centre lies beside it at right angles to the ray: tca = +0, and -0 when every product is a -0;
    neither is < 0, so the lane is a candidate of that sphere (whose t is then negative: Nothing) and goes on to the one behind."""
    scene = (spheres_of(pkg, [(0.3, 0.0, 0.0), (0.0, 0.0, -6.0)], [1.0, 1.0]), np.array([], dtype=pkg.world.PLANE_DTYPE))
    plus = np.array((0.0, 0.0, 0.0, 0.0, 0.0, -1.0), F)
    minus = np.array((0.0, 0.0, 0.0, -0.0, -0.0, -1.0), F)
    tiny_back = np.array((0.0, 0.0, 0.0, -1e-30, 0.0, -1.0), F)                   # tca tiny and negative: no candidate
    t_plus, t_minus, t_back = (terms(r, scene[0][0])[0] for r in (plus, minus, tiny_back))
    assert t_plus == 0 and not np.signbit(t_plus) and t_minus == 0 and np.signbit(t_minus) and t_back < 0
    check(ctx, ora, scene, in_waves([plus, minus, tiny_back], 320), "tca of either zero", bvh)


def test_spheres_that_are_not_finite(ctx, pkg, ora):
    """r^2 = inf (x = inf: a candidate whose t is -inf), a centre at inf (d2 and x are NaN: both compares answer false, a candidate) and a
    NaN centre; rays that hit the finite sphere in front, behind and beside them, in waves with ordinary rays."""
    W = pkg.world
    none = np.array([], dtype=W.PLANE_DTYPE)
    finite = [(0.0, 0.0, -6.0), (1.5, 0.5, -4.0)]
    rays = [np.array(AXIS, F), np.array((1.5, 0.5, 0.0, 0.0, 0.0, -1.0), F), np.array((0.0, 0.0, -12.0, 0.0, 0.0, 1.0), F)]
    for what, centre, radius in (("r2 = inf", (0.0, 0.0, -20.0), np.inf), ("r2 overflows", (0.0, 0.0, -20.0), 1e30),
                                 ("a centre at inf", (np.inf, 0.0, -8.0), 1.0), ("a centre at -inf in z", (0.0, 0.0, -np.inf), 1.0),
                                 ("a NaN centre", (np.nan, 0.0, -8.0), 1.0)):
        for place in (0, 2):
            centres, radii = list(finite), [1.0, 0.7]
            centres.insert(place, centre)
            radii.insert(place, radius)
            with np.errstate(all="ignore"):
                scene = (spheres_of(pkg, centres, radii), none)
                check(ctx, ora, scene, in_waves(rays, 330), "%s at index %d" % (what, place))


@pytest.mark.parametrize("bvh", [False, True], ids=["linear", "bvh"])
def test_two_candidates_in_one_lane_run_a_pass_on_a_taken_stash(ctx, pkg, ora, bvh):
    """Skewered spheres (tests/test_gpu_sphere_pass.py): an axis ray is a candidate of each in front of it, so the second candidate meets
    a taken stash; with a grazing sphere (d2 = r2) between them and lanes of ordinary rays around."""
    spheres, planes = skewer(pkg, 3, "nearest_last")
    graze = spheres_of(pkg, [(1.0, 0.0, -5.0)], [1.0])
    scene = (np.concatenate([spheres[:1], graze, spheres[1:]]), planes)
    rays = skewer_rays(3)
    assert max(sum(ora.distance_to_sphere(r[:3], r[3:], s) is not None for s in scene[0]) for r in rays) >= 3
    check(ctx, ora, scene, rays, "skewer with a grazing sphere", bvh)
    check(ctx, ora, scene, in_waves(list(rays[::8]), 340), "skewer rays among ordinary ones", bvh)


def axis_screen(w, h):
    """an explicit screen: the pixels of even columns shoot through the image's centre (the exact -z axis of a camera without rotation),
    the others through their own places"""
    xs, ys = np.meshgrid(np.arange(w, dtype=np.int64), np.arange(h, dtype=np.int64))
    xs, ys = xs.copy(), ys.copy()
    xs[:, ::2], ys[:, ::2] = w // 2, h // 2
    return np.ascontiguousarray(xs), np.ascontiguousarray(ys)


@pytest.mark.parametrize("bvh", [False, True], ids=["linear", "bvh"])
def test_renders_with_axis_rays_equal_the_oracle(ctx, pkg, ora, bvh):
    """8 x 8, limit 4, one application of render Inline with an explicit screen: half of each wave's lanes trace the axis ray -- which
    grazes three spheres at d2 = r2 and hits the small one behind --, the rest their own pixels; all seven planes against the oracle."""
    W = pkg.world
    w, h, limit = 8, 8, 4
    cam = W.camera((0.0, 0.0, 0.0), (0.0, 0.0, 0.0), 90)
    screen = axis_screen(w, h)
    o, d = ora.primary_ray(cam, w, h, w // 2, h // 2)
    assert np.array_equal(o, np.zeros(3, F)) and np.array_equal(d, np.array((0.0, 0.0, -1.0), F))
    spheres, _ = grazing_scene(pkg)
    scene = (spheres, W.main_scene()[1])
    start = initial_planes(ora, w, h)
    (ctx.set_scene_bvh if bvh else ctx.set_scene)(*scene)
    got = ctx.render1(cam, limit, w, h, start, pkg.INLINE, screen=screen)
    want, _ = ora.render_inline(scene[0], scene[1], cam, w, h, limit, 1, start, screen=screen)
    assert np.any(np.asarray(want[0]) != 0.0)
    assert_planes_equal(got, want, "axis rays, %s" % ("bvh" if bvh else "linear"))


def test_render_with_a_centre_at_inf_equals_the_oracle(ctx, pkg, ora):
    """... and with a sphere whose centre is at inf: every lane's x is a NaN there, the wave ends in the literal fold (colour planes:
    NaN == NaN by position)."""
    W = pkg.world
    w, h, limit = 8, 8, 4
    cam = W.camera((0.0, 0.0, 0.0), (0.0, 0.0, 0.0), 90)
    screen = axis_screen(w, h)
    spheres, _ = grazing_scene(pkg)
    spheres = spheres.copy()
    spheres["position"][2] = (np.inf, 0.0, -5.0)
    start = initial_planes(ora, w, h)
    ctx.set_scene(spheres, W.main_scene()[1])
    got = ctx.render1(cam, limit, w, h, start, pkg.INLINE, screen=screen)
    with np.errstate(all="ignore"):
        want, _ = ora.render_inline(spheres, W.main_scene()[1], cam, w, h, limit, 1, start, screen=screen)
    for a, b in zip(got[:3], want[:3]):
        a, b = np.asarray(a), np.asarray(b)
        assert np.array_equal(np.isnan(a), np.isnan(b))
        assert np.array_equal(a[~np.isnan(a)].view(np.uint32), b[~np.isnan(b)].view(np.uint32))
    for a, b in zip(got[3:], want[3:]):
        assert np.array_equal(np.asarray(a), np.asarray(b))
