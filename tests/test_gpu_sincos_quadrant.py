"""The three-angle sin/cos of the render kernels on the device (quaternion_from_half_angles, csrc/ptmi_core.h): one vote per wave sends
the wave to the quadrant-by-comparison form (every angle of every active lane strictly inside (T2n, T2p), none below 2^-12 in
magnitude) or to three evaluations of sincos().  ptmi_eval_quaternion runs the kernels' inline function with 64 consecutive inputs per
wave; the expected quaternions are built from ptmi_eval_sincos of each angle -- that kernel evaluates sincos() alone and is pinned to
the oracle and libm by tests/test_gpu_intersection.py -- combined on the host in binary32 with the function's product order.  Compared
bit for bit; a component whose expected value is a NaN (an inf or NaN angle) must be a NaN.  And one render: a Glossy sphere with
p = -4 (hk = 2.5, so hk * rv leaves the fast range for some lanes of a wave and not for others), Inline and Streams against the oracle."""
import numpy as np
import pytest

from conftest import assert_planes_equal, initial_planes

pytestmark = pytest.mark.gpu
F = np.float32
T1P, T1N, T2P, T2N, TINY = 0x3f490fdb, 0xbf490fdd, 0x4016cbe4, 0xc016cbe5, 0x39800000      # ptmi_core.h: kQuadT1p ...


def bits(*patterns):
    return np.array(patterns, dtype=np.uint32).view(F)


def expected_quaternions(ctx, half_angles):
    a = np.ascontiguousarray(half_angles, dtype=F).reshape(-1, 3)
    s, c = ctx.eval_sincos(a.reshape(-1))
    s, c = s.reshape(-1, 3), c.reshape(-1, 3)
    sr, sp, sy = s[:, 0], s[:, 1], s[:, 2]
    cr, cp, cy = c[:, 0], c[:, 1], c[:, 2]
    with np.errstate(all="ignore"):
        q = np.stack([cy * cp * cr + sy * sp * sr, cy * cp * sr - sy * sp * cr, sy * cp * sr + cy * sp * cr, sy * cp * cr - cy * sp * sr], axis=1)
    assert q.dtype == F
    return q


def assert_quaternions_equal(got, want, what):
    nan = np.isnan(want)
    assert np.all(np.isnan(got[nan])), what + ": a NaN component is expected and a number was returned"
    g, w = got.view(np.uint32)[~nan], want.view(np.uint32)[~nan]
    bad = np.flatnonzero(g != w)
    assert bad.size == 0, "%s: %d of %d components differ bitwise (first %#x vs %#x)" % (what, bad.size, g.size, g[bad[0]], w[bad[0]])


def fast_values():
    """Angles inside the fast range that sit on the steps of the quadrant: each T1 threshold's pattern and its two neighbours each side,
    with both signs; the last two patterns before each T2; 2^-12 and the two patterns above it, with both signs."""
    v = []
    for t in (T1P, T1N & 0x7fffffff):
        v += [t + d for d in (-2, -1, 0, 1, 2)] + [(t + d) | 0x80000000 for d in (-2, -1, 0, 1, 2)]
    v += [T2P - 1, T2P - 2, T2N - 1, T2N - 2, (T2P - 1) | 0x80000000]
    v += [TINY, TINY + 1, TINY + 2, TINY | 0x80000000, (TINY + 1) | 0x80000000, (TINY + 2) | 0x80000000]
    return bits(*v)


def slow_values():
    """Angles one of which sends its whole wave to sincos(): T2p, -T2n and their neighbours outward, the ends of reduce_fast's range and
    beyond, inf, NaN, and the |y| < 2^-12 side: zeros, 2^-12 itself (the guard's boundary) and the pattern below it, 2^-13, a denormal."""
    v = [T2P, T2P + 1, T2P + 2, T2N, T2N + 1, T2N + 2, T2P | 0x80000000]
    v += list(np.array([119.99999, 120.0, 1e30, np.inf, -np.inf, np.nan, 0.0, -0.0, 2.0 ** -12, -(2.0 ** -12), 2.0 ** -13, 1e-40], dtype=F).view(np.uint32))
    v += [TINY - 1, (TINY - 1) | 0x80000000, 0xffc00000]
    return bits(*[int(x) for x in v])


def fast_group(r, n=64):
    """n rows of angles inside the fast range, away from zero"""
    a = r.uniform(-2.35, 2.35, (n, 3)).astype(F)
    small = np.abs(a) < 2.0 ** -10
    a[small] = F(0.5)
    return a


def test_fast_waves_with_lanes_on_every_step(ctx):
    """(a) 64-lane groups entirely inside the fast range; the step values sit in every angle position and lane."""
    r = np.random.default_rng(11)
    steps = fast_values()
    groups = []
    for k in range(6):
        g = fast_group(r)
        assert steps.size <= 64
        lanes = r.permutation(64)[:steps.size]
        g[lanes, k % 3] = steps
        g[lanes, (k + 1) % 3] = np.roll(steps, k + 1)
        groups.append(g)
    lane = np.arange(64)                                 # and a wave in which every angle of every lane is a step value
    groups.append(np.stack([steps[lane % steps.size], steps[(lane + 7) % steps.size], steps[(lane + 13) % steps.size]], axis=1))
    a = np.concatenate(groups)
    assert_quaternions_equal(ctx.eval_quaternion(a), expected_quaternions(ctx, a), "fast waves")


def test_one_lane_sends_its_wave_to_the_slow_path(ctx):
    """(b), (c): groups in which exactly one lane holds one angle that the fast form does not cover -- in lane 0 (first angle), in lane 63
    (second angle) and in a middle lane's third angle only; the other 63 lanes hold fast-range angles, steps among them."""
    r = np.random.default_rng(12)
    steps = fast_values()
    groups = []
    for bad in slow_values():
        for lane, angle in ((0, 0), (63, 1), (17, 2)):
            g = fast_group(r)
            others = np.array([i for i in range(64) if i != lane])
            pick = r.permutation(others)[:8]
            g[pick, r.integers(0, 3, 8)] = r.choice(steps, 8)
            g[lane, angle] = bad
            groups.append(g)
    a = np.concatenate(groups)
    assert_quaternions_equal(ctx.eval_quaternion(a), expected_quaternions(ctx, a), "one slow lane per wave")


@pytest.mark.parametrize("last", [0.8, 1e30, 0.0, float("nan")])
def test_last_partial_wave(ctx, last):
    """(d) n = 64 k + 1: the last wave holds one active lane, and votes alone."""
    r = np.random.default_rng(13)
    a = np.concatenate([fast_group(r, 128), fast_group(r, 1)])
    a[-1, 1] = F(last)
    assert a.shape[0] == 129
    assert_quaternions_equal(ctx.eval_quaternion(a), expected_quaternions(ctx, a), "partial wave, last lane %r" % last)


@pytest.mark.parametrize("algorithm", ["inline", "streams"])
def test_render_with_mixed_waves_equals_the_oracle(ctx, pkg, ora, algorithm):
    """A Matte and a Glossy sphere; the Glossy p = -4 gives hk = (1 - p) / 2 = 2.5, so a Glossy hit's half angles hk * rv reach
    +-2.5 > T2 = 2.356...: waves whose lanes shade both spheres hold angles inside and outside the fast range -- the mixed wave inside a real
    kernel.  16 x 16, 4 spp, limit 4; all seven planes bit for bit against the oracle."""
    W = pkg.world
    spheres = np.array([W.sphere((-1.3, 0.0, -4.0), 1.2, (0.9, 0.5, 0.3), 3.0, W.MATTE, 0.8),
                        W.sphere((1.3, 0.0, -4.0), 1.2, (0.4, 0.6, 0.9), 1.0, W.GLOSSY, -4.0)], dtype=W.SPHERE_DTYPE)
    planes = np.array([], dtype=W.PLANE_DTYPE)
    cam = W.camera((0.0, 0.0, 0.0), (0.0, 0.0, 0.0), 90)
    w, h, limit, spp = 16, 16, 4, 4
    start = initial_planes(ora, w, h)
    ctx.set_scene(spheres, planes)
    ctx.resize(w, h)
    ctx.upload_state(*start)
    if algorithm == "inline":
        ctx.render(cam, limit, spp, pkg.INLINE)
        want, _ = ora.render_inline(spheres, planes, cam, w, h, limit, spp, start)
    else:
        ctx.render(cam, limit, spp, pkg.STREAMS)
        want, _ = ora.render_streams(spheres, planes, cam, w, h, 1 << 16, spp, start)
    got = ctx.download_state()
    assert np.any(np.asarray(want[0]) != 0.0)          # the spheres are in view and lit
    assert_planes_equal(got, want, "mixed waves, %s" % algorithm)
