"""Angles below 2^-12 inside the render kernels' fast sin/cos (quaternion_from_half_angles, csrc/ptmi_core.h): one vote per wave now has
three outcomes -- an angle at or beyond +-T2, inf or NaN in any active lane sends the wave to three sincos(); otherwise every lane runs
the quadrant form, and behind a second wave-uniform branch the lanes whose angle is below 2^-12 in magnitude take (y, 1), per angle.
ptmi_eval_quaternion runs the kernels' inline function with 64 consecutive inputs per wave; the expected quaternions are built from
ptmi_eval_sincos of each angle, as tests/test_gpu_sincos_quadrant.py builds them.  Compared bit for bit.  And one render whose Glossy
spheres draw tiny angles only (p = 1: every angle 0; p = 0.9998: hk = 1e-4, every angle below 2^-12) beside a Matte one, Inline and
Streams, all seven planes against the oracle."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from conftest import assert_planes_equal, initial_planes  # noqa: E402
from test_gpu_sincos_quadrant import TINY, assert_quaternions_equal, bits, expected_quaternions, fast_group, fast_values  # noqa: E402

pytestmark = pytest.mark.gpu
F = np.float32


def tiny_values():
    """+0, -0, a denormal, 2^-13, the pattern below 2^-12 (all tiny), with both signs; and 2^-12 itself, which is not."""
    v = [0x00000000, 0x80000000, TINY - 1, (TINY - 1) | 0x80000000, TINY, TINY | 0x80000000]
    v += list(np.array([1e-40, -1e-40, 2.0 ** -13, -(2.0 ** -13)], dtype=F).view(np.uint32))
    return bits(*[int(x) for x in v])


def test_one_tiny_angle_among_fast_lanes(ctx):
    """Exactly one lane holds one tiny angle -- lane 0 (first angle), lane 63 (second), a middle lane (third), and every other pairing of
    lane and angle position -- among 63 lanes of fast-range angles, quadrant steps among them: the wave stays in the fast form, the tiny
    lane's angle alone takes (y, 1), its other two angles and every other lane the quadrant form."""
    r = np.random.default_rng(21)
    steps = fast_values()
    groups = []
    for value in tiny_values():
        for lane in (0, 63, 17):
            for angle in (0, 1, 2):
                g = fast_group(r)
                others = np.array([i for i in range(64) if i != lane])
                pick = r.permutation(others)[:8]
                g[pick, r.integers(0, 3, 8)] = r.choice(steps, 8)
                g[lane, angle] = value
                groups.append(g)
    a = np.concatenate(groups)
    assert_quaternions_equal(ctx.eval_quaternion(a), expected_quaternions(ctx, a), "one tiny angle per wave")


def test_waves_of_tiny_angles(ctx):
    """Every angle of every lane zero (the Glossy p = 1 sphere's shade); every angle of every lane one of the tiny values; and a wave in
    which tiny and fast-range angles alternate by lane and by position."""
    r = np.random.default_rng(22)
    tv = tiny_values()
    lane = np.arange(64)
    zeros = np.zeros((64, 3), dtype=F)
    all_tiny = np.stack([tv[lane % tv.size], tv[(lane + 3) % tv.size], tv[(lane + 5) % tv.size]], axis=1)
    mixed = fast_group(r)
    mixed[lane % 2 == 0, 0] = tv[(lane[lane % 2 == 0] // 2) % tv.size]
    mixed[lane % 3 == 1, 1] = F(0.0)
    mixed[lane % 5 == 2, 2] = tv[(lane[lane % 5 == 2]) % tv.size]
    a = np.concatenate([zeros, all_tiny, mixed])
    assert_quaternions_equal(ctx.eval_quaternion(a), expected_quaternions(ctx, a), "waves of tiny angles")


@pytest.mark.parametrize("slow", [2.4, -2.4, 1e30, float("inf"), float("nan")])
def test_a_tiny_lane_beside_a_lane_that_leaves_the_fast_form(ctx, slow):
    """A tiny angle in one lane and an angle beyond +-T2, inf or NaN in another: the whole wave takes sincos(), whose own last line serves
    the tiny lane."""
    r = np.random.default_rng(23)
    groups = []
    for value in tiny_values():
        g = fast_group(r)
        g[5, 1] = value
        g[40, 2] = F(slow)
        groups.append(g)
        g = fast_group(r)
        g[63, 0] = value
        g[63, 2] = F(slow)                                # ... and in the same lane
        groups.append(g)
    a = np.concatenate(groups)
    assert_quaternions_equal(ctx.eval_quaternion(a), expected_quaternions(ctx, a), "tiny lane beside %r" % slow)


@pytest.mark.parametrize("last", [0.0, -0.0, 1e-40, 2.0 ** -13])
def test_last_partial_wave_with_a_tiny_lane(ctx, last):
    """n = 64 k + 1: the last wave holds one active lane, tiny, and votes alone."""
    r = np.random.default_rng(24)
    a = np.concatenate([fast_group(r, 128), fast_group(r, 1)])
    a[-1, 1] = F(last)
    assert a.shape[0] == 129
    assert_quaternions_equal(ctx.eval_quaternion(a), expected_quaternions(ctx, a), "partial wave, last lane %r" % last)


@pytest.mark.parametrize("algorithm", ["inline", "streams"])
def test_render_with_tiny_angles_equals_the_oracle(ctx, pkg, ora, algorithm):
    """A Matte sphere, a Glossy p = 1 sphere (hk = 0: three zero angles at every hit) and a Glossy p = 0.9998 sphere (hk = 1e-4: every angle
    below 2^-12): waves whose lanes shade all three hold tiny and ordinary angles side by side inside a real kernel.  16 x 16, 4 spp,
    limit 4; all seven planes bit for bit against the oracle."""
    W = pkg.world
    spheres = np.array([W.sphere((-2.4, 0.0, -4.5), 1.1, (0.9, 0.5, 0.3), 3.0, W.MATTE, 0.8),
                        W.sphere((0.0, 0.0, -4.5), 1.1, (0.4, 0.6, 0.9), 1.0, W.GLOSSY, 1.0),
                        W.sphere((2.4, 0.0, -4.5), 1.1, (0.5, 0.9, 0.4), 1.0, W.GLOSSY, 0.9998)], dtype=W.SPHERE_DTYPE)
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
    assert_planes_equal(got, want, "tiny angles, %s" % algorithm)
