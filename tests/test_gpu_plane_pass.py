"""The plane fold of check_hit (fold_planes, csrc/ptmi_device.h): the cheap part of every plane test stashes the lane's candidate,
the division runs in dense passes in which every lane works on its own plane.  An exact transformation, so every case here compares
all seven planes bit for bit with the oracle -- scenes with no, one, two, six, 33, 70 and 100 planes (several passes per trace; a
scene beyond the LDS limit, read from global memory by per-lane addresses), through render Inline and render Streams in both forms
-- and the ties, which the oracle decides for the earlier primitive (asserted here on the CPU before the device is asked)."""
import numpy as np
import pytest

from conftest import assert_planes_equal, initial_planes

pytestmark = pytest.mark.gpu
CAP = 1 << 16      # kStreamsHardCap; the reference has no cap (Trace.hs:166-170)


def render_gpu(ctx, pkg, scene, cam, w, h, limit, spp, start, algorithm, stream_form=False):
    B = pkg.binding
    ctx.set_scene(*scene)
    ctx.resize(w, h)
    ctx.upload_state(*start)
    ctx.set_option(B.OPT_STREAMS_FORM, B.FORM_STREAM if stream_form else B.FORM_AUTO)
    try:
        ctx.render(cam, limit, spp, algorithm)
        return ctx.download_state()
    finally:
        ctx.set_option(B.OPT_STREAMS_FORM, B.FORM_AUTO)


def check_inline(ctx, pkg, ora, scene, cam, w, h, limit, spp, what):
    start = initial_planes(ora, w, h)
    got = render_gpu(ctx, pkg, scene, cam, w, h, limit, spp, start, pkg.INLINE)
    with np.errstate(all="ignore"):
        want, _ = ora.render_inline(scene[0], scene[1], cam, w, h, limit, spp, start)
    assert_planes_equal(got, want, what)
    return got


def parallel_planes(pkg, n):
    """n planes facing the camera of initial_camera() from behind the spheres, at distinct depths, the NEAREST LAST (so the fold
    replaces its accumulator at every plane), alternately facing towards and away from the camera (away: never a candidate of a
    primary ray, a candidate of rays coming back), alternating materials, every seventh and the nearest glowing; in front of them a few spheres, one a light."""
    W = pkg.world
    spheres = W.scene16()[0][[1, 2, 3, 5, 9]]
    planes = []
    for k in range(n):
        towards = k % 3 != 1
        planes.append(W.plane((0.0, 0.0, -30.0 - 0.25 * (n - k)), (0.0, 0.0, 1.0 if towards else -1.0),
                              (0.3 + 0.6 * ((k * 7) % 10) / 10.0, 0.5, 0.9 - 0.5 * ((k * 3) % 10) / 10.0),
                              3.0 if k % 7 == 0 or k == n - 1 else 0.0, W.GLOSSY if k % 2 else W.MATTE, 0.8))
    planes += [W.plane((0.0, -3.0, 0.0), (0.0, 1.0, 0.0), (0.43, 0.95, 0.5), 0.0, W.MATTE, 1.5)] if n else []
    return spheres, np.array(planes, dtype=W.PLANE_DTYPE)


@pytest.mark.parametrize("algorithm,stream_form", [("inline", False), ("streams", False), ("streams", True)])
def test_mirror_box_takes_several_passes_per_trace(ctx, pkg, ora, algorithm, stream_form):
    """Six planes, about three candidates per ray: a pass at the third and fifth plane and one at the end."""
    scene = pkg.world.mirror_box()
    cam = pkg.world.initial_camera()
    w, h, limit, spp = 32, 16, 8, 3
    start = initial_planes(ora, w, h)
    if algorithm == "inline":
        got = render_gpu(ctx, pkg, scene, cam, w, h, limit, spp, start, pkg.INLINE)
        want, _ = ora.render_inline(scene[0], scene[1], cam, w, h, limit, spp, start)
    else:
        got = render_gpu(ctx, pkg, scene, cam, w, h, limit, spp, start, pkg.STREAMS, stream_form)
        want, _ = ora.render_streams(scene[0], scene[1], cam, w, h, CAP, spp, start)
    assert_planes_equal(got, want, "mirror box, %s%s" % (algorithm, ", stream form" if stream_form else ""))


@pytest.mark.parametrize("algorithm", ["inline", "streams"])
def test_floor_and_ceiling_share_one_pass(ctx, pkg, ora, algorithm):
    """S16: the two planes' candidates are complementary sets of rays.  64 x 40 has a ragged tile row: some lanes hold no pixel."""
    scene = pkg.world.scene16()
    cam = pkg.world.initial_camera()
    w, h, limit, spp = 64, 40, 8, 4
    start = initial_planes(ora, w, h)
    if algorithm == "inline":
        got = render_gpu(ctx, pkg, scene, cam, w, h, limit, spp, start, pkg.INLINE)
        want, _ = ora.render_inline(scene[0], scene[1], cam, w, h, limit, spp, start)
    else:
        got = render_gpu(ctx, pkg, scene, cam, w, h, limit, spp, start, pkg.STREAMS)
        want, _ = ora.render_streams(scene[0], scene[1], cam, w, h, CAP, spp, start)
    assert_planes_equal(got, want, "S16, %s" % algorithm)


@pytest.mark.parametrize("n_planes", [0, 1, 33, 70])
def test_plane_counts(ctx, pkg, ora, n_planes):
    """No plane, one, and more than 32 (33 still staged in LDS, 70 not)."""
    if n_planes <= 1:
        spheres, planes = pkg.world.scene16()
        scene = (spheres, planes[:n_planes])
    else:
        scene = parallel_planes(pkg, n_planes - 1)
        assert len(scene[1]) == n_planes
    got = check_inline(ctx, pkg, ora, scene, pkg.world.initial_camera(), 16, 16, 8, 2, "%d planes" % n_planes)
    assert np.any(got[0] != 0.0)


def test_scene_beyond_the_lds_limit_reads_planes_by_lane(ctx, pkg, ora):
    """100 planes: 200 records of geometry alone are more than the 3 KB a workgroup stages, so the kernels read the scene from
    global memory and a pass reads each lane's plane by the lane's own address.  Inline and the Streams chain."""
    scene = parallel_planes(pkg, 99)
    assert 2 * 16 * len(scene[1]) > 3 * 1024
    cam = pkg.world.initial_camera()
    w, h = 16, 16
    check_inline(ctx, pkg, ora, scene, cam, w, h, 8, 1, "100 planes, Inline")
    start = initial_planes(ora, w, h)
    got = render_gpu(ctx, pkg, scene, cam, w, h, 8, 1, start, pkg.STREAMS)
    want, _ = ora.render_streams(scene[0], scene[1], cam, w, h, CAP, 1, start)
    assert_planes_equal(got, want, "100 planes, Streams")


def test_the_first_of_two_coincident_planes_wins(ctx, pkg, ora):
    W = pkg.world
    spheres, planes = W.scene16()
    floor_again = np.array([W.plane((0.0, -3.0, 0.0), (0.0, 1.0, 0.0), (0.1, 0.1, 0.9), 7.0, W.GLOSSY, 0.9)], dtype=W.PLANE_DTYPE)
    scene = (spheres, np.concatenate([planes[:1], floor_again, planes[1:]]))
    cam = W.initial_camera()
    w, h = 16, 16
    o, d = ora.primary_ray(cam, w, h, 8, 3)                      # a pixel that sees the floor
    hit = ora.check_hit(scene[0], scene[1], o, d)
    assert hit is not None and np.array_equal(hit[2][0], planes[0]["color"]) and hit[2][1] == 0.0    # the reference: the earlier one
    ctx.set_scene(*scene)
    t, idx, just = ctx.eval_check_hit(np.concatenate([o, d])[None, :])
    assert just[0] == 1 and idx[0] == len(spheres)
    check_inline(ctx, pkg, ora, scene, cam, w, h, 8, 2, "coincident planes")


def test_a_sphere_wins_the_tie_with_a_plane(ctx, pkg, ora):
    """The primary ray of pixel (4, 4) of an 8 x 8 image is (0, 0, -1) exactly; it meets the sphere (centre z = -10, radius 2) and
    the plane z = -8, tangent to it, at t = 8 in both tests."""
    W = pkg.world
    cam = W.camera((0.0, 0.0, 0.0), (0.0, 0.0, 0.0), 90)
    spheres = np.array([W.sphere((0.0, 0.0, -10.0), 2.0, (1.0, 0.2, 0.2), 5.0, W.MATTE, 0.8)], dtype=W.SPHERE_DTYPE)
    planes = np.array([W.plane((0.0, 0.0, -8.0), (0.0, 0.0, 1.0), (0.2, 0.2, 1.0), 9.0, W.MATTE, 0.9),
                       W.plane((0.0, -3.0, 0.0), (0.0, 1.0, 0.0), (0.43, 0.95, 0.5), 0.0, W.MATTE, 1.5)], dtype=W.PLANE_DTYPE)
    w, h = 8, 8
    o, d = ora.primary_ray(cam, w, h, 4, 4)
    assert np.array_equal(d, np.array([0.0, 0.0, -1.0], np.float32))
    ts, tp = ora.distance_to_sphere(o, d, spheres[0]), ora.distance_to_plane(o, d, planes[0])
    assert ts is not None and tp is not None and ts == tp == np.float32(8.0)
    hit = ora.check_hit(spheres, planes, o, d)
    assert np.array_equal(hit[2][0], spheres[0]["color"])                     # the reference: the sphere, being earlier
    ctx.set_scene(spheres, planes)
    t, idx, just = ctx.eval_check_hit(np.concatenate([o, d])[None, :])
    assert just[0] == 1 and idx[0] == 0 and t[0] == np.float32(8.0)
    check_inline(ctx, pkg, ora, (spheres, planes), cam, w, h, 8, 2, "sphere and tangent plane")


def test_a_nan_plane_normal_takes_the_literal_fold(ctx, pkg, ora):
    """A NaN normal makes its plane a candidate of every ray with a NaN key: the fold must fall back to the literal one and agree
    with the oracle on every plane (colour planes: NaN == NaN by position)."""
    spheres, planes = pkg.world.main_scene()
    planes = planes.copy()
    planes["direction"][1] = (0.0, np.nan, 0.0)
    cam = pkg.world.initial_camera()
    w, h = 8, 8
    start = initial_planes(ora, w, h)
    got = render_gpu(ctx, pkg, (spheres, planes), cam, w, h, 4, 1, start, pkg.INLINE)
    with np.errstate(all="ignore"):
        want, _ = ora.render_inline(spheres, planes, cam, w, h, 4, 1, start)
    for a, b in zip(got[:3], want[:3]):
        assert np.array_equal(np.isnan(a), np.isnan(b))
        assert np.array_equal(a[~np.isnan(a)].view(np.uint32), b[~np.isnan(b)].view(np.uint32))
    for a, b in zip(got[3:], want[3:]):
        assert np.array_equal(a, b)
