"""The sphere candidates of check_hit (csrc/ptmi_device.h): the 16-operation test of every sphere only stashes (tca, x, index) in its
candidate lanes, the square root / t / fold update run in dense passes -- when a sphere comes up for a lane whose stash is taken, and
once behind the last sphere.  An exact transformation, so every case compares with the oracle bit for bit: all seven planes of a render
(Inline: the staged walk; the Streams chain; the stream form) and (t, index, Just) of hand-made rays through ctx.eval_check_hit (the
plain walk).  The reference of a single ray is ora.check_hit; the distance functions of the oracle, folded here as expMinWith folds
them (the earlier element stays on `<=`), give the t and the index that ora.check_hit's hit record does not name, and every ray's
fold is held against ora.check_hit's material first.

One exception to "bit for bit", not this file's choice: the stream form on a scene with GLASS adds the several rays of a pixel with
float atomics in no defined order (tests/test_gpu_wavefront.py), so there the four RNG planes and the bounce count are exact and the
colours are held to that file's 1e-4; the tree walk of the same scene is bit for bit."""
import numpy as np
import pytest

from conftest import assert_planes_equal, initial_planes

pytestmark = pytest.mark.gpu
CAP = 1 << 16      # kStreamsHardCap; the reference has no cap (Trace.hs:166-170)
KEY_NOTHING = np.float32(3.40282346638528859812e+38)     # maybe infinite fst (Trace.hs:450-451)


def render_gpu(ctx, pkg, scene, cam, w, h, limit, spp, start, algorithm, stream_form=False):
    B = pkg.binding
    ctx.set_scene(*scene)
    ctx.resize(w, h)
    ctx.upload_state(*start)
    ctx.set_option(B.OPT_STREAMS_FORM, B.FORM_STREAM if stream_form else B.FORM_AUTO)
    try:
        ctx.reset_stats()
        ctx.render(cam, limit, spp, algorithm)
        return ctx.download_state()
    finally:
        ctx.set_option(B.OPT_STREAMS_FORM, B.FORM_AUTO)


def check_render(ctx, pkg, ora, scene, cam, w, h, spp, how, what, limit=8):
    """how: "inline", "streams" (the per-pixel chain) or "stream" (the stream form); no GLASS"""
    start = initial_planes(ora, w, h)
    with np.errstate(all="ignore"):
        if how == "inline":
            got = render_gpu(ctx, pkg, scene, cam, w, h, limit, spp, start, pkg.INLINE)
            want, _ = ora.render_inline(scene[0], scene[1], cam, w, h, limit, spp, start)
        else:
            got = render_gpu(ctx, pkg, scene, cam, w, h, limit, spp, start, pkg.STREAMS, how == "stream")
            want, _ = ora.render_streams(scene[0], scene[1], cam, w, h, CAP, spp, start)
    assert_planes_equal(got, want, "%s, %s" % (what, how))
    return got


def fold(ora, scene, o, d):
    """checkHit as the left fold of expMinWith over the oracle's distances: (Just?, t, index), held against ora.check_hit's record"""
    spheres, planes = scene
    with np.errstate(all="ignore"):
        ts = [ora.distance_to_sphere(o, d, s) for s in spheres] + [ora.distance_to_plane(o, d, p) for p in planes]
        hit = ora.check_hit(spheres, planes, o, d)
    best, best_key = None, None
    for i, t in enumerate(ts):
        key = KEY_NOTHING if t is None else t
        if i == 0 or not (best_key <= key):
            best, best_key = i, key
    if best is None or ts[best] is None:
        assert hit is None
        return False, np.float32(0.0), -1
    colour = (spheres[best] if best < len(spheres) else planes[best - len(spheres)])["color"]
    assert hit is not None and np.array_equal(hit[2][0], colour)
    return True, ts[best], best


def check_rays(ctx, ora, scene, rays, what):
    """ctx.eval_check_hit against the fold, ray by ray: Just, index and the bits of t"""
    ctx.set_scene(*scene)
    rays = np.ascontiguousarray(rays, np.float32)
    t, idx, just = ctx.eval_check_hit(rays)
    for n, r in enumerate(rays):
        w_just, w_t, w_idx = fold(ora, scene, r[:3], r[3:])
        assert bool(just[n]) == w_just, (what, n)
        if w_just:
            assert idx[n] == w_idx and np.float32(t[n]).view(np.uint32) == np.float32(w_t).view(np.uint32), (what, n, idx[n], w_idx, t[n], w_t)


def colour_of(j):
    return (0.15 + 0.08 * (j % 10), 0.9 - 0.07 * (j % 11), 0.2 + 0.06 * (j % 13))      # distinct per index below 100


# ---- 1. several passes per trace, by construction

SKEWER_RADII = (0.6, 0.75, 0.9, 1.05, 1.2)
SKEWER_OFFSETS = (0.0, 0.5, 0.7, 0.85, 1.0, 1.15, 1.3, 5.0)


def skewer(pkg, k, order):
    """k spheres with centres on the z axis, 3 apart from z = -6 on, radii cycling through SKEWER_RADII, in the index order asked for
    (depth position of index i = perm[i]); S16's floor and ceiling behind them.  Every third sphere glows."""
    W = pkg.world
    perm = {"nearest_first": list(range(k)), "nearest_last": list(range(k))[::-1],
            "shuffled": list(np.random.RandomState(7 + k).permutation(k))}[order]
    if order == "shuffled" and (perm == sorted(perm) or perm == sorted(perm)[::-1]):
        perm = perm[1:] + perm[:1]
    spheres = np.array([W.sphere((0.0, 0.0, -6.0 - 3.0 * j), SKEWER_RADII[j % 5], colour_of(i), 4.0 if j % 3 == 0 else 0.0,
                                 W.GLOSSY if j % 2 else W.MATTE, 0.8) for i, j in enumerate(perm)], dtype=W.SPHERE_DTYPE)
    return spheres, W.main_scene()[1]


def skewer_rays(k):
    """64 rays = 8 lateral offsets x 8 origins / directions along the line: from the front, from between spheres (the ones behind the
    origin have tca < 0), from behind the last one, each way, and slightly oblique."""
    z_mid = -6.0 - 3.0 * ((k - 1) // 2) - 1.5
    z_end = -6.0 - 3.0 * (k - 1) - 2.5
    oblique = np.array([0.03, 0.01, -1.0], np.float64)
    oblique = tuple((oblique / np.linalg.norm(oblique)).astype(np.float32))
    starts = [((0.0, 0.0, 0.0), (0.0, 0.0, -1.0)), ((0.0, 0.0, -7.5), (0.0, 0.0, -1.0)), ((0.0, 0.0, z_mid), (0.0, 0.0, -1.0)),
              ((0.0, 0.0, z_end), (0.0, 0.0, -1.0)), ((0.0, 0.0, z_end), (0.0, 0.0, 1.0)), ((0.0, 0.0, z_mid), (0.0, 0.0, 1.0)),
              ((0.0, 0.0, 0.0), (0.0, 0.0, 1.0)), ((0.0, 0.0, 0.0), oblique)]
    return np.array([(o[0] + dx, o[1], o[2]) + tuple(d) for o, d in starts for dx in SKEWER_OFFSETS], np.float32)


@pytest.mark.parametrize("order", ["nearest_first", "nearest_last", "shuffled"])
@pytest.mark.parametrize("k", [2, 3, 5, 9])
def test_skewered_spheres_take_several_passes_per_trace(ctx, pkg, ora, k, order):
    """A ray along the line is a candidate of every sphere in front of it: its lane's stash is taken at each of them, so a pass runs
    at each.  The batch of 64 rays is one wave and mixes lanes with no, one, two and three or more candidates (k = 2 has no lane
    with three: a lane cannot have more candidates than there are spheres); nearest last replaces the accumulator in every pass."""
    scene = skewer(pkg, k, order)
    rays = skewer_rays(k)
    assert len(rays) == 64
    counts, earliest_is_not_nearest = [], False
    for r in rays:
        ts = [ora.distance_to_sphere(r[:3], r[3:], s) for s in scene[0]]
        hits = [(i, t) for i, t in enumerate(ts) if t is not None]
        counts.append(len(hits))
        earliest_is_not_nearest |= len(hits) >= 2 and min(hits, key=lambda it: it[1])[0] != hits[0][0]
    for n in (0, 1, 2):
        assert n in counts, (n, counts)
    assert k < 3 or max(counts) >= 3, counts
    assert earliest_is_not_nearest
    check_rays(ctx, ora, scene, rays, "skewer of %d, %s" % (k, order))
    cam = pkg.world.camera((0.0, 0.0, 0.0), (0.0, 0.0, 0.0), 90)
    for how in ("inline", "streams", "stream"):
        got = check_render(ctx, pkg, ora, scene, cam, 16, 16, 2, how, "skewer of %d, %s" % (k, order))
    assert np.any(got[0] != 0.0)


# ---- 2. every unroll tail of both walks

@pytest.mark.parametrize("ns", [0, 1, 2, 3, 4, 5, 6, 7, 9])
def test_every_unroll_tail_of_both_walks(ctx, pkg, ora, ns):
    """The staged walk takes four spheres per trip, then two, then one (Inline, 16 x 16); the plain walk two and one (eval_check_hit:
    the 8 x 8 primary rays, then 64 rays from the camera at and beside every sphere in turn, so that the last one has candidates)."""
    spheres, planes = pkg.world.scene16()
    scene = (spheres[:ns], planes)
    cam = pkg.world.initial_camera()
    check_render(ctx, pkg, ora, scene, cam, 16, 16, 2, "inline", "%d spheres" % ns)
    rays = [np.concatenate(ora.primary_ray(cam, 8, 8, x, y)) for y in range(8) for x in range(8)]
    for n in range(64 if ns else 0):
        s, m = scene[0][n % ns], n // ns
        aim = s["position"].astype(np.float64) + 0.6 * float(s["radius"]) * np.array([m % 3 - 1, (m // 3) % 3 - 1, 0.0])
        d = aim - cam["position"]
        rays.append(np.concatenate([cam["position"], (d / np.linalg.norm(d)).astype(np.float32)]))
    check_rays(ctx, ora, scene, np.array(rays, np.float32), "%d spheres" % ns)
    if ns:
        assert any(ora.distance_to_sphere(r[:3], r[3:], scene[0][ns - 1]) is not None for r in np.array(rays[64:], np.float32))


# ---- 3. a scene the kernels read from global memory

def test_scene_past_the_lds_limit(ctx, pkg, ora):
    """200 small spheres: 3200 bytes of sphere geometry alone, more than the 3 KB a workgroup stages."""
    W = pkg.world
    spheres = np.array([W.sphere((-9.5 + 1.0 * (j % 20) + 1.0, -2.0 + 0.9 * (j // 20), -9.0 - 0.35 * (j % 7)), 0.3 + 0.02 * (j % 5), colour_of(j),
                                 5.0 if j % 9 == 0 else 0.0, W.GLOSSY if j % 2 else W.MATTE, 0.8) for j in range(200)], dtype=W.SPHERE_DTYPE)
    scene = (spheres, W.main_scene()[1])
    assert 16 * len(spheres) > 3 * 1024
    cam = W.initial_camera()
    got = check_render(ctx, pkg, ora, scene, cam, 16, 16, 1, "inline", "200 spheres")
    check_render(ctx, pkg, ora, scene, cam, 16, 16, 1, "streams", "200 spheres")
    assert np.any(got[0] != 0.0)


# ---- 4. ties and non-hits

def test_the_first_of_two_coincident_spheres_wins(ctx, pkg, ora):
    W = pkg.world
    spheres = np.array([W.sphere((0.0, 0.0, -10.0), 2.0, (1.0, 0.2, 0.2), 5.0, W.MATTE, 0.8),
                        W.sphere((0.0, 0.0, -10.0), 2.0, (0.2, 0.2, 1.0), 9.0, W.GLOSSY, 0.9)], dtype=W.SPHERE_DTYPE)
    scene = (spheres, W.main_scene()[1])
    rays = np.array([(0.0, 0.0, 0.0, 0.0, 0.0, -1.0), (0.5, 0.25, 0.0, 0.0, 0.0, -1.0)], np.float32)
    for r in rays:
        t0, t1 = (ora.distance_to_sphere(r[:3], r[3:], s) for s in spheres)
        assert t0 is not None and t0 == t1
        assert np.array_equal(ora.check_hit(spheres, scene[1], r[:3], r[3:])[2][0], spheres[0]["color"])    # the reference: the earlier one
    ctx.set_scene(*scene)
    t, idx, just = ctx.eval_check_hit(rays)
    assert list(just) == [1, 1] and list(idx) == [0, 0]
    check_rays(ctx, ora, scene, rays, "coincident spheres")
    check_render(ctx, pkg, ora, scene, W.camera((0.0, 0.0, 0.0), (0.0, 0.0, 0.0), 90), 8, 8, 2, "inline", "coincident spheres")


@pytest.mark.parametrize("inside_first", [False, True])
def test_a_candidate_behind_the_origin_is_a_nothing(ctx, pkg, ora, inside_first):
    """The origin lies inside a sphere whose centre is ahead: a candidate (tca >= 0, x >= 0) with t < 0, a Nothing.  It must not
    displace the Just of an earlier sphere, and a later Just replaces it."""
    W = pkg.world
    hit = W.sphere((0.0, 0.0, -10.0), 2.0, (1.0, 0.2, 0.2), 5.0, W.MATTE, 0.8)
    around = W.sphere((0.0, 0.0, -1.0), 3.0, (0.2, 0.2, 1.0), 9.0, W.MATTE, 0.9)
    spheres = np.array([around, hit] if inside_first else [hit, around], dtype=W.SPHERE_DTYPE)
    scene = (spheres, W.main_scene()[1][:0])
    rays = np.array([(0.0, 0.0, 0.0, 0.0, 0.0, -1.0), (0.25, 0.5, 0.0, 0.0, 0.0, -1.0)], np.float32)
    i_hit = 1 if inside_first else 0
    for r in rays:
        assert ora.distance_to_sphere(r[:3], r[3:], spheres[1 - i_hit]) is None and ora.distance_to_sphere(r[:3], r[3:], spheres[i_hit]) is not None
    ctx.set_scene(*scene)
    t, idx, just = ctx.eval_check_hit(rays)
    assert list(just) == [1, 1] and list(idx) == [i_hit, i_hit] and t[0] == np.float32(8.0)
    check_rays(ctx, ora, scene, rays, "origin inside a sphere")
    # alone, the sphere around the origin is no hit at all
    ctx.set_scene(spheres[[1 - i_hit]], scene[1])
    assert list(ctx.eval_check_hit(rays)[2]) == [0, 0]


def test_a_tangent_ray_hits(ctx, pkg, ora):
    """x == 0 exactly: l = (0, 2, -10), tca = 10, d2 = 104 - 100 = 4 = r^2; t = 10 - sqrt 0."""
    W = pkg.world
    spheres = np.array([W.sphere((0.0, 2.0, -10.0), 2.0, (1.0, 0.2, 0.2), 5.0, W.MATTE, 0.8)], dtype=W.SPHERE_DTYPE)
    scene = (spheres, W.main_scene()[1])
    rays = np.array([(0.0, 0.0, 0.0, 0.0, 0.0, -1.0)], np.float32)
    assert ora.distance_to_sphere(rays[0, :3], rays[0, 3:], spheres[0]) == np.float32(10.0)
    ctx.set_scene(*scene)
    t, idx, just = ctx.eval_check_hit(rays)
    assert just[0] == 1 and idx[0] == 0 and t[0] == np.float32(10.0)
    check_rays(ctx, ora, scene, rays, "tangent ray")


def test_a_sphere_wins_the_tie_with_a_plane(ctx, pkg, ora):
    """The ray (0, 0, -1) meets the sphere (centre z = -10, radius 2) and the plane z = -8, tangent to it, at t = 8 in both tests: the
    sphere is folded in the pass behind the last sphere, before the planes."""
    W = pkg.world
    cam = W.camera((0.0, 0.0, 0.0), (0.0, 0.0, 0.0), 90)
    spheres = np.array([W.sphere((0.0, 0.0, -10.0), 2.0, (1.0, 0.2, 0.2), 5.0, W.MATTE, 0.8)], dtype=W.SPHERE_DTYPE)
    planes = np.array([W.plane((0.0, 0.0, -8.0), (0.0, 0.0, 1.0), (0.2, 0.2, 1.0), 9.0, W.MATTE, 0.9),
                       W.plane((0.0, -3.0, 0.0), (0.0, 1.0, 0.0), (0.43, 0.95, 0.5), 0.0, W.MATTE, 1.5)], dtype=W.PLANE_DTYPE)
    o, d = ora.primary_ray(cam, 8, 8, 4, 4)
    assert np.array_equal(d, np.array([0.0, 0.0, -1.0], np.float32))
    ts, tp = ora.distance_to_sphere(o, d, spheres[0]), ora.distance_to_plane(o, d, planes[0])
    assert ts is not None and tp is not None and ts == tp == np.float32(8.0)
    assert np.array_equal(ora.check_hit(spheres, planes, o, d)[2][0], spheres[0]["color"])       # the reference: the sphere, being earlier
    ctx.set_scene(spheres, planes)
    t, idx, just = ctx.eval_check_hit(np.concatenate([o, d])[None, :])
    assert just[0] == 1 and idx[0] == 0 and t[0] == np.float32(8.0)
    check_render(ctx, pkg, ora, (spheres, planes), cam, 8, 8, 2, "inline", "sphere and tangent plane")


# ---- 5. non-finite input

def test_a_nan_sphere_centre_takes_the_literal_fold(ctx, pkg, ora):
    """A NaN centre makes its sphere a candidate of every ray with a NaN key: the wave must fall back to the literal fold and agree
    with the oracle on every plane (colour planes: NaN == NaN by position)."""
    spheres, planes = pkg.world.main_scene()
    spheres = spheres.copy()
    spheres["position"][1] = (6.0, np.nan, -9.0)
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


# ---- 6. the benchmark's scenes on an image with a ragged tile row

@pytest.mark.parametrize("how,spp", [("inline", 4), ("streams", 2), ("stream", 2)])
def test_s16_with_lanes_that_hold_no_pixel(ctx, pkg, ora, how, spp):
    """64 x 40: five rows of 8 x 8 tiles; the lanes of the stream form's last wave and of a part-filled tile hold no pixel."""
    check_render(ctx, pkg, ora, pkg.world.scene16(), pkg.world.initial_camera(), 64, 40, spp, how, "S16")


@pytest.mark.parametrize("stream_form", [False, True])
def test_glass_scene_with_lanes_that_hold_no_pixel(ctx, pkg, ora, stream_form):
    """The glass scene (render Inline refuses GLASS): the tree walk bit for bit; the stream form adds a pixel's rays in no defined
    order, so its RNG planes and bounce count are exact and its colours within tests/test_gpu_wavefront.py's 1e-4."""
    scene = pkg.world.glass_scene()
    cam = pkg.world.initial_camera()
    w, h, spp = 64, 40, 2
    start = initial_planes(ora, w, h)
    got = render_gpu(ctx, pkg, scene, cam, w, h, 15, spp, start, pkg.STREAMS, stream_form)
    live = ctx.stats()["live_bounces"]
    if not stream_form:
        want, live_ref = ora.render_streams_tree(scene[0], scene[1], cam, w, h, CAP, spp, start)[:2]
        assert_planes_equal(got, want, "glass, tree walk")
    else:
        want, live_ref = ora.render_streams_wavefront(scene[0], scene[1], cam, w, h, CAP, spp, start)[:2]
        for a, b in zip(got[3:], want[3:]):
            assert np.array_equal(a, b)
        for a, b in zip(got[:3], want[:3]):
            assert np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-3)) <= 1e-4
    assert live == live_ref
