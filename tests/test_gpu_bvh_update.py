"""ptmi_update_spheres and ptmi_set_bvh_spheres on the device: a BVH or mesh scene's spheres moved by refitting their hierarchy, or
replaced by building a new one, against everything a fresh ptmi_set_scene_bvh / ptmi_set_scene_mesh of the new spheres is tested
against.  The hierarchy read back (ptmi_bvh_read_layout) equals the host twins (ptmi_bvh_refit_layout, ptmi_bvh_layout_morton) bit for
bit at every count at which a kernel takes another path; ptmi_eval_check_hit equals the literal fold over the new spheres; renders equal
a second context set afresh and the linear scene, on all seven planes; an animation of five updates; device tensors, aligned and not;
the refusals, after which the scene renders as before; a partitioned context and a group.  Every comparison is bit-exact."""
import os
import sys

import numpy as np
import pytest

from conftest import assert_planes_equal, initial_planes

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bvh_rays  # noqa: E402
import bvh_update_scenes as scenes  # noqa: E402

pytestmark = pytest.mark.gpu
W = bvh_rays.world
COUNTS = scenes.COUNTS


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return bvh_rays.traverse_lib(tmp_path_factory.mktemp("bvhupdatewalk"))


@pytest.fixture()
def fresh(pkg):
    c = pkg.Context(0)
    yield c
    c.close()


def moved(s, amount, kind, seed=0):
    return W.with_sphere_geometry(s, W.displaced_spheres(W.sphere_geometry(s), amount, kind, seed))


def extent(s):
    return float(np.ptp(s["position"], axis=0).max()) if len(s) > 1 else 1.0


def shoot(c, cam, w, h, limit, spp, start, algorithm):
    c.resize(w, h)
    c.upload_state(*start)
    c.render(cam, limit, spp, algorithm)
    return c.download_state()


def same_layout(got, want, what):
    assert got[0].tobytes() == want[0].tobytes(), "%s: the nodes differ" % what
    assert np.array_equal(got[1], want[1]), "%s: the leaf order differs" % what


def render_scene(glass=False):
    """1 000 spheres and sphere_field's planes: within what ptmi_set_scene holds too"""
    return W.sphere_field(1000, 7, glass_fraction=0.2 if glass else 0.0)


@pytest.mark.parametrize("n", COUNTS)
def test_the_refitted_hierarchy_is_the_host_refits_bit_for_bit(ctx, pkg, n):
    B = pkg.binding
    s, p = scenes.field(n, seed=n)
    nodes, order = B.bvh_layout(s)
    ctx.set_scene_bvh(s, p)
    same_layout(ctx.bvh_read_layout(), (nodes, order), "as set")
    for kind, amount in (("wave", 0.5), ("noise", extent(s))):
        s2 = moved(s, amount, kind, seed=3)
        ctx.update_spheres(W.sphere_geometry(s2))
        want = B.bvh_refit_layout(s2, nodes, order)
        assert n == 0 or want.tobytes() != nodes.tobytes()
        same_layout(ctx.bvh_read_layout(), (want, order), "%d %s" % (n, kind))
    ctx.update_spheres(W.sphere_geometry(s))
    same_layout(ctx.bvh_read_layout(), (nodes, order), "moved back")


@pytest.mark.parametrize("name", sorted(scenes.families()))
def test_the_refit_and_the_build_agree_with_the_host_on_every_family(ctx, pkg, name):
    B = pkg.binding
    s, p = scenes.families()[name]
    nodes, order = B.bvh_layout(s)
    ctx.set_scene_bvh(s, p)
    s2 = moved(s, 0.25 * extent(s), "noise", seed=5)
    ctx.update_spheres(W.sphere_geometry(s2))
    same_layout(ctx.bvh_read_layout(), (B.bvh_refit_layout(s2, nodes, order), order), name + " refitted")
    ctx.set_bvh_spheres(s)
    same_layout(ctx.bvh_read_layout(), B.bvh_layout_morton(s), name + " built")


@pytest.mark.parametrize("n", COUNTS)
def test_the_built_hierarchy_is_the_host_twins_bit_for_bit(ctx, pkg, n):
    """from 300 spheres to n: a count change up or down, to 0 with planes present"""
    B = pkg.binding
    s0, p = scenes.field(300, seed=1)
    s, _ = scenes.field(n, seed=n + 1)
    want = B.bvh_layout_morton(s)
    ctx.set_scene_bvh(s0, p)
    ctx.set_bvh_spheres(s)
    same_layout(ctx.bvh_read_layout(), want, "%d from numpy" % n)
    # ... and an update of the built tree is the host refit of it
    s2 = moved(s, 0.5, "wave", seed=2)
    ctx.update_spheres(W.sphere_geometry(s2))
    same_layout(ctx.bvh_read_layout(), (B.bvh_refit_layout(s2, *want), want[1]), "%d built, then refitted" % n)


def fold_equal(ctx, fresh, lib, s, p, rays, what):
    """t, index and just of ptmi_eval_check_hit: bit for bit those of a context given ptmi_set_scene_bvh with the same spheres, and bit
    for bit the linear fold's -- index and just for every ray, t for every ray whose t is neither NaN nor a zero.  There two ENCODINGS
    differ between the CPU fold and any device scene, a freshly set one included (tests/test_gpu_bvh.py: a NaN key of a NaN origin
    carries the host's or the device's default sign; a ray that starts exactly on a sphere has t = +0 there and -0 here): those rays must
    agree as numbers, and they are counted against the rays that CAN differ so -- the fold's NaN and zero t.
    Measured on these scenes: 69 of 100 000 rays, the same rays for the updated, the built and the freshly set scene."""
    got = ctx.eval_check_hit(rays)
    fresh.set_scene_bvh(s, p)
    again = fresh.eval_check_hit(rays)
    want = bvh_rays.linear_fold(lib, s, p, rays)
    for a, b, name in zip(got, again, ("t", "idx", "just")):
        bad = np.flatnonzero(np.asarray(a).view(np.uint32) != np.asarray(b).view(np.uint32))
        assert bad.size == 0, "%s against a fresh scene: %s differs for %d rays, first %d" % (what, name, bad.size, bad[0])
    for k, name in ((1, "idx"), (2, "just")):
        bad = np.flatnonzero(np.asarray(got[k]).view(np.uint32) != np.asarray(want[k]).view(np.uint32))
        assert bad.size == 0, "%s against the linear fold: %s differs for %d rays, first %d" % (what, name, bad.size, bad[0])
    t0, t1 = np.asarray(got[0]), np.asarray(want[0])
    may_differ = np.isnan(t1) | (t1 == 0)
    differs = t0.view(np.uint32) != t1.view(np.uint32)
    print("%s: t differs from the CPU fold's in encoding only for %d of %d rays (%d have a NaN or zero t)" % (what, differs.sum(), len(rays), may_differ.sum()))
    bad = np.flatnonzero(differs & ~may_differ)
    assert bad.size == 0, "%s against the linear fold: t differs for %d rays, first %d" % (what, bad.size, bad[0])
    bad = np.flatnonzero(differs & ~((t0 == t1) | (np.isnan(t0) & np.isnan(t1))))
    assert bad.size == 0, "%s against the linear fold: t differs as a number for %d rays, first %d" % (what, bad.size, bad[0])
    assert int(differs.sum()) <= int(may_differ.sum()) < len(rays) // 10
    return want


@pytest.mark.parametrize("kind, amount", [("wave", 0.5), ("noise", 8.0)])
def test_check_hit_after_an_update_and_a_set_is_the_fold_over_the_new_spheres(ctx, fresh, pkg, lib, kind, amount):
    s, p = bvh_rays.adversarial_scene(3000, seed=4)
    s2 = moved(s, amount, kind, seed=2)
    rays = bvh_rays.adversarial_rays(s2, 100_000, seed=21)
    ctx.set_scene_bvh(s, p)
    ctx.update_spheres(W.sphere_geometry(s2))
    want = fold_equal(ctx, fresh, lib, s2, p, rays, "updated " + kind)
    # every sphere moved: more than a tenth of the rays hit one (checked on the CPU for this scene and these seeds: 0.62 / 0.43)
    assert int(np.sum(want[2].astype(bool) & (want[1] < len(s2)))) > len(rays) // 10
    ctx.set_scene_bvh(s[:100], p)
    ctx.set_bvh_spheres(s2)
    fold_equal(ctx, fresh, lib, s2, p, rays, "set " + kind)


CASES = [("inline", 8), ("inline", 3), ("streams_keep", 8), ("streams_from_result", 8), ("glass_tree", 8)]


def render_case(pkg, case):
    B = pkg.binding
    algorithm = pkg.INLINE if case == "inline" else pkg.STREAMS
    rule = {"streams_keep": B.SEED_KEEP_ACCUMULATOR, "streams_from_result": B.SEED_FROM_RESULT}.get(case, B.SEED_AUTO)
    return algorithm, rule


@pytest.mark.parametrize("case, limit", CASES)
def test_renders_after_an_update_and_a_set_equal_a_fresh_and_the_linear_scene(ctx, fresh, pkg, ora, case, limit):
    B = pkg.binding
    s, p = render_scene(case == "glass_tree")
    s2 = moved(s, 1.5, "wave", seed=1)
    cam = pkg.world.initial_camera()
    w, h = 64, 48
    start = initial_planes(ora, w, h)
    algorithm, rule = render_case(pkg, case)
    for c in (ctx, fresh):
        c.set_option(B.OPT_STREAMS_SEED_RULE, rule)
    try:
        ctx.set_scene_bvh(s, p)
        before = shoot(ctx, cam, w, h, limit, 2, start, algorithm)
        ctx.update_spheres(W.sphere_geometry(s2))
        updated = shoot(ctx, cam, w, h, limit, 2, start, algorithm)
        ctx.set_scene_bvh(s[:77], p)
        ctx.set_bvh_spheres(s2)
        built = shoot(ctx, cam, w, h, limit, 2, start, algorithm)
        fresh.set_scene_bvh(s2, p)
        again = shoot(fresh, cam, w, h, limit, 2, start, algorithm)
        fresh.set_scene(s2, p)
        linear = shoot(fresh, cam, w, h, limit, 2, start, algorithm)
    finally:
        for c in (ctx, fresh):
            c.set_option(B.OPT_STREAMS_SEED_RULE, B.SEED_AUTO)
    assert_planes_equal(updated, again, "%s after an update, against a fresh scene" % case)
    assert_planes_equal(built, again, "%s after a set, against a fresh scene" % case)
    assert_planes_equal(updated, linear, "%s after an update, against the linear scene" % case)
    assert not np.array_equal(np.asarray(updated[0]), np.asarray(before[0])), "nothing moved"


@pytest.mark.parametrize("case, limit", CASES)
def test_mesh_scene_renders_after_an_update_and_a_set_equal_a_fresh_scene(ctx, fresh, pkg, ora, case, limit):
    B = pkg.binding
    glass = case == "glass_tree"
    _, t, p = W.mesh_room(3)
    s = W.sphere_field(300, 9, glass_fraction=0.2 if glass else 0.0)[0]
    s2 = moved(s, 1.5, "wave", seed=1)
    cam = pkg.world.initial_camera()
    w, h = 64, 48
    start = initial_planes(ora, w, h)
    algorithm, rule = render_case(pkg, case)
    for c in (ctx, fresh):
        c.set_option(B.OPT_STREAMS_SEED_RULE, rule)
    try:
        ctx.set_scene_mesh(s, t, p)
        before = shoot(ctx, cam, w, h, limit, 2, start, algorithm)
        ctx.update_spheres(W.sphere_geometry(s2))
        updated = shoot(ctx, cam, w, h, limit, 2, start, algorithm)
        ctx.set_scene_mesh(s[:40], t, p)
        ctx.set_bvh_spheres(s2)
        built = shoot(ctx, cam, w, h, limit, 2, start, algorithm)
        ctx.set_mesh_triangles(t)                            # (the triangle build finds the scene block where the sphere build put it)
        rebuilt = shoot(ctx, cam, w, h, limit, 2, start, algorithm)
        fresh.set_scene_mesh(s2, t, p)
        again = shoot(fresh, cam, w, h, limit, 2, start, algorithm)
    finally:
        for c in (ctx, fresh):
            c.set_option(B.OPT_STREAMS_SEED_RULE, B.SEED_AUTO)
    assert_planes_equal(updated, again, "mesh %s after an update" % case)
    assert_planes_equal(built, again, "mesh %s after a set" % case)
    assert_planes_equal(rebuilt, again, "mesh %s after a set and new triangles" % case)
    assert not np.array_equal(np.asarray(updated[0]), np.asarray(before[0])), "nothing moved"


@pytest.mark.parametrize("n_new", [20, 1293 + 640])
def test_an_update_after_new_triangles_keeps_the_new_triangles_materials(ctx, fresh, pkg, ora, n_new):
    """update, new triangles of another count (fewer, more) and other materials, update again: the second update must not bring back the
    scene block of the first, which held the old triangles' materials"""
    _, t, p = W.mesh_room(3)
    s = W.sphere_field(300, 9)[0]
    cam = pkg.world.initial_camera()
    w, h = 64, 48
    start = initial_planes(ora, w, h)
    t2 = np.concatenate([t, t[-640:]])[:n_new].copy()
    t2["color"] = t2["color"][:, ::-1] * np.float32(0.5)
    t2["illuminance"] += np.float32(3.0)
    t2["brdf_tag"] = W.GLOSSY
    t2["brdf_param"] = np.float32(0.75)
    s1, s2 = moved(s, 1.0, "wave", seed=1), moved(s, 1.5, "wave", seed=2)
    ctx.set_scene_mesh(s, t, p)
    ctx.update_spheres(W.sphere_geometry(s1))
    ctx.set_mesh_triangles(t2)
    ctx.update_spheres(W.sphere_geometry(s2))
    got = shoot(ctx, cam, w, h, 8, 2, start, pkg.INLINE)
    fresh.set_scene_mesh(s2, t2, p)
    assert_planes_equal(got, shoot(fresh, cam, w, h, 8, 2, start, pkg.INLINE), "update, %d new triangles, update" % n_new)
    ctx.update_spheres(W.sphere_geometry(s1))                   # (the other block of the pair)
    got = shoot(ctx, cam, w, h, 8, 2, start, pkg.INLINE)
    fresh.set_scene_mesh(s1, t2, p)
    assert_planes_equal(got, shoot(fresh, cam, w, h, 8, 2, start, pkg.INLINE), "... and a third update")


def test_an_animation_of_five_updates_equals_a_fresh_scene_every_frame(ctx, fresh, pkg, ora):
    s, p = render_scene()
    cam = pkg.world.initial_camera()
    w, h = 64, 48
    start = initial_planes(ora, w, h)
    ctx.set_scene_bvh(s, p)
    last = None
    for frame in range(5):
        s2 = moved(s, 0.4 * (frame + 1), "wave", seed=frame)
        ctx.update_spheres(W.sphere_geometry(s2))
        got = shoot(ctx, cam, w, h, 8, 1, start, pkg.INLINE)
        fresh.set_scene_bvh(s2, p)
        assert_planes_equal(got, shoot(fresh, cam, w, h, 8, 1, start, pkg.INLINE), "frame %d" % frame)
        assert last is None or not np.array_equal(np.asarray(got[0]), np.asarray(last[0]))
        last = got


TENSOR_SCRIPT = r"""
import os, sys
sys.path.insert(0, %r)
sys.path.insert(0, os.path.join(%r, "tests"))
import numpy as np
import torch
torch.cuda.set_device(0)
torch.zeros(1, device="cuda:0")                          # torch brings the HIP runtime up first: the library then shares it
import bvh_update_scenes as scenes
pkg = scenes.pkg
W, B = pkg.world, pkg.binding
cam = W.initial_camera()
w, h = 64, 48

def shoot(c):
    c.resize(w, h); c.init_output(0x5EED1234); c.render(cam, 8, 2, pkg.INLINE)
    return [np.asarray(x).view(np.uint32) for x in c.download_state()]

def same(a, b, what):
    assert all(np.array_equal(x, y) for x, y in zip(a, b)), what

def same_layout(got, want, what):
    assert got[0].tobytes() == want[0].tobytes() and np.array_equal(got[1], want[1]), what

def words_of(s):
    return np.ascontiguousarray(s).view(np.float32).reshape(-1, 10).copy()

def unaligned(a):                                        # 4 bytes off a 16-byte boundary: the kernels' scalar path
    odd = torch.zeros(a.size + 1, dtype=torch.float32, device="cuda:0")
    odd[1:] = torch.from_numpy(a).to("cuda:0").reshape(-1)
    return odd[1:].reshape(a.shape)

s0, p = scenes.field(300, seed=1)
with pkg.Context(0) as dev:
    # the build from a device tensor at every count, up and down and to 0 with planes present
    for n in scenes.COUNTS:
        s, _ = scenes.field(n, seed=n + 1)
        dev.set_scene_bvh(s0, p)
        d = torch.from_numpy(words_of(s)).to("cuda:0").contiguous()
        torch.cuda.synchronize()
        dev.set_bvh_spheres(d)
        same_layout(dev.bvh_read_layout(), B.bvh_layout_morton(s), "%%d from a device tensor" %% n)
        dev.synchronize()
s, p = W.sphere_field(1000, 7)
s2 = W.with_sphere_geometry(s, W.displaced_spheres(W.sphere_geometry(s), 1.0, "noise", 5))
g, g2 = W.sphere_geometry(s), W.sphere_geometry(s2)
with pkg.Context(0) as host, pkg.Context(0) as dev:
    host.set_scene_bvh(s, p); dev.set_scene_bvh(s, p)
    before = shoot(dev)
    host.update_spheres(g2)
    want_layout, want = host.bvh_read_layout(), shoot(host)
    assert not np.array_equal(want[0], before[0])
    d = torch.from_numpy(g2).to("cuda:0").contiguous()
    odd = unaligned(g2)
    torch.cuda.synchronize()
    for tensor, what in ((d, "aligned"), (odd, "unaligned")):
        dev.update_spheres(torch.from_numpy(g).to("cuda:0"))      # back
        same(shoot(dev), before, what + ": moved back")
        dev.update_spheres(tensor)
        same_layout(dev.bvh_read_layout(), want_layout, what + ": layout")
        same(shoot(dev), want, what + ": planes")
    # the device entries refuse as the host entries do, and the scene stays
    bad = g2.copy(); bad[77, 1] = np.nan
    for arg, names in ((bad, "sphere 77"), (g2[:-1], None)):
        try:
            dev.update_spheres(torch.from_numpy(np.ascontiguousarray(arg)).to("cuda:0"))
            raise SystemExit("a bad update was accepted")
        except B.PtmiError as e:
            assert e.code == B.PTMI_EINVAL and (names is None or names in str(e)), str(e)
    badw = words_of(s2); badw[55, 8] = np.array([17], np.int32).view(np.float32)[0]
    try:
        dev.set_bvh_spheres(torch.from_numpy(badw).to("cuda:0"))
        raise SystemExit("a bad set was accepted")
    except B.PtmiError as e:
        assert e.code == B.PTMI_EINVAL and "sphere 55" in str(e), str(e)
    same_layout(dev.bvh_read_layout(), want_layout, "layout after refusals")
    same(shoot(dev), want, "planes after refusals")
    odd10 = unaligned(words_of(s2))
    torch.cuda.synchronize()
    dev.set_bvh_spheres(odd10)
    same_layout(dev.bvh_read_layout(), B.bvh_layout_morton(s2), "built from an unaligned tensor")
    same(shoot(dev), want, "planes built from an unaligned tensor")
    dev.synchronize()
print("TENSOR_OK")
"""


def test_device_tensors_aligned_and_not_give_what_the_host_arrays_give():
    """In a process of its own, where torch brings the HIP runtime up before the library is loaded (bench.py's order): the build from a
    device tensor at every count, updates and a build from aligned and unaligned tensors, the device entries' refusals."""
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    res = subprocess.run([sys.executable, "-c", TENSOR_SCRIPT % (root, root)], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0 and "TENSOR_OK" in res.stdout, (res.stdout + res.stderr)[-4000:]


def test_refusals_leave_the_scene_as_it_was(ctx, pkg, ora):
    B = pkg.binding
    s, p = render_scene()
    cam = pkg.world.initial_camera()
    w, h = 64, 48
    start = initial_planes(ora, w, h)
    ctx.set_scene_bvh(s, p)
    ctx.update_spheres(W.sphere_geometry(moved(s, 1.0, "wave")))
    before, layout = shoot(ctx, cam, w, h, 8, 2, start, pkg.INLINE), ctx.bvh_read_layout()

    def unchanged(what):
        same_layout(ctx.bvh_read_layout(), layout, "after " + what)
        assert_planes_equal(shoot(ctx, cam, w, h, 8, 2, start, pkg.INLINE), before, "after " + what)

    g = W.sphere_geometry(s)
    nan, big = g.copy(), g.copy()
    nan[471, 2] = np.nan
    nan[900, 0] = np.inf                                         # (the smaller index is the one named)
    big[5, 3] = 1e30                                             # radius^2 overflows
    for bad, names in ((nan, "sphere 471"), (big, "sphere 5"), (g[:-1], None)):
        with pytest.raises(B.PtmiError) as e:
            ctx.update_spheres(bad)
        assert e.value.code == B.PTMI_EINVAL and (names is None or names in str(e.value)), str(e.value)
        unchanged("a refused update (%s)" % (names or "wrong count"))
    with pytest.raises(B.PtmiError) as e:
        ctx._check(ctx._lib.ptmi_update_spheres(ctx._h, None, len(s)))
    assert e.value.code == B.PTMI_EINVAL
    pos, mat, tag = s.copy(), s.copy(), s.copy()
    pos["position"][33, 1] = np.inf
    mat["color"][44, 2] = np.nan
    tag["brdf_tag"][55] = 17
    for bad, names in ((pos, "sphere 33"), (mat, "sphere 44"), (tag, "sphere 55")):
        with pytest.raises(B.PtmiError) as e:
            ctx.set_bvh_spheres(bad)
        assert e.value.code == B.PTMI_EINVAL and names in str(e.value), str(e.value)
        unchanged("a refused set (%s)" % names)
    held = pkg.binding._ptr(np.ascontiguousarray(s))                # (never read: the count is refused first)
    for args, code in (((None, 3), B.PTMI_EINVAL), ((None, -1), B.PTMI_EINVAL), ((held, B.MAX_BVH_SPHERES + 1), B.PTMI_ELIMIT)):
        with pytest.raises(B.PtmiError) as e:
            ctx._check(ctx._lib.ptmi_set_bvh_spheres(ctx._h, *args))
        assert e.value.code == code
    unchanged("bad arguments")
    ctx.set_scene_bvh(s[:9], p[:0])
    with pytest.raises(B.PtmiError) as e:
        ctx.set_bvh_spheres(s[:0])                               # nothing else in the scene
    assert e.value.code == B.PTMI_EINVAL
    same_layout(ctx.bvh_read_layout(), B.bvh_layout(s[:9]), "after a refused empty set")
    sp, pl = pkg.world.scene16()
    ctx.set_scene(sp, pl)
    for call in (lambda: ctx.update_spheres(W.sphere_geometry(sp)), lambda: ctx.set_bvh_spheres(sp), lambda: ctx.bvh_read_layout()):
        with pytest.raises(B.PtmiError) as e:
            call()
        assert e.value.code == B.PTMI_ESTATE
    ctx.resize(32, 16)
    ctx.init_output(1)
    ctx.render(cam, 8, 1)                                        # the linear scene is untouched too


def test_a_partitioned_context_and_a_group_update_as_the_single_context(ctx, pkg, ora):
    s, p = render_scene()
    s2 = moved(s, 1.5, "wave", seed=3)
    g2 = W.sphere_geometry(s2)
    cam = pkg.world.initial_camera()
    w, h, n_parts, stripe = 48, 50, 3, 4
    ctx.set_scene_bvh(s, p)
    ctx.update_spheres(g2)
    ctx.resize(w, h)
    ctx.init_output(0x5EED1234)
    ctx.render(cam, 8, 2)
    want = ctx.download_state()
    stitched = [np.zeros_like(x) for x in want]
    for part in range(n_parts):
        with pkg.Context(0) as c:
            c.set_scene_bvh(s[:500], p)
            c.set_partition(stripe, n_parts, part)
            c.resize(w, h)
            c.set_bvh_spheres(s)
            c.update_spheres(g2)
            rows = c.global_rows()
            c.init_output(0x5EED1234)
            c.render(cam, 8, 2)
            for dst, src in zip(stitched, c.download_state()):
                dst[rows] = src
    assert_planes_equal(stitched, want, "%d stripes after a set and an update" % n_parts)
    with pkg.Group([0], 8) as g:
        g.set_scene_bvh(s[:500], p)
        g.resize(w, h)
        g.set_bvh_spheres(s)
        g.update_spheres(g2)
        g.init_output(0x5EED1234)
        g.render(cam, 8, 2)
        assert_planes_equal(g.download_color(), want[:3], "a one-member group after a set and an update")
        with pytest.raises(pkg.binding.PtmiError) as e:
            g.update_spheres(g2[:-1])
        assert e.value.code == pkg.binding.PTMI_EINVAL
