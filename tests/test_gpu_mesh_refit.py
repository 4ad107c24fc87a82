"""ptmi_update_mesh_vertices on the device: a mesh scene's vertices moved by refitting its hierarchy, against everything a fresh
ptmi_set_scene_mesh of the moved triangles is tested against.  The hierarchy read back (ptmi_mesh_read_layout) equals
ptmi_mesh_refit_layout bit for bit; ptmi_eval_check_hit equals the literal fold over the moved triangles; renders equal the mesh
reference (tests/cxx/mesh_reference.c) and a second context set afresh, on all seven planes; an animation of five updates; the device
tensor entry; the refusals, after which the scene renders as before; a partitioned context and a group."""
import os
import sys

import numpy as np
import pytest

from conftest import assert_planes_equal, initial_planes

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_rays  # noqa: E402
from test_gpu_mesh_renders import scene as room_scene  # noqa: E402

pytestmark = pytest.mark.gpu
CAP = 1 << 16
THREADS = max(1, min(16, os.cpu_count() or 1))
W = mesh_rays.world


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return mesh_rays.reference_lib(tmp_path_factory.mktemp("meshrefitref"))


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return mesh_rays.traverse_lib(tmp_path_factory.mktemp("meshrefitwalk"))


@pytest.fixture()
def fresh(pkg):
    c = pkg.Context(0)
    yield c
    c.close()


def the_scene(pkg, which, glass=False):
    """"room": test_gpu_mesh_renders' scene (mesh_room(3) and a plane); "adversarial": mesh_rays.adversarial_scene(6), 82 757 triangles
    with duplicates, five of zero area and a plane through a triangle"""
    if which == "room":
        return room_scene(pkg, glass)
    s, t, p = mesh_rays.adversarial_scene(6, seed=6)
    if glass:
        t = t.copy()
        t["brdf_tag"][13:] = W.GLASS
        t["brdf_param"][13:] = 1.5
        t["color"][13:] = (0.95, 0.95, 0.95)
    return s, t, p


def moved(t, amount=0.1, kind="wave", seed=0):
    return W.with_vertices(t, W.displaced(W.triangle_vertices(t), amount, kind, seed=seed))


def shoot(c, cam, w, h, limit, spp, start, algorithm):
    c.resize(w, h)
    c.upload_state(*start)
    c.render(cam, limit, spp, algorithm)
    return c.download_state()


def same_layout(got, want, what):
    assert got[0].tobytes() == want[0].tobytes(), "%s: the nodes differ" % what
    assert np.array_equal(got[1], want[1]), "%s: the leaf order differs" % what


@pytest.mark.parametrize("which", ["room", "adversarial"])
def test_the_refitted_hierarchy_is_the_host_refits_bit_for_bit(ctx, pkg, which):
    B = pkg.binding
    s, t, p = the_scene(pkg, which)
    nodes, order = B.mesh_layout(t)
    ctx.set_scene_mesh(s, t, p)
    same_layout(ctx.mesh_read_layout(), (nodes, order), "as set")
    for kind, amount in (("wave", 0.1), ("noise", 1.0)):
        t2 = moved(t, amount, kind)
        ctx.update_mesh_vertices(W.triangle_vertices(t2))
        want = B.mesh_refit_layout(t2, nodes, order)
        assert want.tobytes() != nodes.tobytes()
        same_layout(ctx.mesh_read_layout(), (want, order), "%s %s" % (which, kind))
    ctx.update_mesh_vertices(W.triangle_vertices(t))
    same_layout(ctx.mesh_read_layout(), (nodes, order), "moved back")


@pytest.mark.parametrize("which", ["room", "adversarial"])
@pytest.mark.parametrize("kind, amount", [("wave", 0.1), ("noise", 1.0)])
def test_check_hit_after_an_update_is_the_fold_over_the_moved_triangles(ctx, pkg, lib, which, kind, amount):
    s, t, p = the_scene(pkg, which)
    t2 = moved(t, amount, kind, seed=2)
    ctx.set_scene_mesh(s, t, p)
    ctx.update_mesh_vertices(W.triangle_vertices(t2))
    rays = mesh_rays.adversarial_rays(t2, 100_000, seed=21)
    got = ctx.eval_check_hit(rays)
    want = mesh_rays.linear_fold(lib, s, t2, p, rays)
    for a, b, name in zip(got, want, ("t", "idx", "just")):
        bad = np.flatnonzero(np.asarray(a).view(np.uint32) != np.asarray(b).view(np.uint32))
        assert bad.size == 0, "%s %s: %s differs for %d rays, first %d" % (which, kind, name, bad.size, bad[0])
    first = len(s) + len(p)
    assert int(np.sum(want[2].astype(bool) & (want[1] >= first + 13))) > 10_000          # icosphere triangles are hit


CASES = [("inline", 8), ("inline", 3), ("streams_keep", 8), ("streams_from_result", 8), ("glass_tree", 8)]


@pytest.mark.parametrize("which", ["room", "adversarial"])
@pytest.mark.parametrize("case, limit", CASES)
def test_renders_after_an_update_equal_the_reference_and_a_fresh_scene(ctx, fresh, pkg, ora, ref, which, case, limit):
    B = pkg.binding
    glass = case == "glass_tree"
    s, t, p = the_scene(pkg, which, glass)
    t2 = moved(t, 0.1, "wave", seed=1)
    cam = pkg.world.initial_camera()
    w, h = (67, 45) if which == "room" else (48, 32)
    start = initial_planes(ora, w, h)
    algorithm = pkg.INLINE if case == "inline" else pkg.STREAMS
    rule = {"streams_keep": B.SEED_KEEP_ACCUMULATOR, "streams_from_result": B.SEED_FROM_RESULT}.get(case, B.SEED_AUTO)
    for c in (ctx, fresh):
        c.set_option(B.OPT_STREAMS_SEED_RULE, rule)
    try:
        ctx.set_scene_mesh(s, t, p)
        before = shoot(ctx, cam, w, h, limit, 2, start, algorithm)
        ctx.update_mesh_vertices(W.triangle_vertices(t2))
        got = shoot(ctx, cam, w, h, limit, 2, start, algorithm)
        fresh.set_scene_mesh(s, t2, p)
        again = shoot(fresh, cam, w, h, limit, 2, start, algorithm)
    finally:
        ctx.set_option(B.OPT_STREAMS_SEED_RULE, B.SEED_AUTO)
    with mesh_rays.MeshOracle(ref, t2) as mo:
        if case == "inline":
            want, _ = mo.render_inline(s, p, cam, w, h, limit, 2, start, n_threads=THREADS)
        elif glass:
            want = mo.render_streams_tree(s, p, cam, w, h, CAP, 2, start, n_threads=THREADS)[0]
        else:
            ora_rule = ora.SEED_KEEP_ACCUMULATOR if case == "streams_keep" else ora.SEED_FROM_RESULT
            want, _ = mo.render_streams(s, p, cam, w, h, CAP, 2, start, seed_rule=ora_rule, n_threads=THREADS)
    assert_planes_equal(got, want, "%s %s after an update, against the mesh reference" % (which, case))
    assert_planes_equal(got, again, "%s %s after an update, against a fresh scene" % (which, case))
    assert not np.array_equal(np.asarray(got[0]), np.asarray(before[0])), "nothing moved"


def test_an_animation_of_five_updates_equals_a_fresh_scene_every_frame(ctx, fresh, pkg, ora):
    s, t, p = the_scene(pkg, "room")
    cam = pkg.world.initial_camera()
    w, h = 64, 40
    start = initial_planes(ora, w, h)
    ctx.set_scene_mesh(s, t, p)
    last = None
    for frame in range(5):
        t2 = moved(t, 0.05 * (frame + 1), "wave", seed=frame)
        ctx.update_mesh_vertices(W.triangle_vertices(t2))
        got = shoot(ctx, cam, w, h, 8, 1, start, pkg.INLINE)
        fresh.set_scene_mesh(s, t2, p)
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
import __graft_entry__ as graft
pkg = graft.load_package()
import mesh_rays
from test_gpu_mesh_renders import scene as room_scene
W, B = pkg.world, pkg.binding
cam = W.initial_camera()
w, h = 56, 32

def shoot(c):
    c.resize(w, h); c.init_output(0x5EED1234); c.render(cam, 8, 2, pkg.INLINE)
    return [np.asarray(x).view(np.uint32) for x in c.download_state()]

def same(a, b, what):
    assert all(np.array_equal(x, y) for x, y in zip(a, b)), what

for which in ("room", "adversarial"):
    s, t, p = room_scene(pkg) if which == "room" else mesh_rays.adversarial_scene(6, seed=6)
    v2 = W.displaced(W.triangle_vertices(t), 0.1, "noise", seed=5)
    with pkg.Context(0) as host, pkg.Context(0) as dev:
        host.set_scene_mesh(s, t, p); dev.set_scene_mesh(s, t, p)
        before = shoot(dev)
        host.update_mesh_vertices(v2)
        want_nodes, want_order = host.mesh_read_layout()
        want = shoot(host)
        d = torch.from_numpy(v2).to("cuda:0").contiguous()
        torch.cuda.synchronize()
        dev.update_mesh_vertices(d)
        nodes, order = dev.mesh_read_layout()
        assert nodes.tobytes() == want_nodes.tobytes() and np.array_equal(order, want_order), which + ": layout"
        same(shoot(dev), want, which + ": planes")
        assert not np.array_equal(want[0], before[0])
        dev.update_mesh_vertices(torch.from_numpy(W.triangle_vertices(t)).to("cuda:0"))      # back
        same(shoot(dev), before, which + ": moved back")
        odd = torch.zeros(v2.size + 1, dtype=torch.float32, device="cuda:0")                 # 4 bytes off a 16-byte boundary: the kernels' scalar path
        odd[1:] = d.reshape(-1)
        torch.cuda.synchronize()
        dev.update_mesh_vertices(odd[1:].reshape(-1, 9))
        nodes, order = dev.mesh_read_layout()
        assert nodes.tobytes() == want_nodes.tobytes(), which + ": layout from an unaligned tensor"
        same(shoot(dev), want, which + ": planes from an unaligned tensor")
        # the device entry refuses as the host entry does, and the scene stays
        bad = v2.copy(); bad[77, 2, 1] = np.nan
        for arg, names in ((bad, "triangle 77"), (v2[:-1], None)):
            try:
                dev.update_mesh_vertices(torch.from_numpy(np.ascontiguousarray(arg)).to("cuda:0"))
                raise SystemExit("a bad update was accepted")
            except B.PtmiError as e:
                assert e.code == B.PTMI_EINVAL and (names is None or names in str(e)), str(e)
        same(shoot(dev), want, which + ": planes after refusals")
print("TENSOR_OK")
"""


def test_a_device_tensor_gives_what_the_host_array_gives():
    """In a process of its own, where torch brings the HIP runtime up before the library is loaded (bench.py's order)."""
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    res = subprocess.run([sys.executable, "-c", TENSOR_SCRIPT % (root, root)], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0 and "TENSOR_OK" in res.stdout, (res.stdout + res.stderr)[-4000:]


def test_refused_updates_leave_the_scene_as_it_was(ctx, pkg, ora):
    B = pkg.binding
    s, t, p = the_scene(pkg, "adversarial")
    cam = pkg.world.initial_camera()
    w, h = 64, 40
    start = initial_planes(ora, w, h)
    ctx.set_scene_mesh(s, t, p)
    ctx.update_mesh_vertices(W.triangle_vertices(moved(t, 0.1, "wave")))
    before, layout = shoot(ctx, cam, w, h, 8, 2, start, pkg.INLINE), ctx.mesh_read_layout()
    v = W.triangle_vertices(t)
    flat = len(t) - 2                                             # one of the five triangles of zero area
    nan, area = v.copy(), v.copy()
    nan[4711, 1, 2] = np.nan
    nan[60000, 0, 0] = np.inf                                    # (the smaller index is the one named)
    area[flat, 2] += np.float32(0.5)
    for bad, code, names in ((nan, B.PTMI_EINVAL, "triangle 4711"), (v[:-1], B.PTMI_EINVAL, None), (area, B.PTMI_EINVAL, "triangle %d" % flat)):
        with pytest.raises(B.PtmiError) as e:
            ctx.update_mesh_vertices(bad)
        assert e.value.code == code, str(e.value)
        if names:
            assert names in str(e.value), str(e.value)
        if bad is area:
            assert "ptmi_set_scene_mesh" in str(e.value)
        same_layout(ctx.mesh_read_layout(), layout, "after a refusal")
        assert_planes_equal(shoot(ctx, cam, w, h, 8, 2, start, pkg.INLINE), before, "after a refused update (%s)" % (names or "wrong count"))
    with pytest.raises(B.PtmiError) as e:
        ctx._check(ctx._lib.ptmi_update_mesh_vertices(ctx._h, None, len(t)))
    assert e.value.code == B.PTMI_EINVAL
    sp, pl = pkg.world.scene16()
    for setter in (ctx.set_scene, ctx.set_scene_bvh):
        setter(sp, pl)
        with pytest.raises(B.PtmiError) as e:
            ctx.update_mesh_vertices(v)
        assert e.value.code == B.PTMI_ESTATE
        with pytest.raises(B.PtmiError) as e:
            ctx.mesh_read_layout()
        assert e.value.code == B.PTMI_ESTATE
        ctx.resize(32, 16)
        ctx.init_output(1)
        ctx.render(cam, 8, 1)                                     # the non-mesh scene is untouched too


def test_a_kept_triangle_collapsed_to_a_point_is_accepted(ctx, fresh, pkg, ora):
    s, t, p = the_scene(pkg, "room")
    cam = pkg.world.initial_camera()
    w, h = 64, 40
    start = initial_planes(ora, w, h)
    col = t.copy()
    for k in range(13, 400, 7):
        col["v1"][k] = col["v0"][k]
        col["v2"][k] = col["v0"][k]
    ctx.set_scene_mesh(s, t, p)
    ctx.update_mesh_vertices(W.triangle_vertices(col))
    fresh.set_scene_mesh(s, col, p)
    assert_planes_equal(shoot(ctx, cam, w, h, 8, 2, start, pkg.INLINE), shoot(fresh, cam, w, h, 8, 2, start, pkg.INLINE), "collapsed triangles")


def test_a_partitioned_context_and_a_group_update_as_the_single_context(ctx, pkg, ora):
    s, t, p = the_scene(pkg, "room")
    t2 = moved(t, 0.1, "wave", seed=3)
    v2 = W.triangle_vertices(t2)
    cam = pkg.world.initial_camera()
    w, h, n_parts, stripe = 48, 50, 3, 4
    ctx.set_scene_mesh(s, t, p)
    ctx.update_mesh_vertices(v2)
    ctx.resize(w, h)
    ctx.init_output(0x5EED1234)
    ctx.render(cam, 8, 2)
    want = ctx.download_state()
    stitched = [np.zeros_like(x) for x in want]
    for part in range(n_parts):
        with pkg.Context(0) as c:
            c.set_scene_mesh(s, t, p)
            c.set_partition(stripe, n_parts, part)
            c.resize(w, h)
            c.update_mesh_vertices(v2)
            rows = c.global_rows()
            c.init_output(0x5EED1234)
            c.render(cam, 8, 2)
            for dst, src in zip(stitched, c.download_state()):
                dst[rows] = src
    assert_planes_equal(stitched, want, "%d stripes after an update" % n_parts)
    with pkg.Group([0], 8) as g:
        g.set_scene_mesh(s, t, p)
        g.resize(w, h)
        g.update_mesh_vertices(v2)
        g.init_output(0x5EED1234)
        g.render(cam, 8, 2)
        assert_planes_equal(g.download_color(), want[:3], "a one-member group after an update")
        with pytest.raises(pkg.binding.PtmiError) as e:
            g.update_mesh_vertices(v2[:-1])
        assert e.value.code == pkg.binding.PTMI_EINVAL
