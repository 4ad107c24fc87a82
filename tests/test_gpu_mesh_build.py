"""ptmi_set_mesh_triangles on the device: a mesh scene given new triangles -- another count, another mesh -- whose hierarchy is built on
the device.  The hierarchy read back (ptmi_mesh_read_layout) equals ptmi_mesh_layout_morton bit for bit; all seven planes of every
render, Inline and Streams, GLASS included, and ptmi_eval_check_hit equal those of a fresh context given ptmi_set_scene_mesh; a later
ptmi_update_mesh_vertices equals a fresh scene with the moved triangles; the device tensor entry; the refusals, after which the scene
renders and reads back as before; a partitioned context and a group.  Renders are 64 x 48, 2 samples, limit 4."""
import os
import sys

import numpy as np
import pytest

from conftest import assert_planes_equal, initial_planes

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_rays  # noqa: E402
from test_gpu_mesh_renders import scene as room_scene  # noqa: E402
from test_mesh_morton_layout import FAMILIES  # noqa: E402

pytestmark = pytest.mark.gpu
W = mesh_rays.world
WIDTH, HEIGHT, SPP, LIMIT = 64, 48, 2, 4


@pytest.fixture()
def fresh(pkg):
    c = pkg.Context(0)
    yield c
    c.close()


def shoot(c, cam, start, algorithm):
    c.resize(WIDTH, HEIGHT)
    c.upload_state(*start)
    c.render(cam, LIMIT, SPP, algorithm)
    return c.download_state()


def same_layout(got, want, what):
    assert got[0].tobytes() == want[0].tobytes(), "%s: the nodes differ" % what
    assert np.array_equal(got[1], want[1]), "%s: the leaf order differs" % what


def icosphere5():
    s, t, p = W.mesh_room(5)
    assert len(t) == 20_493
    return s, t, p, t


def glassy(t):
    t = t.copy()
    t["brdf_tag"][13:] = W.GLASS
    t["brdf_param"][13:] = 1.5
    t["color"][13:] = (0.95, 0.95, 0.95)
    return t


@pytest.mark.parametrize("family", sorted(FAMILIES) + ["icosphere5"])
def test_the_device_built_hierarchy_is_the_host_twins_bit_for_bit(ctx, pkg, family):
    B = pkg.binding
    s, t, p, _ = icosphere5() if family == "icosphere5" else FAMILIES[family]()
    s0, t0, p0 = room_scene(pkg)
    if len(s) + len(p) == 0:                                        # (a scene of triangles alone may not be given 0 of them: these have some)
        s0, p0 = s, p
    ctx.set_scene_mesh(s0, t0, p0)
    ctx.set_mesh_triangles(t)
    same_layout(ctx.mesh_read_layout(), B.mesh_layout_morton(t), family)


CASES = [("inline", False), ("streams_keep", False), ("streams_from_result", False), ("glass_tree", True)]


@pytest.mark.parametrize("case, glass", CASES)
def test_renders_and_check_hit_equal_a_fresh_scene_through_count_changes(ctx, fresh, pkg, ora, case, glass):
    """1 293 -> 5 -> 20 493 triangles; with `glass` the new triangles bring the scene's only GLASS (has_glass comes from the device)"""
    B = pkg.binding
    s, t, p = room_scene(pkg)
    big = W.mesh_room(5)[1]
    steps = [t[13:18].copy(), glassy(big) if glass else big, glassy(t) if glass else mesh_rays.adversarial_scene(3, seed=4)[1]]
    cam = pkg.world.initial_camera()
    start = initial_planes(ora, WIDTH, HEIGHT)
    algorithm = pkg.INLINE if case == "inline" else pkg.STREAMS
    rule = {"streams_keep": B.SEED_KEEP_ACCUMULATOR, "streams_from_result": B.SEED_FROM_RESULT}.get(case, B.SEED_AUTO)
    for c in (ctx, fresh):
        c.set_option(B.OPT_STREAMS_SEED_RULE, rule)
    try:
        ctx.set_scene_mesh(s, t, p)
        last = shoot(ctx, cam, start, algorithm)
        for k, t2 in enumerate(steps):
            ctx.set_mesh_triangles(t2)
            got = shoot(ctx, cam, start, algorithm)
            fresh.set_scene_mesh(s, t2, p)
            assert_planes_equal(got, shoot(fresh, cam, start, algorithm), "%s, step %d (%d triangles)" % (case, k, len(t2)))
            assert not np.array_equal(np.asarray(got[0]), np.asarray(last[0])), "step %d changed nothing" % k
            last = got
            rays = mesh_rays.adversarial_rays(t2, 20_000, seed=k)
            for a, b, name in zip(ctx.eval_check_hit(rays), fresh.eval_check_hit(rays), ("t", "idx", "just")):
                assert np.array_equal(np.asarray(a).view(np.uint32), np.asarray(b).view(np.uint32)), "%s step %d: %s" % (case, k, name)
    finally:
        for c in (ctx, fresh):
            c.set_option(B.OPT_STREAMS_SEED_RULE, B.SEED_AUTO)


def test_an_update_after_a_build_equals_a_fresh_scene_and_zero_areas_stay_out(ctx, fresh, pkg, ora):
    B = pkg.binding
    s, t, p = room_scene(pkg)
    _, t2, _, _ = FAMILIES["zero_areas"]()
    cam = pkg.world.initial_camera()
    start = initial_planes(ora, WIDTH, HEIGHT)
    ctx.set_scene_mesh(s, t, p)
    ctx.set_mesh_triangles(t2)
    nodes, order = ctx.mesh_read_layout()
    moved = W.with_vertices(t2, W.displaced(W.triangle_vertices(t2), 0.1, "wave", seed=1))
    ctx.update_mesh_vertices(W.triangle_vertices(moved))
    same_layout(ctx.mesh_read_layout(), (B.mesh_refit_layout(moved, nodes, order), order), "refit of a device-built hierarchy")
    fresh.set_scene_mesh(s, moved, p)
    for algorithm in (pkg.INLINE, pkg.STREAMS):
        assert_planes_equal(shoot(ctx, cam, start, algorithm), shoot(fresh, cam, start, algorithm), "an update after a build")
    before = shoot(ctx, cam, start, pkg.INLINE)
    area = W.triangle_vertices(moved)
    area[0, 2] += np.float32(0.5)                                   # triangle 0 had zero area at the build
    with pytest.raises(B.PtmiError) as e:
        ctx.update_mesh_vertices(area)
    assert e.value.code == B.PTMI_EINVAL and "triangle 0 " in str(e.value), str(e.value)
    assert_planes_equal(shoot(ctx, cam, start, pkg.INLINE), before, "after the refused update")


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
from test_gpu_mesh_renders import scene as room_scene
W, B = pkg.world, pkg.binding
cam = W.initial_camera()

def shoot(c):
    c.resize(64, 48); c.init_output(0x5EED1234); c.render(cam, 4, 2, pkg.INLINE)
    return [np.asarray(x).view(np.uint32) for x in c.download_state()]

def same(a, b, what):
    assert all(np.array_equal(x, y) for x, y in zip(a, b)), what

def as_tensor(t):
    flat = np.ascontiguousarray(t).view(np.float32).reshape(-1, 15)       # brdf_tag as its bit pattern
    return torch.from_numpy(flat.copy()).to("cuda:0").contiguous()

s, t, p = room_scene(pkg)
t2 = W.mesh_room(5)[1]
with pkg.Context(0) as host, pkg.Context(0) as dev:
    host.set_scene_mesh(s, t, p); dev.set_scene_mesh(s, t, p)
    before = shoot(dev)
    host.set_mesh_triangles(t2)
    want_nodes, want_order = host.mesh_read_layout()
    want = shoot(host)
    d = as_tensor(t2)
    torch.cuda.synchronize()
    dev.set_mesh_triangles(d)
    nodes, order = dev.mesh_read_layout()
    assert nodes.tobytes() == want_nodes.tobytes() and np.array_equal(order, want_order), "layout"
    same(shoot(dev), want, "planes")
    assert not np.array_equal(want[0], before[0])
    odd = torch.zeros(d.numel() + 1, dtype=torch.float32, device="cuda:0")     # 4 bytes off a 16-byte boundary: the kernels' scalar path
    odd[1:] = d.reshape(-1)
    torch.cuda.synchronize()
    dev.set_mesh_triangles(as_tensor(t))
    dev.set_mesh_triangles(odd[1:].reshape(-1, 15))
    nodes, order = dev.mesh_read_layout()
    assert nodes.tobytes() == want_nodes.tobytes() and np.array_equal(order, want_order), "layout from an unaligned tensor"
    same(shoot(dev), want, "planes from an unaligned tensor")
    bad = t2.copy(); bad["v1"][77, 1] = np.nan
    try:
        dev.set_mesh_triangles(as_tensor(bad))
        raise SystemExit("bad triangles were accepted")
    except B.PtmiError as e:
        assert e.code == B.PTMI_EINVAL and "triangle 77" in str(e), str(e)
    try:
        dev.set_mesh_triangles(d.reshape(-1)[:-1])
        raise SystemExit("a tensor that is no whole number of triangles was accepted")
    except ValueError:
        pass
    same(shoot(dev), want, "planes after refusals")
print("TENSOR_OK")
"""


def test_a_device_tensor_gives_what_the_host_array_gives():
    """In a process of its own, where torch brings the HIP runtime up before the library is loaded (bench.py's order)."""
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    res = subprocess.run([sys.executable, "-c", TENSOR_SCRIPT % (root, root)], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0 and "TENSOR_OK" in res.stdout, (res.stdout + res.stderr)[-4000:]


def test_refusals_leave_the_renders_and_the_layout_as_they_were(ctx, pkg, ora):
    B = pkg.binding
    s, t, p = room_scene(pkg)
    big = W.mesh_room(5)[1]
    cam = pkg.world.initial_camera()
    start = initial_planes(ora, WIDTH, HEIGHT)
    ctx.set_scene_mesh(s, t, p)
    ctx.set_mesh_triangles(big)
    before, layout = shoot(ctx, cam, start, pkg.INLINE), ctx.mesh_read_layout()

    def spoiled(field, value, k=4711, also=None):
        bad = big.copy()
        if bad[field].ndim == 2:
            bad[field][k, 1] = value
        else:
            bad[field][k] = value
        if also:
            bad[also[0]][also[1], 0] = also[2]
        return bad
    huge = spoiled("v2", 3e38)
    huge["v0"][4711, 1] = -3e38                                     # finite vertices, an edge that is not
    cases = [(spoiled("v1", np.nan, also=("v0", 20000, np.inf)), "triangle 4711"), (spoiled("color", np.inf), "triangle 4711"),
             (spoiled("illuminance", np.nan), "triangle 4711"), (spoiled("brdf_param", np.inf), "triangle 4711"), (huge, "triangle 4711"),
             (spoiled("brdf_tag", 7), "triangle 4711"), (spoiled("brdf_tag", -1, k=20492), "triangle 20492")]
    for bad, names in cases:
        with pytest.raises(B.PtmiError) as e:
            ctx.set_mesh_triangles(bad)
        assert e.value.code == B.PTMI_EINVAL and names in str(e.value), str(e.value)
        same_layout(ctx.mesh_read_layout(), layout, "after a refusal")
    assert_planes_equal(shoot(ctx, cam, start, pkg.INLINE), before, "after refused triangles")
    for call, code in ((lambda: ctx._lib.ptmi_set_mesh_triangles(ctx._h, None, 5), B.PTMI_EINVAL),
                       (lambda: ctx._lib.ptmi_set_mesh_triangles(ctx._h, B._ptr(big), -1), B.PTMI_EINVAL),
                       (lambda: ctx._lib.ptmi_set_mesh_triangles_device(ctx._h, None, 5), B.PTMI_EINVAL),
                       (lambda: ctx._lib.ptmi_set_mesh_triangles(ctx._h, B._ptr(big), (1 << 22) + 1), B.PTMI_ELIMIT)):
        assert call() == code
    same_layout(ctx.mesh_read_layout(), layout, "after refused arguments")
    assert_planes_equal(shoot(ctx, cam, start, pkg.INLINE), before, "after refused arguments")
    # 0 triangles: fine beside spheres and planes, refused where nothing would be left
    ctx.set_mesh_triangles(big[:0])
    assert len(ctx.mesh_read_layout()[1]) == 0
    none_s, none_p = s[:0], p[:0]
    ctx.set_scene_mesh(none_s, t, none_p)
    only = shoot(ctx, cam, start, pkg.INLINE)
    with pytest.raises(B.PtmiError) as e:
        ctx.set_mesh_triangles(t[:0])
    assert e.value.code == B.PTMI_EINVAL
    assert_planes_equal(shoot(ctx, cam, start, pkg.INLINE), only, "after a refused emptying")
    sp, pl = pkg.world.scene16()
    for setter in (ctx.set_scene, ctx.set_scene_bvh):
        setter(sp, pl)
        with pytest.raises(B.PtmiError) as e:
            ctx.set_mesh_triangles(t)
        assert e.value.code == B.PTMI_ESTATE
        ctx.resize(32, 16)
        ctx.init_output(1)
        ctx.render(cam, 8, 1)                                       # the non-mesh scene is untouched too


def test_a_partitioned_context_and_a_group_build_as_the_single_context(ctx, pkg):
    s, t, p = room_scene(pkg)
    t2 = W.mesh_room(4)[1]
    cam = pkg.world.initial_camera()
    w, h, n_parts, stripe = 48, 50, 3, 4
    ctx.set_scene_mesh(s, t, p)
    ctx.set_mesh_triangles(t2)
    ctx.resize(w, h)
    ctx.init_output(0x5EED1234)
    ctx.render(cam, LIMIT, SPP)
    want = ctx.download_state()
    stitched = [np.zeros_like(x) for x in want]
    for part in range(n_parts):
        with pkg.Context(0) as c:
            c.set_scene_mesh(s, t, p)
            c.set_partition(stripe, n_parts, part)
            c.resize(w, h)
            c.set_mesh_triangles(t2)
            rows = c.global_rows()
            c.init_output(0x5EED1234)
            c.render(cam, LIMIT, SPP)
            for dst, src in zip(stitched, c.download_state()):
                dst[rows] = src
    assert_planes_equal(stitched, want, "%d stripes after a build" % n_parts)
    with pkg.Group([0], 8) as g:
        g.set_scene_mesh(s, t, p)
        g.resize(w, h)
        g.set_mesh_triangles(t2)
        g.init_output(0x5EED1234)
        g.render(cam, LIMIT, SPP)
        assert_planes_equal(g.download_color(), want[:3], "a one-member group after a build")
        bad = t2.copy()
        bad["v0"][5, 0] = np.nan
        with pytest.raises(pkg.binding.PtmiError) as e:
            g.set_mesh_triangles(bad)
        assert e.value.code == pkg.binding.PTMI_EINVAL
