"""ptmi_set_bvh_spheres under PTMI_OPT_BVH_DEVICE_BUILD = PTMI_BVH_BUILD_SPATIAL on the device: the hierarchy read back
(ptmi_bvh_read_layout) equals the host twin ptmi_bvh_layout_spatial bit for bit, nodes and order, from a numpy array and from a device
tensor, at the counts at which a kernel or the root takes another path and on the families of tests/bvh_spatial_scenes.py -- the chain on
which the depth guard acts among them; renders (Inline, Streams under both seed rules, the GLASS tree walk; 64 x 48, 2 spp, bounce limit 4)
and ptmi_eval_check_hit equal a fresh ptmi_set_scene_bvh bitwise; a later ptmi_update_spheres refits the spatial tree as
ptmi_bvh_refit_layout refits the twin; a mesh scene and a group of one member; the default builds ptmi_bvh_layout_morton's tree as
before; refusals leave the scene as it was."""
import os
import sys

import numpy as np
import pytest

from conftest import assert_planes_equal, initial_planes

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bvh_rays  # noqa: E402
import bvh_spatial_scenes as spatial  # noqa: E402
import bvh_update_scenes as scenes  # noqa: E402

pytestmark = pytest.mark.gpu
W = bvh_rays.world
COUNTS = (0, 1, 4, 5, 64, 1020, 5000)
WIDTH, HEIGHT, SPP, LIMIT = 64, 48, 2, 4
RENDERS = ("inline", "streams_keep", "streams_from_result")


@pytest.fixture(scope="module")
def sctx(pkg):
    """a context of this module's own whose later ptmi_set_bvh_spheres build the spatial tree"""
    c = pkg.Context(0)
    c.set_option(pkg.binding.OPT_BVH_DEVICE_BUILD, pkg.binding.BVH_BUILD_SPATIAL)
    yield c
    c.close()


@pytest.fixture(scope="module")
def fresh(pkg):
    c = pkg.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def start(ora):
    return initial_planes(ora, WIDTH, HEIGHT)


@pytest.fixture(scope="module")
def rays():
    """one set of adversarial rays for every scene: aimed at a field of 1 020 spheres, which the other fields overlap"""
    return bvh_rays.adversarial_rays(scenes.field(1020, seed=24)[0], 20_000, seed=21)


def same_layout(got, want, what):
    assert got[0].tobytes() == want[0].tobytes(), "%s: the nodes differ" % what
    assert np.array_equal(got[1], want[1]), "%s: the leaf order differs" % what


def shoot(pkg, c, start, case):
    B = pkg.binding
    algorithm = pkg.INLINE if case == "inline" else pkg.STREAMS
    rule = {"streams_keep": B.SEED_KEEP_ACCUMULATOR, "streams_from_result": B.SEED_FROM_RESULT}.get(case, B.SEED_AUTO)
    c.set_option(B.OPT_STREAMS_SEED_RULE, rule)
    try:
        c.resize(WIDTH, HEIGHT)
        c.upload_state(*start)
        c.render(pkg.world.initial_camera(), LIMIT, SPP, algorithm)
        return c.download_state()
    finally:
        c.set_option(B.OPT_STREAMS_SEED_RULE, B.SEED_AUTO)


def same_hits(c, fresh, rays, what):
    got, want = c.eval_check_hit(rays), fresh.eval_check_hit(rays)
    for a, b, name in zip(got, want, ("t", "idx", "just")):
        bad = np.flatnonzero(np.asarray(a).view(np.uint32) != np.asarray(b).view(np.uint32))
        assert bad.size == 0, "%s: %s of ptmi_eval_check_hit differs from a fresh scene's for %d rays, first %d" % (what, name, bad.size, bad[0])


def check_built(pkg, sctx, fresh, start, rays, s, p, what, cases=RENDERS):
    """sctx holds a scene into which `s` was just built: the twin's tree, and a fresh scene's results"""
    same_layout(sctx.bvh_read_layout(), pkg.binding.bvh_layout_spatial(s), what)
    fresh.set_scene_bvh(s, p)
    for case in cases:
        assert_planes_equal(shoot(pkg, sctx, start, case), shoot(pkg, fresh, start, case), "%s, %s" % (what, case))
    same_hits(sctx, fresh, rays, what)


@pytest.mark.parametrize("n", COUNTS)
def test_the_built_tree_is_the_twins_and_the_results_are_a_fresh_scenes(pkg, sctx, fresh, start, rays, n):
    """from 300 spheres to n: up and down, to 0 with planes present"""
    s0, p = scenes.field(300, seed=1)
    s, _ = scenes.field(n, seed=24)
    sctx.set_scene_bvh(s0, p)
    sctx.set_bvh_spheres(s)
    check_built(pkg, sctx, fresh, start, rays, s, p, "%d spheres from numpy" % n)
    if n >= 5:
        assert sctx.bvh_read_layout()[0].tobytes() != pkg.binding.bvh_layout_morton(s)[0].tobytes(), "the option chose nothing"


def test_the_glass_tree_walk_over_the_spatial_tree(pkg, sctx, fresh, start, rays):
    s, p = W.sphere_field(1000, 7, glass_fraction=0.2)
    sctx.set_scene_bvh(s[:77], p)
    sctx.set_bvh_spheres(s)
    check_built(pkg, sctx, fresh, start, rays, s, p, "a field with GLASS", cases=("glass_tree",))


@pytest.mark.parametrize("name", sorted(spatial.families()))
def test_the_special_scenes(pkg, sctx, fresh, start, rays, name):
    s, p = spatial.families()[name]
    sctx.set_scene_bvh(scenes.field(300, seed=1)[0], p)
    sctx.set_bvh_spheres(s)
    check_built(pkg, sctx, fresh, start, bvh_rays.adversarial_rays(s, 20_000, seed=9), s, p, name, cases=("inline", "streams_keep"))
    if name == "chain":
        assert spatial.levels_of(sctx.bvh_read_layout()[0]).max() == pkg.binding.BVH_MAX_DEPTH - 1


def test_a_later_update_refits_the_spatial_tree(pkg, sctx, fresh, start, rays):
    B = pkg.binding
    s, p = scenes.field(1020, seed=24)
    s2 = W.with_sphere_geometry(s, W.displaced_spheres(W.sphere_geometry(s), 1.5, "wave", 1))
    sctx.set_scene_bvh(s[:100], p)
    sctx.set_bvh_spheres(s)
    nodes, order = B.bvh_layout_spatial(s)
    for moved, what in ((s2, "moved"), (s, "moved back")):
        sctx.update_spheres(W.sphere_geometry(moved))
        want = B.bvh_refit_layout(moved, nodes, order)
        same_layout(sctx.bvh_read_layout(), (want, order), what)
        fresh.set_scene_bvh(moved, p)
        for case in ("inline", "streams_keep"):
            assert_planes_equal(shoot(pkg, sctx, start, case), shoot(pkg, fresh, start, case), "%s, %s" % (what, case))
        same_hits(sctx, fresh, rays, what)
    assert B.bvh_refit_layout(s2, nodes, order).tobytes() != nodes.tobytes()


def test_a_mesh_scene_builds_the_spatial_tree_and_keeps_its_triangles(pkg, sctx, fresh, start):
    _, t, p = W.mesh_room(3)
    s = W.sphere_field(300, 9)[0]
    sctx.set_scene_mesh(s[:40], t, p)
    triangles_before = sctx.mesh_read_layout()
    sctx.set_bvh_spheres(s)
    same_layout(sctx.bvh_read_layout(), pkg.binding.bvh_layout_spatial(s), "a mesh scene")
    after = sctx.mesh_read_layout()
    assert after[0].tobytes() == triangles_before[0].tobytes() and np.array_equal(after[1], triangles_before[1])
    fresh.set_scene_mesh(s, t, p)
    for case in ("inline", "streams_keep"):
        assert_planes_equal(shoot(pkg, sctx, start, case), shoot(pkg, fresh, start, case), "a mesh scene, %s" % case)
    s2 = W.with_sphere_geometry(s, W.displaced_spheres(W.sphere_geometry(s), 1.0, "wave", 2))
    sctx.update_spheres(W.sphere_geometry(s2))
    fresh.set_scene_mesh(s2, t, p)
    assert_planes_equal(shoot(pkg, sctx, start, "inline"), shoot(pkg, fresh, start, "inline"), "a mesh scene after an update")


def test_a_group_of_one_member_takes_the_option(pkg, fresh):
    B = pkg.binding
    s, p = scenes.field(1020, seed=24)
    cam = pkg.world.initial_camera()
    fresh.set_scene_bvh(s, p)
    fresh.resize(WIDTH, HEIGHT)
    fresh.init_output(0x5EED1234)
    fresh.render(cam, LIMIT, SPP)
    want = fresh.download_state()
    with pkg.Group([0], 8) as g:
        g.set_option(B.OPT_BVH_DEVICE_BUILD, B.BVH_BUILD_SPATIAL)
        for bad in (2, -1):
            with pytest.raises(B.PtmiError) as e:
                g.set_option(B.OPT_BVH_DEVICE_BUILD, bad)                    # (the members refuse it: the option does reach them)
            assert e.value.code == B.PTMI_EINVAL
        g.set_scene_bvh(s[:500], p)
        g.resize(WIDTH, HEIGHT)
        g.set_bvh_spheres(s)
        g.init_output(0x5EED1234)
        g.render(cam, LIMIT, SPP)
        assert_planes_equal(g.download_color(), want[:3], "a one-member group over the spatial tree")


def test_the_default_builds_todays_tree_and_the_option_leaves_the_scene_alone(pkg, fresh):
    B = pkg.binding
    s0, p = scenes.field(300, seed=1)
    s, _ = scenes.field(1020, seed=24)
    with pkg.Context(0) as c:
        assert c.get_option(B.OPT_BVH_DEVICE_BUILD) == B.BVH_BUILD_EQUAL_COUNT
        c.set_scene_bvh(s0, p)
        c.set_bvh_spheres(s)
        same_layout(c.bvh_read_layout(), B.bvh_layout_morton(s), "the default")
        c.set_option(B.OPT_BVH_DEVICE_BUILD, B.BVH_BUILD_SPATIAL)
        assert c.get_option(B.OPT_BVH_DEVICE_BUILD) == B.BVH_BUILD_SPATIAL
        same_layout(c.bvh_read_layout(), B.bvh_layout_morton(s), "setting the option changes nothing held")
        c.set_scene_bvh(s, p)                                        # the scene call does not look at it
        same_layout(c.bvh_read_layout(), B.bvh_layout(s), "ptmi_set_scene_bvh under the option")
        c.set_bvh_spheres(s)
        same_layout(c.bvh_read_layout(), B.bvh_layout_spatial(s), "the option")
        for bad in (2, -1):
            with pytest.raises(B.PtmiError) as e:
                c.set_option(B.OPT_BVH_DEVICE_BUILD, bad)
            assert e.value.code == B.PTMI_EINVAL
        assert c.get_option(B.OPT_BVH_DEVICE_BUILD) == B.BVH_BUILD_SPATIAL
        c.set_option(B.OPT_BVH_DEVICE_BUILD, B.BVH_BUILD_EQUAL_COUNT)
        c.set_bvh_spheres(s)
        same_layout(c.bvh_read_layout(), B.bvh_layout_morton(s), "set back to 0")


def test_refusals_leave_the_previous_scene_in_place(pkg, sctx, start):
    B = pkg.binding
    s0, p = scenes.field(300, seed=1)
    s, _ = scenes.field(1020, seed=24)
    sctx.set_scene_bvh(s0, p)
    sctx.set_bvh_spheres(s)
    layout, before = sctx.bvh_read_layout(), shoot(pkg, sctx, start, "inline")
    bigger, _ = scenes.field(2000, seed=3)
    pos, rad, mat, tag = bigger.copy(), bigger.copy(), bigger.copy(), bigger.copy()
    pos["position"][1033, 1] = np.nan
    pos["position"][1700, 0] = np.inf                                # (the smaller index is the one named)
    rad["radius"][5] = 1e30                                          # radius^2 overflows
    mat["color"][44, 2] = np.nan
    tag["brdf_tag"][1999] = 17
    for bad, names in ((pos, "sphere 1033"), (rad, "sphere 5"), (mat, "sphere 44"), (tag, "sphere 1999")):
        with pytest.raises(B.PtmiError) as e:
            sctx.set_bvh_spheres(bad)
        assert e.value.code == B.PTMI_EINVAL and names in str(e.value), str(e.value)
        same_layout(sctx.bvh_read_layout(), layout, "after a refused set (%s)" % names)
        assert_planes_equal(shoot(pkg, sctx, start, "inline"), before, "after a refused set (%s)" % names)
    held = B._ptr(np.ascontiguousarray(s))                           # (never read: the count is refused first)
    with pytest.raises(B.PtmiError) as e:
        sctx._check(sctx._lib.ptmi_set_bvh_spheres(sctx._h, held, B.MAX_BVH_SPHERES + 1))
    assert e.value.code == B.PTMI_ELIMIT
    same_layout(sctx.bvh_read_layout(), layout, "after more spheres than the limit")
    assert_planes_equal(shoot(pkg, sctx, start, "inline"), before, "after more spheres than the limit")


TENSOR_SCRIPT = r"""
import os, sys
sys.path.insert(0, %r)
sys.path.insert(0, os.path.join(%r, "tests"))
import numpy as np
import torch
torch.cuda.set_device(0)
torch.zeros(1, device="cuda:0")                          # torch brings the HIP runtime up first: the library then shares it
import bvh_update_scenes as scenes
import bvh_spatial_scenes as spatial
pkg = scenes.pkg
W, B = pkg.world, pkg.binding
cam = W.initial_camera()

def shoot(c):
    c.resize(64, 48); c.init_output(0x5EED1234); c.render(cam, 4, 2, pkg.INLINE)
    return [np.asarray(x).view(np.uint32) for x in c.download_state()]

def words_of(s):
    return np.ascontiguousarray(s).view(np.float32).reshape(-1, 10).copy()

s0, p = scenes.field(300, seed=1)
cases = [("%%d spheres" %% n, scenes.field(n, seed=24)[0]) for n in (0, 1, 4, 5, 64, 1020, 5000)] + [("chain", spatial.chain()[0])]
with pkg.Context(0) as dev, pkg.Context(0) as fresh:
    dev.set_option(B.OPT_BVH_DEVICE_BUILD, B.BVH_BUILD_SPATIAL)
    for what, s in cases:
        dev.set_scene_bvh(s0, p)
        d = torch.from_numpy(words_of(s)).to("cuda:0").contiguous()
        odd = torch.zeros(d.numel() + 1, dtype=torch.float32, device="cuda:0")      # 4 bytes off a 16-byte boundary
        odd[1:] = d.reshape(-1)
        torch.cuda.synchronize()
        want = B.bvh_layout_spatial(s)
        fresh.set_scene_bvh(s, p)
        image = shoot(fresh)
        for tensor, how in ((d, "aligned"), (odd[1:].reshape(-1, 10), "unaligned")):
            dev.set_bvh_spheres(tensor)
            got = dev.bvh_read_layout()
            assert got[0].tobytes() == want[0].tobytes() and np.array_equal(got[1], want[1]), what + " from a device tensor, " + how
            assert all(np.array_equal(x, y) for x, y in zip(shoot(dev), image)), what + " from a device tensor: planes"
        dev.synchronize()
print("TENSOR_OK")
"""


def test_a_device_tensor_gives_what_the_host_array_gives():
    """In a process of its own, where torch brings the HIP runtime up before the library is loaded (bench.py's order): the spatial build
    from an [n, 10] device tensor, aligned and not, at every count and on the chain."""
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    res = subprocess.run([sys.executable, "-c", TENSOR_SCRIPT % (root, root)], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0 and "TENSOR_OK" in res.stdout, (res.stdout + res.stderr)[-4000:]
