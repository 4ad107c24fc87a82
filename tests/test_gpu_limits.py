"""The hierarchies at their limits and past every builder threshold, on the device, on the scenes of tests/limit_scenes.py -- a lit room
of mirrors with a few dozen spheres and a small icosphere in it, and up to 2^22 spheres and 2^22 triangles of ballast so far outside that
the room's own scene (the core) is a bit-exact reference:
  * ptmi_set_scene_bvh with exactly PTMI_MAX_BVH_SPHERES spheres and 64 planes, the core spheres last and at both ends, and
    ptmi_set_scene_mesh with PTMI_MAX_MESH_TRIANGLES triangles besides: render Inline, the Streams chain under both seed rules and the
    GLASS tree walk (whose start records hold a primitive index of 24 bits: here all of them are in use) equal the oracle's renders of the
    core scene on all seven planes, ptmi_eval_check_hit equals the core scene's literal fold with the index mapped; one primitive more is
    refused and the scene stays;
  * the device builders (ptmi_set_bvh_spheres under both PTMI_OPT_BVH_DEVICE_BUILD values, ptmi_set_mesh_triangles) and the refits behind
    them at the counts at which the check kernels walk a second chunk, the spatial numbering sums the workgroups before it in two trips,
    and at 2^22: the trees read back equal the host twins bit for bit;
  * refusals that a check kernel finds in a later pass of its chunk loop: the smallest bad index is the one named, the scene stays.
Every comparison is bitwise or an exact count.  64 x 48, 2 samples, bounce limit 4."""
import os
import sys
import time

import numpy as np
import pytest

from conftest import assert_planes_equal, initial_planes

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bvh_rays  # noqa: E402
import limit_scenes as limits  # noqa: E402
import mesh_rays  # noqa: E402

pytestmark = pytest.mark.gpu
W = limits.world
CAP = 1 << 16                                  # the default step cap of render Streams
THREADS = max(1, min(16, os.cpu_count() or 1))
WIDTH, HEIGHT, SPP, LIMIT = 64, 48, 2, 4
N_RAYS = 20_000
CHUNK, PASS = 256, 512 * 256                   # a check kernel's chunk, and the records its 512 workgroups take in one pass
SPATIAL_WIDE_COUNT, WIDE_LEVEL = limits.SPATIAL_WIDE_COUNT, limits.WIDE_LEVEL
COUNTS = (PASS, PASS + 1, 2 * PASS + 257, SPATIAL_WIDE_COUNT, 1 << 22)
RENDER_AND_HITS_AT = (PASS + 1, 1 << 22)


@pytest.fixture(scope="module")
def trav(tmp_path_factory):
    return bvh_rays.traverse_lib(tmp_path_factory.mktemp("limitbvh"))


@pytest.fixture(scope="module")
def mtrav(tmp_path_factory):
    return mesh_rays.traverse_lib(tmp_path_factory.mktemp("limitmesh"))


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return mesh_rays.reference_lib(tmp_path_factory.mktemp("limitref"))


@pytest.fixture(scope="module")
def fresh(pkg):
    c = pkg.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def bctx(pkg):
    """a context of this module's own for the device builders (its PTMI_OPT_BVH_DEVICE_BUILD changes)"""
    c = pkg.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def start(ora):
    return initial_planes(ora, WIDTH, HEIGHT)


@pytest.fixture(scope="module")
def planes():
    return limits.planes()


def shoot(pkg, c, start, case):
    B = pkg.binding
    algorithm = pkg.INLINE if case == "inline" else pkg.STREAMS
    rule = {"streams_keep": B.SEED_KEEP_ACCUMULATOR, "streams_from_result": B.SEED_FROM_RESULT}.get(case, B.SEED_AUTO)
    c.set_option(B.OPT_STREAMS_SEED_RULE, rule)
    try:
        c.resize(WIDTH, HEIGHT)
        c.upload_state(*start)
        c.render(W.initial_camera(), LIMIT, SPP, algorithm)
        return c.download_state()
    finally:
        c.set_option(B.OPT_STREAMS_SEED_RULE, B.SEED_AUTO)


def oracle_render(o, s, p, start, case):
    """the oracle module (or a MeshOracle's) on the core scene"""
    cam = W.initial_camera()
    if case == "inline":
        return o.render_inline(s, p, cam, WIDTH, HEIGHT, LIMIT, SPP, start, n_threads=THREADS)[0]
    if case == "glass_tree":
        return o.render_streams_tree(s, p, cam, WIDTH, HEIGHT, CAP, SPP, start, n_threads=THREADS)[0]
    rule = {"streams_keep": o.SEED_KEEP_ACCUMULATOR, "streams_from_result": o.SEED_FROM_RESULT}[case]
    return o.render_streams(s, p, cam, WIDTH, HEIGHT, CAP, SPP, start, seed_rule=rule, n_threads=THREADS)[0]


def lit(image):
    return float(np.mean(np.asarray(image[0]) != 0))


def same_hits(got, want, what):
    """t as a number (tests/test_gpu_bvh.py: a NaN key's sign and the zero of a ray that starts on a sphere are encodings), idx and just exactly"""
    (t0, i0, j0), (t1, i1, j1) = got, want
    same_t = (t0 == t1) | (np.isnan(t0) & np.isnan(t1))
    bad = np.flatnonzero(~same_t | (i0 != i1) | (j0 != j1))
    assert bad.size == 0, "%s: %d of %d rays differ, e.g. ray %d: device (%r, %d, %d), the core fold (%r, %d, %d)" % (
        what, bad.size, len(t0), bad[0], t0[bad[0]], i0[bad[0]], j0[bad[0]], t1[bad[0]], i1[bad[0]], j1[bad[0]])


def same_bits(got, want, what):
    for a, b, name in zip(got, want, ("t", "idx", "just")):
        bad = np.flatnonzero(np.asarray(a).view(np.uint32) != np.asarray(b).view(np.uint32))
        assert bad.size == 0, "%s: %s of ptmi_eval_check_hit differs for %d rays, first %d" % (what, name, bad.size, bad[0])


def same_layout(got, want, what):
    assert len(got[0]) == len(want[0]), "%s: %d nodes, the twin has %d" % (what, len(got[0]), len(want[0]))
    assert got[0].tobytes() == want[0].tobytes(), "%s: the nodes differ" % what
    assert np.array_equal(got[1], want[1]), "%s: the leaf order differs" % what


# ---- a. the sphere limit ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ordering", ["last", "ends"])
def test_the_sphere_limit_renders_and_hits_as_the_core_scene(ctx, pkg, ora, trav, start, planes, ordering):
    B = pkg.binding
    n = B.MAX_BVH_SPHERES
    began = time.time()
    full, core, index = limits.spheres(n, ordering, glass=False)
    full_g, core_g, _ = limits.spheres(n, ordering, glass=True)
    assert len(full) == n and len(planes) == B.MAX_BVH_PLANES
    limits.premise_holds(full, index)
    print("two scenes of %d spheres: %.1f s" % (n, time.time() - began))
    began = time.time()
    ctx.set_scene_bvh(full, planes)
    print("ptmi_set_scene_bvh: %.1f s" % (time.time() - began))
    for case in ("inline", "streams_keep", "streams_from_result"):
        want = oracle_render(ora, core, planes, start, case)
        assert_planes_equal(shoot(pkg, ctx, start, case), want, "%d spheres, the core %s, %s" % (n, ordering, case))
        assert lit(want) > 0.9
    ctx.set_scene_bvh(full_g, planes)
    want = oracle_render(ora, core_g, planes, start, "glass_tree")
    assert_planes_equal(shoot(pkg, ctx, start, "glass_tree"), want, "%d spheres, the core %s, the GLASS tree walk" % (n, ordering))
    assert not np.array_equal(want[0], oracle_render(ora, core, planes, start, "streams_keep")[0]), "no GLASS in sight"
    # checkHit
    rays = limits.sphere_rays(core_g, N_RAYS, seed=41)
    sizes = ((len(core_g), len(planes)), (n, len(planes)))
    t, idx, just = bvh_rays.linear_fold(trav, core_g, planes, rays)
    want = (t, limits.map_index(idx, *sizes, index), just)
    got = ctx.eval_check_hit(rays)
    same_hits(got, want, "%d spheres, the core %s" % (n, ordering))
    top = np.arange(n - (len(core_g) - (len(core_g) // 2 if ordering == "ends" else 0)), n)
    assert np.array_equal(index[-len(top):], top)
    on_top, on_planes = int(np.sum((got[2] == 1) & (got[1] >= top[0]) & (got[1] < n))), int(np.sum((got[2] == 1) & (got[1] >= n)))
    print("%d rays hit the top-index spheres, %d a plane" % (on_top, on_planes))
    assert on_top > 1000 and on_planes > 0
    if ordering == "ends":
        assert int(np.sum((got[2] == 1) & (got[1] < len(core_g) // 2))) > 1000          # ... and the lowest ones
    # the premise on the data itself: the full literal fold, 256 rays
    began = time.time()
    few = np.arange(0, N_RAYS, N_RAYS // 256)[:256]
    folded = limits.in_slices(lambda r: bvh_rays.linear_fold(trav, full_g, planes, r), rays[few])
    same_bits(folded, tuple(a[few] for a in want), "the literal fold over %d spheres" % n)
    print("the literal fold of 256 rays: %.1f s" % (time.time() - began))
    # one sphere more
    with pytest.raises(B.PtmiError) as e:
        ctx.set_scene_bvh(np.concatenate([full_g, full_g[:1]]), planes)
    assert e.value.code == B.PTMI_ELIMIT
    same_bits(ctx.eval_check_hit(rays), got, "after one sphere too many")
    assert_planes_equal(shoot(pkg, ctx, start, "glass_tree"), oracle_render(ora, core_g, planes, start, "glass_tree"), "after one sphere too many")


# ---- b. the mesh limit -----------------------------------------------------------------------------------------------------------------
def test_the_mesh_limit_renders_and_hits_as_the_core_scene(ctx, pkg, ora, mtrav, ref, start, planes):
    B = pkg.binding
    ns, nt = B.MAX_BVH_SPHERES, B.MAX_MESH_TRIANGLES
    began = time.time()
    s, s_core, s_index = limits.spheres(ns, "last", glass=False)
    t, t_core, t_index = limits.triangles(nt, "last", glass=False)
    t_g, t_core_g, _ = limits.triangles(nt, "last", glass=True)
    assert len(s) == ns and len(t) == nt and len(planes) == B.MAX_BVH_PLANES
    limits.premise_holds(s, s_index, t, t_index)
    first = ns + len(planes)                                              # the fold index of triangle 0
    high = np.flatnonzero(first + t_index >= 1 << 23)
    glass_high = high[t_core_g["brdf_tag"][high] == W.GLASS]
    assert len(high) == 64 and len(glass_high) == 16
    print("the scenes of %d spheres and %d triangles: %.1f s" % (ns, nt, time.time() - began))
    began = time.time()
    ctx.set_scene_mesh(s, t, planes)
    print("ptmi_set_scene_mesh: %.1f s" % (time.time() - began))
    with mesh_rays.MeshOracle(ref, t_core) as mo:
        for case in ("inline", "streams_keep", "streams_from_result"):
            want = oracle_render(mo, s_core, planes, start, case)
            assert_planes_equal(shoot(pkg, ctx, start, case), want, "the mesh limit, %s" % case)
            assert lit(want) > 0.9
        plain = oracle_render(mo, s_core, planes, start, "streams_keep")
    ctx.set_scene_mesh(s, t_g, planes)
    with mesh_rays.MeshOracle(ref, t_core_g) as mo:
        want = oracle_render(mo, s_core, planes, start, "glass_tree")
    assert_planes_equal(shoot(pkg, ctx, start, "glass_tree"), want, "the mesh limit, the GLASS tree walk")
    assert not np.array_equal(want[0], plain[0]), "no GLASS in sight"
    # the camera sees GLASS triangles whose fold index is 2^23 or more: start records with bit 23 of the primitive field set
    _, idx, just = ctx.eval_check_hit(limits.camera_rays_at(t_core_g[glass_high]))
    assert int(np.sum((just == 1) & (idx == first + t_index[glass_high]))) >= 12
    # checkHit
    rays = limits.mesh_rays_for(s_core, t_core_g, N_RAYS, seed=43)
    sizes = ((len(s_core), len(planes)), (ns, len(planes)))
    ft, fidx, fjust = mesh_rays.linear_fold(mtrav, s_core, t_core_g, planes, rays)
    want = (ft, limits.map_index(fidx, *sizes, s_index, t_index), fjust)
    got = ctx.eval_check_hit(rays)
    same_hits(got, want, "the mesh limit")
    on_high = int(np.sum((got[2] == 1) & (got[1] >= 1 << 23)))
    on_spheres = int(np.sum((got[2] == 1) & (got[1] >= ns - len(s_core)) & (got[1] < ns)))
    print("%d rays hit triangles whose fold index is 2^23 or more, %d the top-index spheres" % (on_high, on_spheres))
    assert on_high > 500 and on_spheres > 1000
    # the premise on the data itself: the full literal fold, 256 rays
    began = time.time()
    few = np.arange(0, N_RAYS, N_RAYS // 256)[:256]
    folded = limits.mesh_fold_in_slices(mtrav, s, t_g, planes, rays[few])
    same_bits(folded, tuple(a[few] for a in want), "the literal fold over the mesh limit")
    print("the literal fold of 256 rays: %.1f s" % (time.time() - began))
    # one triangle more
    with pytest.raises(B.PtmiError) as e:
        ctx.set_scene_mesh(s, np.concatenate([t_g, t_g[:1]]), planes)
    assert e.value.code == B.PTMI_ELIMIT
    with pytest.raises(B.PtmiError) as e:
        ctx.set_mesh_triangles(np.concatenate([t_g, t_g[:1]]))
    assert e.value.code == B.PTMI_ELIMIT
    same_bits(ctx.eval_check_hit(rays), got, "after one triangle too many")
    assert_planes_equal(shoot(pkg, ctx, start, "glass_tree"), want_tree(ref, s_core, t_core_g, planes, start), "after one triangle too many")


def want_tree(ref, s_core, t_core, planes, start):
    with mesh_rays.MeshOracle(ref, t_core) as mo:
        return oracle_render(mo, s_core, planes, start, "glass_tree")


# ---- c. the device builders past their thresholds --------------------------------------------------------------------------------------
def waved(x, amount, seed):
    """positions (any shape ending in 3) moved along y by a wave over x and z"""
    p = np.asarray(x, np.float64).copy()
    p[..., 1] += amount * np.sin(0.7 * p[..., 0] + 0.9 * seed) * np.cos(0.5 * p[..., 2])
    return p.astype(np.float32)


@pytest.mark.parametrize("n", COUNTS)
def test_the_device_builders_and_refits_equal_the_host_twins(bctx, fresh, pkg, start, planes, n):
    B = pkg.binding
    began = time.time()
    s = limits.spheres(n, "last", glass=False)[0]
    t = limits.triangles(n, "last", glass=False)[0]
    s2 = s.copy()
    s2["position"] = waved(s["position"], 0.5, 3)
    v2 = waved(W.triangle_vertices(t), 0.25, 5)
    t2 = W.with_vertices(t, v2)
    print("the scenes of %d: %.1f s" % (n, time.time() - began))
    bctx.set_scene_mesh(limits.core_spheres(False), limits.core_triangles(False), planes)
    try:
        for option, twin in ((B.BVH_BUILD_EQUAL_COUNT, B.bvh_layout_morton), (B.BVH_BUILD_SPATIAL, B.bvh_layout_spatial)):
            bctx.set_option(B.OPT_BVH_DEVICE_BUILD, option)
            want = twin(s)
            bctx.set_bvh_spheres(s)
            got = bctx.bvh_read_layout()
            same_layout(got, want, "%d spheres built, option %d" % (n, option))
            if option == B.BVH_BUILD_SPATIAL and n == SPATIAL_WIDE_COUNT:
                assert max(limits.level_counts(got[0])) >= WIDE_LEVEL
            bctx.update_spheres(W.sphere_geometry(s2))
            refitted = B.bvh_refit_layout(s2, *want)
            assert refitted.tobytes() != want[0].tobytes()
            same_layout(bctx.bvh_read_layout(), (refitted, want[1]), "%d spheres built, option %d, then refitted" % (n, option))
    finally:
        bctx.set_option(B.OPT_BVH_DEVICE_BUILD, B.BVH_BUILD_EQUAL_COUNT)
    want = B.mesh_layout_morton(t)
    bctx.set_mesh_triangles(t)
    same_layout(bctx.mesh_read_layout(), want, "%d triangles built" % n)
    if n in RENDER_AND_HITS_AT:
        # spheres moved on a spatial tree, triangles built: against a scene set afresh
        fresh.set_scene_mesh(s2, t, planes)
        assert_planes_equal(shoot(pkg, bctx, start, "inline"), shoot(pkg, fresh, start, "inline"), "%d built, Inline" % n)
        rays = limits.mesh_rays_for(limits.core_spheres(False), limits.core_triangles(False), N_RAYS, seed=45)
        same_bits(bctx.eval_check_hit(rays), fresh.eval_check_hit(rays), "%d built" % n)
    bctx.update_mesh_vertices(v2)
    refitted = B.mesh_refit_layout(t2, *want)
    assert refitted.tobytes() != want[0].tobytes()
    same_layout(bctx.mesh_read_layout(), (refitted, want[1]), "%d triangles built, then refitted" % n)
    if n in RENDER_AND_HITS_AT:
        fresh.set_mesh_triangles(t2)
        assert_planes_equal(shoot(pkg, bctx, start, "inline"), shoot(pkg, fresh, start, "inline"), "%d built and refitted, Inline" % n)


# ---- d. refusals from a later pass of a check kernel -----------------------------------------------------------------------------------
def test_a_check_kernels_later_passes_name_the_smallest_bad_index_and_leave_the_scene(ctx, pkg, ref, start, planes):
    B = pkg.binding
    n = 3 * PASS + 77
    second = PASS + 5                              # workgroup 0's second chunk
    third = (2 * 512 + 37) * CHUNK + 9             # workgroup 37's third chunk
    last = n - 5                                   # the last, partial chunk: workgroup 0's fourth
    assert second // CHUNK == 512 and third // CHUNK % 512 == 37 and third // CHUNK // 512 == 2 and last // CHUNK == n // CHUNK == 3 * 512
    s, s_core, _ = limits.spheres(n, "last", glass=False)
    t, t_core, _ = limits.triangles(n, "last", glass=False)
    ctx.set_scene_mesh(s, t, planes)
    before = shoot(pkg, ctx, start, "inline")
    with mesh_rays.MeshOracle(ref, t_core) as mo:
        assert_planes_equal(before, oracle_render(mo, s_core, planes, start, "inline"), "%d spheres and triangles, Inline" % n)
    assert lit(before) > 0.9
    layouts = ctx.bvh_read_layout(), ctx.mesh_read_layout()
    g, v = W.sphere_geometry(s), W.triangle_vertices(t)

    def spoiled(kind, where):
        """the argument of call `kind` with a non-finite record at every index of `where`, a NaN at the first and an infinity behind"""
        values = [np.nan] + [np.inf] * (len(where) - 1)
        if kind == "update_spheres":
            bad = g.copy()
            for i, x in zip(where, values):
                bad[i, 1] = x
        elif kind == "set_bvh_spheres":
            bad = s.copy()
            for i, x in zip(where, values):
                bad["color"][i, 2] = x
        elif kind == "set_mesh_triangles":
            bad = t.copy()
            for i, x in zip(where, values):
                bad["v1"][i, 0] = x
        else:
            bad = v.copy()
            for i, x in zip(where, values):
                bad[i, 2, 1] = x
        return bad

    for kind, noun in (("update_spheres", "sphere"), ("set_bvh_spheres", "sphere"), ("set_mesh_triangles", "triangle"), ("update_mesh_vertices", "triangle")):
        for where in ((second, third), (third, last), (last,)):
            with pytest.raises(B.PtmiError) as e:
                getattr(ctx, kind)(spoiled(kind, where))
            text = str(e.value)
            assert e.value.code == B.PTMI_EINVAL and ("%s %d" % (noun, where[0])) in text, text
            same_layout(ctx.bvh_read_layout(), layouts[0], "the spheres after a refused %s" % kind)
            same_layout(ctx.mesh_read_layout(), layouts[1], "the triangles after a refused %s" % kind)
            assert_planes_equal(shoot(pkg, ctx, start, "inline"), before, "after a refused %s (%s %d)" % (kind, noun, where[0]))
    # ... and what they refuse they would have taken
    ctx.update_spheres(g)
    ctx.update_mesh_vertices(v)
    assert_planes_equal(shoot(pkg, ctx, start, "inline"), before, "after an accepted update")
