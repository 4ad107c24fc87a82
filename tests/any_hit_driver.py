"""Child program of tests/test_gpu_any_hit.py (not a test module): `python tests/any_hit_driver.py WORKDIR`.

ptmi_occluded_device held to the closest hit on the device, on the trees and at the scales the hierarchies serve: Context.occluded against
`just && t < t_max` of the literal fold (bvh_rays.linear_fold, mesh_rays.linear_fold) for every family of t_max, exactly, and
Context.trace_rays against ptmi_eval_check_hit bit for bit, in a process where torch brings the HIP runtime up before the library is loaded
(the convention of tests/ray_query_driver.py).  Every case builds its scene and rays (tests/any_hit_rays.py), asserts on them what keeps
it from passing vacuously -- any_hit_rays.assert_conditions, from the fold and from the path the CPU restatement
(tests/cxx/any_hit_traverse.c) takes through the tree the device holds -- answers each query once, and is compared on the host.  One line
per case, `ok <case>` or `FAILED <case>: <why>`; a failed comparison does not end the process, a runtime error does; the last line is
ANY_HIT_DONE."""
import os
import sys
import time
import traceback

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

# (spelled out, so that the test module can name the cases without loading the library; setup() holds them to their sources)
SPHERE_SCENES = ("field x 2^-20", "field x 2^-12 + (1e3, -2e3, 5e2)", "field x 3 + (1e3, -2e3, 5e2)", "field x 2^12 + (3e5, 1e5, -7e5)", "field x 2^20",
                 "field + (1e7, 1e7, 1e7)", "radii 2^-20 .. 2^20")
MESH_FAMILIES = ("room", "needles", "slivers", "planar_grid", "coincident_grids", "multiscale", "icosphere", "mixed", "needles_1e7")
PLACEMENTS = ("room", "moved", "far")
UPDATES = ("mesh vertices to moved", "mesh vertices to far", "mesh vertices to squashed", "spheres by a wave")
DEVICE_BUILDS = ("set_bvh_spheres, equal counts", "set_bvh_spheres, spatial", "set_mesh_triangles")
LINEAR = ("mainScene", "bench scene", "reach below 2^40", "reach above 2^40")
GUARDS = ("bvh, 0 spheres and 2 planes", "bvh, 1 sphere", "mesh, 0 spheres", "mesh, 0 triangles", "mesh, zero areas alone", "bvh, 300 coincident spheres")
CASES = (["a " + s for s in SPHERE_SCENES] + ["b %s, %s" % (f, p) for f in MESH_FAMILIES for p in PLACEMENTS] + ["c " + u for u in UPDATES] +
         ["d " + b for b in DEVICE_BUILDS] + ["e " + s for s in LINEAR] + ["f " + g for g in GUARDS])
N_SPHERE_RAYS, N_MESH_RAYS, N_GUARD_RAYS = 20_000, 6000, 4096

torch = pkg = B = W = A = None
bvh_rays = mesh_rays = None
libs = alib = None


def setup(workdir):
    global torch, pkg, B, W, A, bvh_rays, mesh_rays, libs, alib
    import torch as _torch
    torch = _torch
    torch.zeros(1, device="cuda")                      # torch brings the runtime up first
    torch.cuda.synchronize()
    import __graft_entry__ as graft
    pkg = graft.load_package()
    pkg._build.build_lib()
    graft.load_oracle().build()
    B, W = pkg.binding, pkg.world
    import any_hit_rays as _a
    import bvh_rays as _b
    import mesh_rays as _m
    A, bvh_rays, mesh_rays = _a, _b, _m
    libs = (bvh_rays.traverse_lib(workdir), mesh_rays.traverse_lib(workdir))
    alib = A.any_hit_lib(workdir)
    assert len(list(A.sphere_scenes())) == len(SPHERE_SCENES) and MESH_FAMILIES == A.MESH_FAMILIES and PLACEMENTS == tuple(mesh_rays.PLACEMENTS)
    assert LINEAR == tuple(x[0] for x in A.linear_scenes())


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda")


def host(t):
    return t.cpu().numpy()


def bits(a):
    return np.asarray(a).view(np.uint32)


def compare(case, c, conditions=True):
    """The conditions on the case's own inputs, then the two comparisons, each query answered once on the context's own stream"""
    if case.kind == "linear":
        restated, path, _ = case.walk(alib)
    else:                                              # the path through the tree the device holds, however it was built
        restated, path, _ = case.walk(alib, sphere_tree=c.bvh_read_layout() if len(case.spheres) else None,
                                      triangle_tree=c.mesh_read_layout() if case.kind == "mesh" and len(case.triangles) else None)
    if conditions:
        A.assert_conditions(case, path)
    d_rays, d_t_max = dev(case.rays), dev(case.t_max)
    torch.cuda.synchronize()
    occ, (t, idx) = c.occluded(d_rays, d_t_max), c.trace_rays(d_rays)
    c.synchronize()
    got, t, idx = host(occ), host(t), host(idx)
    bad = case.wrong(got)
    assert bad.size == 0, "occluded: %d rays differ, e.g. %s; the restatement says %d by path '%s'" % (
        bad.size, case.describe(bad[0], got[bad[0]]), restated[bad[0]], A.PATHS[path[bad[0]]])
    e_t, e_idx, _ = c.eval_check_hit(case.rays)
    bad = np.flatnonzero((bits(t) != bits(e_t)) | (idx != e_idx))
    assert bad.size == 0, "trace_rays: %d rays differ from ptmi_eval_check_hit, e.g. ray %d: (%r, %d), expected (%r, %d)" % (
        bad.size, bad[0], t[bad[0]], idx[bad[0]], e_t[bad[0]], e_idx[bad[0]])
    bad = case.wrong(restated)
    assert bad.size == 0, "the restatement: %d rays differ, e.g. %s" % (bad.size, case.describe(bad[0], restated[bad[0]]))


# ---- the cases ---------------------------------------------------------------------------------------------------------------------

def sphere_case(name, s, p):
    return A.Case(name, "bvh", s, p, A.sphere_rays(s, N_SPHERE_RAYS), libs)


def mesh_case(name, scene, family, seed):
    s, t, p = scene
    return A.Case(name, "mesh", s, p, A.mesh_case_rays(family, scene, N_MESH_RAYS, seed, libs[1]), libs, triangles=t)


def cases_a():
    """a: sphere hierarchies beyond the field -- test_mesh_exact.bvh_cases()"""
    for name, (_, (s, p)) in zip(SPHERE_SCENES, A.sphere_scenes()):
        def run(s=s, p=p, name=name):
            with pkg.Context(0) as c:
                c.set_scene_bvh(s, p)
                compare(sphere_case(name, s, p), c)
        yield "a " + name, run


def cases_b():
    """b: mesh families by placement"""
    for family in MESH_FAMILIES:
        for placement in PLACEMENTS:
            def run(family=family, placement=placement):
                scene = mesh_rays.placed(family, placement, seed=1)
                with pkg.Context(0) as c:
                    c.set_scene_mesh(*scene)
                    compare(mesh_case("%s, %s" % (family, placement), scene, "needles" if family == "needles_1e7" else family, 5), c)
            yield "b %s, %s" % (family, placement), run


def cases_c():
    """c: trees no build produced -- after update_mesh_vertices and update_spheres, against the fold of the NEW geometry"""
    for target in ("moved", "far", "squashed"):
        def run(target=target):
            s, t, p = mesh_rays.placed("room", "room", seed=1)
            t2 = A.squashed(t) if target == "squashed" else mesh_rays.placed("room", target, seed=1)[1]
            with pkg.Context(0) as c:
                c.set_scene_mesh(s, t, p)
                c.update_mesh_vertices(W.triangle_vertices(t2))
                assert c.mesh_read_layout()[0].tobytes() == B.mesh_refit_layout(t2, *B.mesh_layout(t)).tobytes(), "not the refitted tree"
                compare(mesh_case("room refitted to " + target, (s, t2, p), "room", 11), c)
        yield "c mesh vertices to " + target, run

    def wave():
        s, p = bvh_rays.adversarial_scene(1500, seed=4)
        g, moved = A.moved_spheres(s)
        with pkg.Context(0) as c:
            c.set_scene_bvh(s, p)
            c.update_spheres(g)
            nodes, order = B.bvh_layout(s)
            assert c.bvh_read_layout()[0].tobytes() == B.bvh_refit_layout(moved, nodes, order).tobytes(), "not the refitted tree"
            compare(sphere_case("field after a wave of 0.5", moved, p), c)
    yield "c spheres by a wave", wave


def cases_d():
    """d: device-built trees -- a field of 3 000 spheres under both builds, the room at subdivision 3"""
    for name, build in (("equal counts", "BVH_BUILD_EQUAL_COUNT"), ("spatial", "BVH_BUILD_SPATIAL")):
        def run(build=build):
            s, p = bvh_rays.adversarial_scene(3000, seed=6)
            other = bvh_rays.adversarial_scene(40, seed=7)[0]
            with pkg.Context(0) as c:
                before = c.get_option(B.OPT_BVH_DEVICE_BUILD)
                try:
                    c.set_option(B.OPT_BVH_DEVICE_BUILD, getattr(B, build))
                    c.set_scene_bvh(other, p)
                    c.set_bvh_spheres(s)
                    want = (B.bvh_layout_spatial if build == "BVH_BUILD_SPATIAL" else B.bvh_layout_morton)(s)
                    assert c.bvh_read_layout()[0].tobytes() == want[0].tobytes(), "not the device build's tree"
                    compare(sphere_case("3 000 spheres, " + build, s, p), c)
                finally:
                    c.set_option(B.OPT_BVH_DEVICE_BUILD, before)
        yield "d set_bvh_spheres, " + name, run

    def triangles():
        s, t, p = mesh_rays.adversarial_scene(3, seed=2)
        with pkg.Context(0) as c:
            c.set_scene_mesh(s, mesh_rays.adversarial_scene(0, seed=1)[1], p)
            c.set_mesh_triangles(t)
            assert c.mesh_read_layout()[0].tobytes() == B.mesh_layout_morton(t)[0].tobytes(), "not the device build's tree"
            compare(mesh_case("room at subdivision 3, set_mesh_triangles", (s, t, p), None, 3), c)
    yield "d set_mesh_triangles", triangles


def cases_e():
    """e: linear scenes, sphere_reach on either side of its limit"""
    for name, s, p, served_at_all in A.linear_scenes():
        def run(name=name, s=s, p=p, served_at_all=served_at_all):
            rays = np.concatenate([bvh_rays.adversarial_rays(s, N_SPHERE_RAYS // 2, seed=8), bvh_rays.admission_rays(s, N_SPHERE_RAYS // 2, seed=8)])
            case = A.Case(name, "linear", s, p, rays, libs)
            if not served_at_all:
                path = case.walk(alib)[1]
                assert (path == A.NOT_SERVED).all() and case.want.sum() >= len(rays) // 100, "sphere_reach does not refuse the scene"
            with pkg.Context(0) as c:
                c.set_scene(s, p)
                compare(case, c, conditions=served_at_all)
        yield "e " + name, run


def guard_rays(aim):
    """4 096 rays about the spheres `aim`: adversarial rays, admission-bracket rays and rays that leave the scene (a scene of a few
    primitives must still hold every family of t_max for misses), the non-finite four of ray_query_driver.py at the end"""
    k = 3 * N_GUARD_RAYS // 8
    c = np.asarray(aim)["position"].astype(np.float64)
    rays = np.concatenate([bvh_rays.adversarial_rays(aim, k, seed=9), bvh_rays.admission_rays(aim, k, seed=9)])
    rays = A.with_misses(rays, c.min(0) - 1.0, c.max(0) + 1.0, N_GUARD_RAYS - 2 * k, seed=9)
    rays[-4:] = [[np.nan, 0, 0, 0, 1, 0], [1, 0, -5, 0, np.inf, 0], [np.inf, 1, 2, 0, 0, -1], [1, 0, -5, 0, 0, 0]]
    assert rays.shape == (N_GUARD_RAYS, 6)
    return rays


def cases_f():
    """f: the guards -- ns > 0, M.n_kept > 0 -- and full leaves of ties"""
    field, planes = W.sphere_field(8, seed=3)
    room_s, room_t, _ = mesh_rays.adversarial_scene(0, seed=1)
    flat = room_t[:50].copy()
    flat["v2"] = flat["v1"]
    one = field[:1]
    table = (("bvh, 0 spheres and 2 planes", "bvh", field[:0], planes[:2], None, field),
             ("bvh, 1 sphere", "bvh", one, planes, None, one),
             ("mesh, 0 spheres", "mesh", field[:0], planes[:1], room_t, field),
             ("mesh, 0 triangles", "mesh", field, planes, room_t[:0], field),
             ("mesh, zero areas alone", "mesh", field, planes, flat, field),
             ("bvh, 300 coincident spheres", "bvh", np.concatenate([field[3:4]] * 300), planes, None, field))
    for name, kind, s, p, t, aim in table:
        def run(name=name, kind=kind, s=s, p=p, t=t, aim=aim):
            case = A.Case(name, kind, s, p, guard_rays(aim), libs, triangles=t)
            with pkg.Context(0) as c:
                if kind == "mesh":
                    c.set_scene_mesh(s, t, p)
                    kept = len(c.mesh_read_layout()[1]) if len(t) else 0
                    assert kept == (len(t) - 5 if name == "mesh, 0 spheres" else 0), "n_kept is not what the case is about"
                else:
                    c.set_scene_bvh(s, p)
                compare(case, c)
        yield "f " + name, run


def main():
    setup(sys.argv[1])
    runs = [x for make in (cases_a, cases_b, cases_c, cases_d, cases_e, cases_f) for x in make()]
    assert [name for name, _ in runs] == CASES
    for name, run in runs:
        t0 = time.perf_counter()
        try:
            run()
            print("ok %s" % name, flush=True)
        except AssertionError as e:
            print("FAILED %s: %s" % (name, str(e).replace("\n", " ")[:1500] or traceback.format_exc()[-1500:].replace("\n", " | ")), flush=True)
        except B.PtmiError as e:                     # a runtime error: nothing more is started on the device
            print("FAILED %s: %s" % (name, e), flush=True)
            raise SystemExit(3)
        print("   %.1f s" % (time.perf_counter() - t0), flush=True)
    print("ANY_HIT_DONE", flush=True)


if __name__ == "__main__":
    main()
