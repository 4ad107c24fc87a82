"""Driver of tests/test_mesh_build_host_sanitized.py (a CHILD process with the HIP stand-in and the sanitizer runtime preloaded; not a
test module): tests/hostsan_driver.py's walk -- plainly, then with every k-th allocation / copy / launch / synchronise failing -- over
one scenario, the calls that give a mesh scene new triangles.  Kernels do not run on the stand-in: the check kernel's kept count is
placed into its read-back (hipstub_poke), so that the sort, the order, the scatter and every level of the hierarchy are launched."""
import ctypes
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hostsan_driver as D  # noqa: E402

pkg, B, W = D.pkg, D.B, D.pkg.world
KEPT_AT = 7 * 4                                                     # kBuildKept (csrc/ptmi_mesh_morton.h), in bytes
CHECK = b"mesh_build_check_kernel"


def refuses(call, code):
    try:
        call()
    except B.PtmiError as e:
        assert e.code == code or not D.PLAIN, e
        return
    raise AssertionError("a refusal was expected")


def mesh_build():
    s, t, _ = W.mesh_room(2)
    p = np.array([W.plane((0.0, -2.5, 0.0), (0.0, 1.0, 0.0), (0.6, 0.8, 0.6), 0.0, W.MATTE, 0.9)], dtype=W.PLANE_DTYPE)
    t3 = W.mesh_room(3)[1]
    flat = t3[[20]].copy()
    flat["v2"] = flat["v1"]
    t3 = np.concatenate([t3, flat])
    count = lambda name: D.stub.hipstub_launches(name)             # noqa: E731
    D.stub.hipstub_clear_pokes()
    try:
        with pkg.Context(0) as ctx:
            ctx.set_scene_mesh(s, t, p)
            ctx.resize(72, 40)
            ctx.init_output(3)
            ctx.render(D.cam, 8, 2)
            try:
                before = count(b"mesh_build_sort_scatter_kernel"), count(b"mesh_refit_level_kernel")
                D.stub.hipstub_poke(CHECK, 1, KEPT_AT, len(t3) - 1)
                ctx.set_mesh_triangles(t3)                               # from host memory: more triangles
                if D.PLAIN:
                    assert count(b"mesh_build_sort_scatter_kernel") - before[0] == 6 and count(b"mesh_refit_level_kernel") - before[1] >= 8
                    nodes, order = ctx.mesh_read_layout()
                    assert len(order) == len(t3) - 1 and len(nodes) == len(B.mesh_layout_morton(t3)[0])
                ctx.render(D.cam, 8, 1)
                ctx.update_mesh_vertices(W.triangle_vertices(t3))         # the refit over the fresh plan
                with D.DeviceBlocks([t.nbytes]) as (dt,):                 # from a stand-in device block: fewer triangles
                    try:
                        if D.stub.hipMemcpy(ctypes.c_void_p(dt), t.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(t.nbytes), 1) != 0:
                            D.stub.hipstub_clear_error()
                            raise MemoryError("stand-in hipMemcpy (injected)")
                        D.stub.hipstub_poke(CHECK, 1, KEPT_AT, len(t))
                        ctx._check(ctx._lib.ptmi_set_mesh_triangles_device(ctx._h, ctypes.c_void_p(dt), len(t)))
                        ctx.render(D.cam, 8, 1, pkg.STREAMS)
                    finally:
                        D.quiet(ctx.synchronize)
                ctx.set_mesh_triangles(t3[:5])                            # (nothing counted: no triangle is in a leaf)
                ctx.set_mesh_triangles(t3[:0])
                ctx.render(D.cam, 8, 1)
                refuses(lambda: ctx._check(ctx._lib.ptmi_set_mesh_triangles(ctx._h, None, 4)), B.PTMI_EINVAL)
                refuses(lambda: ctx._check(ctx._lib.ptmi_set_mesh_triangles(ctx._h, B._ptr(t), -1)), B.PTMI_EINVAL)
                refuses(lambda: ctx._check(ctx._lib.ptmi_set_mesh_triangles(ctx._h, B._ptr(t), (1 << 22) + 1)), B.PTMI_ELIMIT)
                D.stub.hipstub_poke(CHECK, 1, 0, (77 << 2) | 1)          # the check kernel's verdict: triangle 77, its material
                refuses(lambda: ctx.set_mesh_triangles(t), B.PTMI_EINVAL)
                ctx.mesh_read_layout()
            except (B.PtmiError, MemoryError):
                # after an injected failure inside a build the context is used again: the scene it holds is whole
                for k in range(6):
                    D.stub.hipstub_fail(k, 0)
                D.stub.hipstub_clear_error()
                D.stub.hipstub_clear_pokes()
                n = ctx._lib.ptmi_mesh_read_layout(ctx._h, None, 0, None, None)
                assert n >= 1
                ctx.render(D.cam, 8, 1)
                ctx.mesh_read_layout()
                ctx.set_mesh_triangles(t)
                ctx.render(D.cam, 8, 1)
                ctx.download_color()
                raise
            ctx.set_scene(*W.scene16())                                   # a scene that is no mesh scene
            refuses(lambda: ctx.set_mesh_triangles(t), B.PTMI_ESTATE)
            ctx.render(D.cam, 8, 1)
        with pkg.Group([0, 0], 8) as g:
            g.set_scene_mesh(s, t, p)
            g.resize(48, 32)
            g.init_output(1)
            g.set_mesh_triangles(t3)
            g.render(D.cam, 8, 1)
            g.download_color()
            refuses(lambda: g._check(g._lib.ptmi_group_set_mesh_triangles(g._h, None, 3)), B.PTMI_EINVAL)
            g.member(1).mesh_read_layout()
    finally:
        D.stub.hipstub_clear_pokes()


D.SCENARIOS = [mesh_build]

if __name__ == "__main__":
    D.main()
