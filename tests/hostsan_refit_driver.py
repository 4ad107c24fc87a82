"""Driver of tests/test_mesh_refit_host_sanitized.py (a CHILD process with the HIP stand-in and the sanitizer runtime preloaded; not a
test module): tests/hostsan_driver.py's walk -- plainly, then with every k-th allocation / copy / launch / synchronise failing -- over
one scenario, the calls that move a mesh scene's vertices."""
import ctypes
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hostsan_driver as D  # noqa: E402

pkg, B, W = D.pkg, D.B, D.pkg.world


def refuses(call, code):
    try:
        call()
    except B.PtmiError as e:
        assert e.code == code or not D.PLAIN, e
        return
    raise AssertionError("a refusal was expected")


def mesh_refit():
    s, t, _ = W.mesh_room(2)
    p = np.array([W.plane((0.0, -2.5, 0.0), (0.0, 1.0, 0.0), (0.6, 0.8, 0.6), 0.0, W.MATTE, 0.9)], dtype=W.PLANE_DTYPE)
    flat = t[[20]].copy()
    flat["v2"] = flat["v1"]
    t = np.concatenate([t, flat])
    v = W.triangle_vertices(t)
    v2 = W.displaced(v, 0.1, "wave")
    with pkg.Context(0) as ctx:
        ctx.set_scene_mesh(s, t, p)
        ctx.resize(72, 40)
        ctx.init_output(3)
        ctx.render(D.cam, 8, 2)
        try:
            ctx.update_mesh_vertices(v2)                          # from host memory
            ctx.render(D.cam, 8, 1)
            with D.DeviceBlocks([v2.nbytes]) as (dv,):            # from a stand-in device block
                try:
                    if D.stub.hipMemcpy(ctypes.c_void_p(dv), v.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(v.nbytes), 1) != 0:
                        D.stub.hipstub_clear_error()
                        raise MemoryError("stand-in hipMemcpy (injected)")
                    ctx._check(ctx._lib.ptmi_update_mesh_vertices_device(ctx._h, ctypes.c_void_p(dv), len(t)))
                    ctx.render(D.cam, 8, 1, pkg.STREAMS)
                finally:
                    D.quiet(ctx.synchronize)
            refuses(lambda: ctx.update_mesh_vertices(v2[:-1]), B.PTMI_EINVAL)                       # refused: another count
            refuses(lambda: ctx._check(ctx._lib.ptmi_update_mesh_vertices(ctx._h, None, len(t))), B.PTMI_EINVAL)
            nodes, order = ctx.mesh_read_layout()
            assert len(order) == len(t) - 1 and len(nodes) >= 1 or not D.PLAIN
        except (B.PtmiError, MemoryError):
            # after an injected failure inside an update the context is used again: the scene it holds is whole
            for k in range(6):
                D.stub.hipstub_fail(k, 0)
            D.stub.hipstub_clear_error()
            ctx.update_mesh_vertices(v)
            ctx.render(D.cam, 8, 1)
            ctx.mesh_read_layout()
            ctx.download_color()
            raise
        ctx.set_scene(*W.scene16())                               # a scene that is no mesh scene: the refit's blocks go with the mesh
        refuses(lambda: ctx.update_mesh_vertices(v2), B.PTMI_ESTATE)
        refuses(ctx.mesh_read_layout, B.PTMI_ESTATE)
        ctx.render(D.cam, 8, 1)
    with pkg.Group([0, 0], 8) as g:
        g.set_scene_mesh(s, t, p)
        g.resize(48, 32)
        g.init_output(1)
        g.update_mesh_vertices(v2)
        g.render(D.cam, 8, 1)
        g.download_color()
        refuses(lambda: g.update_mesh_vertices(v2[:-1]), B.PTMI_EINVAL)
        g.member(1).mesh_read_layout()


D.SCENARIOS = [mesh_refit]

if __name__ == "__main__":
    D.main()
