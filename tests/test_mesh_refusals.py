"""ptmi_set_scene_mesh's refusals and its transaction, on the CPU: a CHILD process runs libptmi on the HIP stand-in of
tests/cxx/hip_stub.cpp (preloaded, without a sanitizer: kernels do not run, launches are logged).  Non-finite vertex or material data,
counts over the limits, the stream form, a kernel variant and contracted arithmetic are refused with the documented codes; a failed
allocation or upload leaves the previous scene (the next render launches the previous scene's kernel); triangles of zero area are
accepted; a mesh scene's render launches the mesh kernel."""
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
STUB = os.path.join(ROOT, "build", "hip_stub", "libhipstub_plain.so")


def child(out_path):
    import ctypes
    import __graft_entry__ as graft
    pkg = graft.load_package()
    B, W = pkg.binding, pkg.world
    stub = ctypes.CDLL(os.environ["PTMI_HIPSTUB"])
    assert stub.hipstub_is_the_stub() == 1
    stub.hipstub_log.restype = ctypes.c_char_p
    stub.hipstub_set_device_size.argtypes = [ctypes.c_int, ctypes.c_ulonglong]
    stub.hipstub_set_device_size(8, 4 << 30)
    res = {}
    cam = W.initial_camera()

    def code(call):
        try:
            call()
            return 0
        except B.PtmiError as e:
            return e.code

    def kernels():                                    # the kernels one render launches
        stub.hipstub_clear_log()
        c.render(cam, 4, 1, B.INLINE)
        return [line.split()[1] for line in stub.hipstub_log().decode().splitlines() if line.startswith("launch ")]

    s, t, p = W.mesh_room(1)
    small = W.scene16()
    with pkg.Context(0) as c:
        c.resize(16, 8)
        c.init_output(1)
        c.set_scene(*small)
        bad = {}
        for field, value in (("v0", np.nan), ("v2", np.inf), ("color", np.nan), ("illuminance", np.inf), ("brdf_param", np.nan), ("v1", 3e19)):
            tt = t.copy()
            if field in ("v0", "v1", "v2", "color"):
                tt[field][13, 1] = value
            else:
                tt[field][13] = value
            bad[field + ":" + str(value)] = code(lambda: c.set_scene_mesh(s, tt, p))
        res["non_finite"] = bad
        res["too_many_triangles"] = code(lambda: c.set_scene_mesh(s, np.zeros(B.MAX_MESH_TRIANGLES + 1, W.TRIANGLE_DTYPE), p))
        res["too_many_planes"] = code(lambda: c.set_scene_mesh(s, t, np.repeat(small[1], 33)))
        res["nothing"] = code(lambda: c.set_scene_mesh(s[:0], t[:0], p[:0]))
        res["linear_kernels_after_refusals"] = kernels()
        for kind in (0, 1):                            # the k-th allocation / copy of the call fails: the linear scene stays
            for k in (1, 2, 3):
                stub.hipstub_fail(kind, k)
                rc = code(lambda: c.set_scene_mesh(s, t, p))
                stub.hipstub_fail(kind, 0)
                res["fail_%d_%d" % (kind, k)] = [rc, kernels(), code(lambda: c.set_variant(5)), code(lambda: c.set_variant(0))]
        c.set_option(B.OPT_STREAMS_FORM, B.FORM_STREAM)
        res["stream_form"] = code(lambda: c.set_scene_mesh(s, t, p))
        c.set_option(B.OPT_STREAMS_FORM, B.FORM_AUTO)
        c.set_variant(5)
        res["variant"] = code(lambda: c.set_scene_mesh(s, t, p))
        c.set_variant(0)
        c.set_option(B.OPT_ARITHMETIC, B.ARITH_CONTRACTED)
        res["contracted"] = code(lambda: c.set_scene_mesh(s, t, p))
        c.set_option(B.OPT_ARITHMETIC, B.ARITH_EXACT)
        flat = t.copy()
        flat["v2"] = flat["v1"]
        res["zero_area"] = code(lambda: c.set_scene_mesh(s, flat, p))
        res["mesh_kernels"] = kernels()
        res["mesh_refuses_variant"] = code(lambda: c.set_variant(5))
        res["mesh_refuses_stream_form"] = code(lambda: c.set_option(B.OPT_STREAMS_FORM, B.FORM_STREAM))
        c.set_option(B.OPT_ARITHMETIC, B.ARITH_CONTRACTED)
        stub.hipstub_clear_log()
        res["mesh_refuses_contracted_render"] = code(lambda: c.render(cam, 4, 1, B.INLINE))
        c.set_option(B.OPT_ARITHMETIC, B.ARITH_EXACT)
    with open(out_path, "w") as f:
        json.dump(res, f)


def test_refusals_and_the_transaction_on_the_hip_stand_in(tmp_path):
    from test_host_sanitized import build_stub
    import __graft_entry__ as graft
    B = graft.load_package().binding
    graft.load_package()._build.build_lib()
    stub = build_stub(STUB, sanitize=None)
    out = str(tmp_path / "refusals.json")
    env = dict(os.environ, PTMI_HIPSTUB=stub, LD_PRELOAD=stub)
    run = subprocess.run([sys.executable, os.path.abspath(__file__), out], env=env, capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, (run.stdout + run.stderr)[-4000:]
    res = json.load(open(out))
    assert set(res["non_finite"].values()) == {B.PTMI_EINVAL}, res["non_finite"]
    assert res["too_many_triangles"] == B.PTMI_ELIMIT and res["too_many_planes"] == B.PTMI_ELIMIT and res["nothing"] == B.PTMI_EINVAL
    linear = res["linear_kernels_after_refusals"]
    assert linear and not any("mesh" in k for k in linear), linear
    for key in [k for k in res if k.startswith("fail_")]:
        rc, launched, variant_rc, back_rc = res[key]
        assert rc in (B.PTMI_ENOMEM, B.PTMI_EHIP), (key, rc)
        assert launched == linear, (key, launched)                 # the linear scene still renders
        assert variant_rc == 0 and back_rc == 0, key                # ... and takes variants, which a mesh scene would refuse
    assert res["stream_form"] == B.PTMI_EINVAL and res["variant"] == B.PTMI_EINVAL and res["contracted"] == B.PTMI_EINVAL
    assert res["zero_area"] == 0
    mesh = res["mesh_kernels"]
    assert any("render_inline_mesh_kernel" in k for k in mesh), mesh
    assert res["mesh_refuses_variant"] == B.PTMI_EINVAL and res["mesh_refuses_stream_form"] == B.PTMI_EINVAL
    assert res["mesh_refuses_contracted_render"] == B.PTMI_EINVAL


if __name__ == "__main__":
    child(sys.argv[1])
