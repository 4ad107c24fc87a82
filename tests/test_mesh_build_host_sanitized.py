"""The host side of ptmi_set_mesh_triangles under AddressSanitizer + UndefinedBehaviorSanitizer on the HIP stand-in, with the demands of
tests/test_host_sanitized.py: tests/hostsan_build_driver.py sets a mesh scene, gives it more triangles from host memory and fewer from a
stand-in device block (the check kernel's kept count placed into its read-back, so that the whole path is launched), five and none,
makes refused calls, calls on a scene that is no mesh scene and on a group, reads the layout back and destroys everything -- plainly,
then once per failure point (the k-th allocation, copy, launch or synchronise fails; with the next call of the kind; with every later
one).  After an injected failure inside a build the context still renders and reads back the scene it held, takes new triangles and is
destroyed cleanly.  No sanitizer report, nothing left alive on the stand-in -- none of the fresh blocks, not the sort's scratch --
nothing in the runtime's sticky slot."""
import os
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_host_sanitized as H  # noqa: E402


@H.needs_asan
def test_new_mesh_triangles_are_clean_under_asan_and_ubsan_at_every_failure_point():
    import test_gpu_group_rccl_stub as rccl
    pkg = H.graft.load_package()
    stub = H.build_stub()
    rccl_dir = os.path.dirname(rccl.build_stub())
    lib = pkg._build.build_lib(out=H.SANITIZED, extra_flags=H.HOST_SANITIZE)
    assert "__asan_init" in H.dynamic_symbols(lib, True)
    env = dict(os.environ, PTMI_HIPSTUB=stub, PTMI_SANITIZED_LIB=lib, LD_PRELOAD="%s %s" % (H.asan_runtime(), stub),
               LD_LIBRARY_PATH=rccl_dir + os.pathsep + os.environ.get("LD_LIBRARY_PATH", ""),
               ASAN_OPTIONS="detect_leaks=0:abort_on_error=0:exitcode=23", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    for name in ("PTMI_HOSTSAN_ONLY", "PTMI_HOSTSAN_STRIDE", "PTMI_HOSTSAN_DEFERRED"):
        env.pop(name, None)
    env["PTMI_HOSTSAN_MORE_STRIDE"] = "1"
    driver = os.path.join(H.ROOT, "tests", "hostsan_build_driver.py")
    for deferred in (False, True):                                # (True: the stand-in's streams truly asynchronous)
        if deferred:
            env["PTMI_HOSTSAN_DEFERRED"] = "1"
        run = subprocess.run([sys.executable, driver], capture_output=True, text=True, env=env, timeout=900)
        out = run.stdout + run.stderr
        assert "runtime error" not in out and "AddressSanitizer" not in out and "HIPSTUB:" not in out and "terminate called" not in out, out[-4000:]
        assert run.returncode == 0 and "sanitized host side: done" in run.stdout, out[-4000:]
        reports = [line for line in run.stdout.splitlines() if line.startswith("hostsan mesh_build")]
        assert len(reports) == 1, out[-4000:]
        walked = int(reports[0].split("'failure_points_walked': ")[1].split(",")[0])
        launches = int(reports[0].split("'kernel_launches': ")[1].split(",")[0])
        assert walked >= 100 and launches >= 20, reports
        print(reports[0])
