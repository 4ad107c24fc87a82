"""A caller's own rays on the device: ptmi_trace_rays_device (closest hit with its hit record) and ptmi_occluded_device (anything in the
way before t_max) through Context.trace_rays / Context.occluded with torch tensors, on the context's stream.

The torch part runs in ONE child process (tests/ray_query_driver.py), where torch brings the runtime up before the library is loaded, as
in bench.py -- the convention of tests/test_gpu_mesh_build.py; it is a fresh process and nothing is exec'd.  The child makes five scenes
-- a linear scene without shared-xy runs (mainScene), the 16-primitive bench scene (three runs), a made run (tests/test_gpu_shared_xy.py:
row_scene), bvh_rays.adversarial_scene(3000) as a BVH scene and mesh_rays.adversarial_scene at its smallest subdivision with its 8 spheres --
each with 4 096 adversarial rays (the non-finite, off-length and beyond-2^40 families included) and, once, ptmi_eval_check_hit's answer and
the oracle's fold, and prints one line per case; each test below reads its own line.  The child runs under one time limit; a runtime error
ends it, and the cases behind it count as not run (a failure).

The cases are those of the driver's docstrings:
  1 trace_rays == ptmi_eval_check_hit bit for bit == the oracle's fold, on every scene kind
  2 n = 0, 1, 63, 64, 65, 257, 4 096; rays and hit records 8-byte aligned and 4 bytes off; guard words around every output
  3 the hit record: position o + d * t, sphere normals by ora_hit_sphere (tests/cxx/ray_query_reference.c), plane and triangle normals
    as stored, zeros for a miss
  4 occluded against its specification, t_max from nextafter(t, 0), t, nextafter(t, inf), t / 2, 2 t, 0, -1, +inf, NaN for hits and 1, +inf,
    NaN for misses, every family counted in every scene kind
  5 on torch's non-default stream, read after that stream alone is synchronised
  6 after update_spheres / set_mesh_triangles from device tensors, against a context set afresh
  7 the refusals, through the raw library handle; nothing written
  8 a render between queries equals a render without them on all seven planes
  9 scene data that is not finite (a linear scene's spheres, a linear and a BVH scene's planes): the full search, the specification's answers
The families of t_max are tests/t_max_families.py's.  Occlusion beyond these five scenes -- other trees (refitted, device-built), scales,
offsets, the admission brackets and the guards -- is held to the closest hit by tests/test_any_hit_traversal.py (a CPU restatement of the
any-hit walks, tests/cxx/any_hit_traverse.c) and tests/test_gpu_any_hit.py (tests/any_hit_driver.py, on the device)."""
import os
import subprocess
import sys
import time

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ray_query_driver as driver  # noqa: E402

pytestmark = pytest.mark.gpu
LIMIT = 420                                  # seconds for the child: process start, torch, five scenes, the oracle's folds, eight cases


@pytest.fixture(scope="module")
def outcome(pkg, ora, tmp_path_factory):
    """{case: None if it passed, else why not} from one run of the child"""
    t0 = time.perf_counter()
    res = subprocess.run([sys.executable, os.path.join(HERE, "ray_query_driver.py"), str(tmp_path_factory.mktemp("ray_query"))],
                         capture_output=True, text=True, timeout=LIMIT)
    print(res.stdout)
    print("ray_query_driver: %.1f s, exit %d" % (time.perf_counter() - t0, res.returncode))
    tail = (res.stdout + res.stderr)[-3000:]
    found = {}
    for line in res.stdout.splitlines():
        if line.startswith("ok "):
            found[line[3:]] = None
        elif line.startswith("FAILED "):
            name, _, why = line[7:].partition(": ")
            found[name] = why
    return {name: found.get(name, "not run: the child ended with %d before it\n%s" % (res.returncode, tail)) for name in driver.CASES}


@pytest.mark.parametrize("case", driver.CASES)
def test_ray_queries_on_the_device(outcome, case):
    assert outcome[case] is None, outcome[case]
