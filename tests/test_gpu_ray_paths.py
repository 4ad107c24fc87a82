"""Paths along a caller's own rays on the device: ptmi_trace_paths_device, ptmi_trace_paths_indexed_device and ptmi_path_seeds_device through
Context.trace_paths / Context.path_seeds with torch tensors, on the context's stream -- render Inline's traceInline for rays a camera did
not make, held to the oracle word for word.

The torch part runs in ONE child process (tests/ray_paths_driver.py), where torch brings the runtime up before the library is loaded, as
in bench.py -- the convention of tests/test_gpu_ray_query.py; it is a fresh process and nothing is exec'd.  The child makes the five scenes
of tests/ray_paths_inputs.py, one per kernel -- mainScene, the 16-primitive bench scene, a linear scene just past the LDS budget,
bvh_rays.adversarial_scene(3000) as a BVH scene, world.mesh_room(3) with one plane -- each with 4 096 rays (camera primaries, light probes,
the adversarial families) whose reference tests/test_ray_paths_inputs.py holds to exercising the loop, and prints one line per case; each
test below reads its own line.  The child runs under one time limit; a runtime error ends it, and the cases behind it count as not run (a
failure).

The cases are those of the driver's docstrings:
  1 colour and seed == the reference (ora_trace_inline in ora_render_inline_ex's loop), any NaN a NaN, every scene, limits 1, 3, 8, 1 and 2 spp
  2 n = 0, 1, 63, 64, 65, 257; every array aligned and 4 bytes off; guard words around colour and seed
  3 the oracle's primary rays of a 67 x 45 image + path_seeds + a zero colour == init_output + render(INLINE, 8, 3) on seven planes;
    path_seeds from a first index == ora_gen_seeds
  4 3 spp in one call == three calls of 1 spp; accumulation into a colour that is not zero
  5 through ray_order's permutation the plain words; through an active list the named rays alone
  6 bounce_limit 0 and -1; n_spp 0 and -1
  7 on torch's non-default stream; after update_spheres / set_mesh_triangles; renders around the calls unchanged, statistics untouched
  8 the refusals through the raw handle, a GLASS scene among them; nothing written"""
import os
import subprocess
import sys
import time

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ray_paths_driver as driver  # noqa: E402

pytestmark = pytest.mark.gpu
LIMIT = 420                                  # seconds for the child: process start, torch, five scenes, the references, eight cases


@pytest.fixture(scope="module")
def outcome(pkg, ora, tmp_path_factory):
    """{case: None if it passed, else why not} from one run of the child"""
    t0 = time.perf_counter()
    res = subprocess.run([sys.executable, os.path.join(HERE, "ray_paths_driver.py"), str(tmp_path_factory.mktemp("ray_paths"))],
                         capture_output=True, text=True, timeout=LIMIT)
    print(res.stdout)
    print("ray_paths_driver: %.1f s, exit %d" % (time.perf_counter() - t0, res.returncode))
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
def test_paths_along_a_callers_rays(outcome, case):
    assert outcome[case] is None, outcome[case]
