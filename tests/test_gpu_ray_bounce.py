"""A caller's paths stepped one bounce at a time on the device: ptmi_bounce_rays_device, ptmi_bounce_rays_indexed_device and
ptmi_live_rays_device through Context.bounce_rays / Context.live_rays with torch tensors, on the context's stream -- one prepareRay per
call and the padded list of the rays still alive, held to the oracle word for word.

The torch part runs in ONE child process (tests/ray_bounce_driver.py), where torch brings the runtime up before the library is loaded, as
in bench.py -- the convention of tests/test_gpu_ray_paths.py; it is a fresh process and nothing is exec'd.  The child makes the five scenes
of tests/ray_paths_inputs.py, one per step kernel, each with its 4 096 rays, whose reference tests/test_ray_bounce_inputs.py holds to the
oracle's traceInline and to exercising the step, and prints one line per case; each test below reads its own line.  The child runs under
one time limit; a runtime error ends it, and the cases behind it count as not run (a failure).

The cases are those of the driver's docstrings:
  1 per scene, 8 steps from (1, 0): rays, throughput, radiance, seeds and the hit record == the reference after every step; t, idx and hit
    == Context.trace_rays on the incoming rays where the ray was traced
  2 after k steps 0 + radiance and the seeds == Context.trace_paths(limit k, 1 spp), k = 1, 3, 8
  3 n = 0, 1, 63, 64, 65, 257; every array aligned and 4 bytes off; guard words around every array; the optional outputs given singly
  4 the wavefront loop: step, live_rays in place, no host read; lists == the host twin's, count, empty by step 8; through ray_order's order
  5 live_rays alone against torch.nonzero at every level of the scan; an index with foreign entries; one past the limit refused
  6 through an index only the named rays change
  7 on torch's non-default stream; after update_spheres / set_mesh_triangles; renders around the calls unchanged, statistics untouched
  8 the refusals through the raw handle, a GLASS scene and a short or misaligned workspace among them; nothing written"""
import os
import subprocess
import sys
import time

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ray_bounce_driver as driver  # noqa: E402

pytestmark = pytest.mark.gpu
LIMIT = 420                                  # seconds for the child: process start, torch, five scenes, the references, eight cases


@pytest.fixture(scope="module")
def outcome(pkg, ora, tmp_path_factory):
    """{case: None if it passed, else why not} from one run of the child"""
    t0 = time.perf_counter()
    res = subprocess.run([sys.executable, os.path.join(HERE, "ray_bounce_driver.py"), str(tmp_path_factory.mktemp("ray_bounce"))],
                         capture_output=True, text=True, timeout=LIMIT)
    print(res.stdout)
    print("ray_bounce_driver: %.1f s, exit %d" % (time.perf_counter() - t0, res.returncode))
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
def test_stepped_paths_along_a_callers_rays(outcome, case):
    assert outcome[case] is None, outcome[case]
