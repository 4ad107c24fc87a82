"""ptmi_occluded_device held to the closest hit on every tree and at every scale the hierarchies serve, on the device: Context.occluded
against `just && t < t_max` of the literal fold for every family of t_max, exactly, and Context.trace_rays against ptmi_eval_check_hit bit
for bit.  tests/test_any_hit_traversal.py is the CPU half; tests/test_gpu_ray_query.py holds the queries' interface.

The torch part runs in ONE child process (tests/any_hit_driver.py), where torch brings the runtime up before the library is loaded -- the
convention of tests/test_gpu_ray_query.py; it is a fresh process and nothing is exec'd.  The child prints one line per case and each test
below reads its own; it runs under one time limit, a runtime error ends it, and the cases behind it count as not run (a failure).  Every
case asserts on its own inputs what keeps it from passing vacuously (any_hit_rays.assert_conditions) before it compares.

The cases are those of the driver:
  a  the sphere hierarchies of test_mesh_exact.bvh_cases(), 20 000 adversarial and admission-bracket rays each
  b  the mesh families of mesh_rays.SWEPT and needles_1e7 at every placement, 6 000 rays each and more of what a family is thin in
  c  trees no build produced: after update_mesh_vertices to moved, far and squashed and after update_spheres by a wave, against the fold
     of the new geometry
  d  device-built trees: set_bvh_spheres under both values of PTMI_OPT_BVH_DEVICE_BUILD (3 000 spheres), set_mesh_triangles (the room at
     subdivision 3)
  e  linear scenes: mainScene, the bench scene, and a field with radii up to 2^20 on either side of sphere_reach's limit
  f  the guards: a BVH scene of 0 spheres and 2 planes, of 1 sphere, of 300 coincident spheres; a mesh scene of 0 spheres, of 0 triangles,
     of triangles of zero area alone; 4 096 rays each, four non-finite ones among them"""
import os
import subprocess
import sys
import time

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import any_hit_driver as driver  # noqa: E402

pytestmark = pytest.mark.gpu
# seconds for the child: process start, torch, 51 scenes with their folds and restatements on the host.  One run took 5.0 s on an MI355X machine
# with 16 host threads; the host's share alone takes about 25 s on 8 slower ones
LIMIT = 300


@pytest.fixture(scope="module")
def outcome(pkg, ora, tmp_path_factory):
    """{case: None if it passed, else why not} from one run of the child"""
    t0 = time.perf_counter()
    res = subprocess.run([sys.executable, os.path.join(HERE, "any_hit_driver.py"), str(tmp_path_factory.mktemp("any_hit"))],
                         capture_output=True, text=True, timeout=LIMIT)
    print(res.stdout)
    print("any_hit_driver: %.1f s, exit %d" % (time.perf_counter() - t0, res.returncode))
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
def test_occlusion_is_the_closest_hits_answer_on_the_device(outcome, case):
    assert outcome[case] is None, outcome[case]
