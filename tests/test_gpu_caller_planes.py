"""Renders into caller-owned planes on a caller's stream: the path a PyTorch caller -- bench.py, parallel.py -- takes.

Every other GPU test renders into the seven planes the context allocates itself (one block, every plane 256-byte aligned, padding behind
it) on the context's own stream with a host wait behind every call.  Here the planes are torch memory bound with ptmi_bind_planes:
unaligned, in shuffled order, guard bands around each (tests/caller_planes.py), so that a write past a plane's end, a kernel's wide path
on an unaligned plane, `c->owned` where `active(c)` is meant or a fixed stride between planes all show; and the stream is torch's, with no
host wait between the caller's work and the library's, so that a launch on the wrong stream shows.

torch runs in child processes of their own (tests/caller_planes_driver.py GROUP, one function per group), where it brings the runtime
up before the library is loaded, as in bench.py -- the convention of tests/test_gpu_bvh_update.py.  A child prints one line per case, stops at
its first failure, and ends with CALLER_PLANES_OK <count>; the parent holds the printed names against caller_planes_driver.CASES.

Rows of the table (the driver's case names begin with the letter):
  a Inline, automatic choice, five launches   b Inline variants 4, 5, 13, 17, sample chunks   c row mapping, degenerate sizes, limit 0, spp 0
  d Streams chain   e GLASS tree walk   f stream form without GLASS, automatic and forced tail   g stream form with GLASS, a redone call
  h BVH scenes   i mesh scenes (twin context)   j three parts of a partition, stitched
then the helper entries (init_output, reseed, create_with, upload / download, present, snapshot_color, device_planes), the lifecycle
(unbind, rebind, a refused partial bind, a bind before resize, resize while bound), the caller's stream, and bench.py's configuration.

Row f, the tail: nothing the product library reports -- neither ptmi_stats nor ptmi_debug_counters -- says how many dispatch positions
the per-pixel tail took: where the tail begins is a device word that only the two kernels read.  The cases therefore establish on
the host what makes the library launch the tail (PTMI_OPT_STREAM_TAIL reads back 950, a tiled size, a third and fourth launch with one key,
ptmi_render_blocks 0) and compare every launch bit for bit with the chain; they cannot assert the count of positions.

Row g, the redone call: the overflow streams never hold fewer slots than the waves' static blocks (393 472), so no 64 x 48 image can drop
a child; the redo is forced at 800 x 600 and 4 spp, where tests/test_gpu_wavefront.py forces it."""
import os
import subprocess
import sys
import time

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import caller_planes_driver as driver  # noqa: E402

pytestmark = pytest.mark.gpu
DRIVER = os.path.join(HERE, "caller_planes_driver.py")
LIMITS = {"inline": 240, "streams": 300, "scenes": 240, "helpers": 240, "stream": 240}      # seconds: process start, torch, the oracle's share


@pytest.fixture(scope="module")
def tiny_rings(pkg, tmp_path_factory):
    """libptmi with a ring of 2 and a spill queue of 4 records per wave: children reach the overflow streams (the module's one extra build)"""
    out = os.path.join(str(tmp_path_factory.mktemp("caller_planes_tinyrings")), "libptmi_tinyrings.so")
    return pkg._build.build_lib(out=out, extra_flags=["-DPTMI_RING=2", "-DPTMI_SPILL=4"])


def run_group(group, *args):
    t0 = time.perf_counter()
    res = subprocess.run([sys.executable, DRIVER, group] + list(args), capture_output=True, text=True, timeout=LIMITS[group])
    lines = res.stdout.splitlines()
    print(res.stdout)
    print("group %s: %.1f s" % (group, time.perf_counter() - t0))
    assert res.returncode == 0, (res.stdout + res.stderr)[-4000:]
    names = [line[3:] for line in lines if line.startswith("ok ")]
    assert names == driver.CASES[group], (names, driver.CASES[group])
    assert lines and lines[-1] == "CALLER_PLANES_OK %d" % len(driver.CASES[group]), lines[-3:]


def test_inline_renders_into_caller_planes(pkg, ora):
    """rows a, b, c, j"""
    run_group("inline")


def test_streams_render_into_caller_planes(pkg, ora, tiny_rings):
    """rows d, e, f, g"""
    run_group("streams", tiny_rings)


def test_bvh_and_mesh_scenes_render_into_caller_planes(pkg, ora):
    """rows h, i"""
    run_group("scenes")


def test_helper_entries_and_lifecycle_on_caller_planes(pkg, ora):
    run_group("helpers")


def test_renders_on_the_callers_stream_and_in_the_benchmarks_configuration(pkg, ora):
    """What the stream cases can show and what they cannot is in caller_planes_driver.group_stream's docstring: a launch on the wrong
    stream fails reliably (the filler in front of the start planes lasts ten times the host time of the calls); a missing join of the
    tail's side stream fails only when timing allows, and may pass by luck."""
    run_group("stream")
