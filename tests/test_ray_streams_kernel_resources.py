"""Register, scratch and LDS budgets of the Streams ray kernels (csrc/ptmi_trace_streams.hip; compiled here, no GPU needed), pinned as
tests/test_ray_paths_kernel_resources.py pins the path kernels'.  One kernel per scene kind: a linear scene staged in LDS, a linear scene
through scalar loads, a BVH scene, a mesh scene.

Every kernel keeps the start record -- two start hits of 10 words -- in a lane-private LDS column (5 120 bytes per wave).  The hierarchies'
kernels walk on check_hit_bvh's LDS stack beside it, PTMI_BVH_MAX_DEPTH words per lane, and stay under the 128 VGPRs their four waves per
SIMD allow.  The linear kernels keep the tree walk's budget of six waves per SIMD: 512 / 6 = 85 registers, 80 at the allocation granule of 8.

The deeper levels of the lane's stack of waiting children live in scratch memory, as in the render tree kernels: no kernel here has more
scratch than the render tree kernel of the same scene kind has in the same build (read from ptmi_streams_tree.hip's assembly, not from a
number written here), and none spills a scalar register into a vector register's lanes."""
import importlib.util
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STACK_LDS = 24 * 64 * 4          # PTMI_BVH_MAX_DEPTH words per lane, 64 lanes: check_hit_bvh's stack, which the mesh walk shares
START_LDS = 2 * 10 * 64 * 4      # the start record's columns
TREE_WAVES = 6                   # PTMI_TREE_WAVES
TREE_VGPRS = (512 // TREE_WAVES) // 8 * 8
# kernel -> (VGPRs, static LDS bytes), pinned at what the build produces
PINNED = {
    "trace_streams_linear_lds_kernel": (80, START_LDS),
    "trace_streams_linear_scalar_kernel": (80, START_LDS),
    "trace_streams_bvh_kernel": (110, START_LDS + STACK_LDS),
    "trace_streams_mesh_kernel": (127, START_LDS + STACK_LDS),
}
HIERARCHY = ("trace_streams_bvh_kernel", "trace_streams_mesh_kernel")
LINEAR = ("trace_streams_linear_lds_kernel", "trace_streams_linear_scalar_kernel")
# the render tree kernels of the same scene kind (either mapping of waves to pixels)
RENDER = {"trace_streams_linear_lds_kernel": "render_streams_tree_kernel<true,", "trace_streams_linear_scalar_kernel": "render_streams_tree_kernel<false,",
          "trace_streams_bvh_kernel": "render_streams_tree_bvh_kernel<", "trace_streams_mesh_kernel": "render_streams_tree_mesh_kernel<"}


@pytest.fixture(scope="module")
def units(tmp_path_factory):
    """{unit: {kernel: its figures}} of ptmi_trace_streams.hip and ptmi_streams_tree.hip, each compiled alone (tools/kernel_resources.py)"""
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    names = ["ptmi_trace_streams.hip", "ptmi_streams_tree.hip"]
    asm = kr.assembly(out_dir=str(tmp_path_factory.mktemp("isa")), units=names)
    out = {}
    for unit in names:
        ks = kr.kernels_of(open(asm[unit]).read())
        found = {}
        for (name, body, code), demangled in zip(ks, kr.demangle([k[0] for k in ks])):
            get = lambda k: int(re.search(k + r" (\d+)", body).group(1))   # noqa: E731
            found[demangled] = {"vgpr": get("next_free_vgpr"), "scratch": get("private_segment_fixed_size"), "lds": get("group_segment_fixed_size"),
                                "sgpr_spill_lanes": len(re.findall(r"v_writelane_b32", code))}
        out[unit] = found
    return out


@pytest.fixture(scope="module")
def resources(units):
    return units["ptmi_trace_streams.hip"]


def test_the_unit_holds_exactly_one_kernel_per_scene_kind(resources, pkg):
    assert sorted(resources) == sorted(PINNED)
    for name in resources:
        assert "refit" not in name and "mesh_build" not in name          # (other tests enumerate kernels by these substrings)
    assert "ptmi_trace_streams.hip" in pkg._build.KERNEL_UNITS and "ptmi_trace_streams.cpp" in pkg._build.HOST_SOURCES


@pytest.mark.parametrize("kernel", sorted(PINNED))
def test_registers_and_lds_are_pinned(resources, kernel):
    r = resources[kernel]
    assert (r["vgpr"], r["lds"]) == PINNED[kernel], (kernel, r)


@pytest.mark.parametrize("kernel", HIERARCHY)
def test_the_hierarchy_kernels_hold_the_stack_and_the_start_record_under_128_registers(resources, kernel):
    r = resources[kernel]
    assert r["lds"] == STACK_LDS + START_LDS and r["vgpr"] <= 128, (kernel, r)


@pytest.mark.parametrize("kernel", LINEAR)
def test_the_linear_kernels_keep_the_tree_walks_occupancy_budget(resources, kernel):
    r = resources[kernel]
    assert r["vgpr"] <= TREE_VGPRS == 80 and r["lds"] == START_LDS, (kernel, r)


@pytest.mark.parametrize("kernel", sorted(PINNED))
def test_no_kernel_spills_scalar_registers_into_lanes(resources, kernel):
    assert resources[kernel]["sgpr_spill_lanes"] == 0, (kernel, resources[kernel])


@pytest.mark.parametrize("kernel", sorted(PINNED))
def test_scratch_is_no_larger_than_the_render_tree_kernels_of_the_same_kind(units, kernel):
    render = {name: r["scratch"] for name, r in units["ptmi_streams_tree.hip"].items() if name.replace(" ", "").startswith(RENDER[kernel].replace(" ", ""))}
    assert len(render) == 2, (kernel, sorted(units["ptmi_streams_tree.hip"]))
    ours = units["ptmi_trace_streams.hip"][kernel]["scratch"]
    stack = (16 - 4) * 14 * 4                                            # the scratch levels of the stack of waiting children
    assert stack <= ours <= min(render.values()), (kernel, ours, render)
