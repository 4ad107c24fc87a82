"""Register, scratch and LDS budgets of the path kernels (csrc/ptmi_paths.hip; compiled here, no GPU needed), pinned as
tests/test_ray_query_kernel_resources.py pins the ray queries'.  One kernel per scene kind -- a linear scene staged in LDS without and with
shared-xy runs, a linear scene through scalar loads, a BVH scene, a mesh scene -- and the seeds' kernel.

Every path kernel keeps the restart record in a lane-private LDS column of 10 words (2 560 bytes per wave).  The hierarchies' kernels walk
on check_hit_bvh's LDS stack beside it -- PTMI_BVH_MAX_DEPTH words per lane, 6 KB per wave -- so four waves per SIMD is their ceiling
(PTMI_BVH_WAVES) and they stay under the 128 VGPRs that ceiling allows.  The staged kernels keep render Inline's occupancy budget,
PTMI_INLINE_WAVES = 7 waves per SIMD: 512 / 7 = 73 registers, 72 at the allocation granule of 8.

No kernel of the unit has scratch, a scratch load or store, or a scalar register spilled into a vector register's lanes."""
import importlib.util
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STACK_LDS = 24 * 64 * 4          # PTMI_BVH_MAX_DEPTH words per lane, 64 lanes: check_hit_bvh's stack, which the mesh walk shares
RESTART_LDS = 10 * 64 * 4        # the restart columns
INLINE_WAVES = 7                 # PTMI_INLINE_WAVES
INLINE_VGPRS = (512 // INLINE_WAVES) // 8 * 8
# kernel -> (VGPRs, static LDS bytes), pinned at what the build produces
PINNED = {
    "trace_paths_linear_lds_kernel": (60, RESTART_LDS),
    "trace_paths_shared_xy_lds_kernel": (60, RESTART_LDS),
    "trace_paths_linear_scalar_kernel": (60, RESTART_LDS),
    "trace_paths_bvh_kernel": (81, RESTART_LDS + STACK_LDS),
    "trace_paths_mesh_kernel": (96, RESTART_LDS + STACK_LDS),
    "path_seeds_kernel": (9, 0),
}
HIERARCHY = ("trace_paths_bvh_kernel", "trace_paths_mesh_kernel")
STAGED = ("trace_paths_linear_lds_kernel", "trace_paths_shared_xy_lds_kernel")


@pytest.fixture(scope="module")
def resources(tmp_path_factory):
    """{kernel: its figures} of ptmi_paths.hip alone (tools/kernel_resources.py's compile and parse)"""
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    asm = kr.assembly(out_dir=str(tmp_path_factory.mktemp("isa")), units=["ptmi_paths.hip"])["ptmi_paths.hip"]
    ks = kr.kernels_of(open(asm).read())
    found = {}
    for (name, body, code), demangled in zip(ks, kr.demangle([k[0] for k in ks])):
        get = lambda k: int(re.search(k + r" (\d+)", body).group(1))   # noqa: E731
        found[demangled] = {"vgpr": get("next_free_vgpr"), "scratch": get("private_segment_fixed_size"), "lds": get("group_segment_fixed_size"),
                            "scratch_loads": len(re.findall(r"scratch_load", code)), "scratch_stores": len(re.findall(r"scratch_store", code)),
                            "sgpr_spill_lanes": len(re.findall(r"v_writelane_b32", code))}
    return found


def test_the_unit_holds_one_path_kernel_per_scene_kind_and_the_seeds_kernel(resources, pkg):
    assert sorted(resources) == sorted(PINNED)
    for name in resources:
        assert "refit" not in name and "mesh_build" not in name          # (other tests enumerate kernels by these substrings)
    assert "ptmi_paths.hip" in pkg._build.KERNEL_UNITS


@pytest.mark.parametrize("kernel", sorted(PINNED))
def test_path_kernel_registers_and_lds_are_pinned(resources, kernel):
    r = resources[kernel]
    assert (r["vgpr"], r["lds"]) == PINNED[kernel], (kernel, r)


@pytest.mark.parametrize("kernel", HIERARCHY)
def test_the_hierarchy_kernels_hold_the_stack_and_the_restart_columns_under_128_registers(resources, kernel):
    r = resources[kernel]
    assert r["lds"] == STACK_LDS + RESTART_LDS and r["vgpr"] <= 128, (kernel, r)


@pytest.mark.parametrize("kernel", STAGED)
def test_the_staged_kernels_keep_render_inlines_occupancy_budget(resources, kernel):
    r = resources[kernel]
    assert r["vgpr"] <= INLINE_VGPRS == 72 and r["lds"] == RESTART_LDS, (kernel, r)


@pytest.mark.parametrize("kernel", sorted(PINNED))
def test_no_path_kernel_has_scratch_or_spills(resources, kernel):
    r = resources[kernel]
    assert (r["scratch"], r["scratch_loads"], r["scratch_stores"], r["sgpr_spill_lanes"]) == (0, 0, 0, 0), (kernel, r)
