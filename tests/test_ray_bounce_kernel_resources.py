"""Register, scratch and LDS budgets of the stepped path kernels (csrc/ptmi_bounce.hip; compiled here, no GPU needed), pinned as
tests/test_ray_paths_kernel_resources.py pins the path kernels'.  The unit holds exactly the five step kernels -- a linear scene staged in
LDS without and with shared-xy runs, a linear scene through scalar loads, a BVH scene, a mesh scene -- and the three kernels of the live
list's compaction (count, scan, scatter).

A step has nothing to restart from, so the hierarchies' kernels hold check_hit_bvh's LDS stack alone -- PTMI_BVH_MAX_DEPTH words per lane,
6 KB per wave -- and stay under the 128 VGPRs that four waves per SIMD (PTMI_BVH_WAVES) allow.  The staged kernels keep render Inline's
occupancy budget, PTMI_INLINE_WAVES = 7 waves per SIMD: 512 / 7 = 73 registers, 72 at the allocation granule of 8; their LDS is the
scene's, given at launch.  The compaction's static LDS is one word per wave of a block (count, scatter) and the scan's two buffers.

No kernel of the unit has scratch, a scratch load or store, or a scalar register spilled into a vector register's lanes."""
import importlib.util
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNIT = "ptmi_bounce.hip"
STACK_LDS = 24 * 64 * 4          # PTMI_BVH_MAX_DEPTH words per lane, 64 lanes: check_hit_bvh's stack, which the mesh walk shares
INLINE_WAVES = 7                 # PTMI_INLINE_WAVES
INLINE_VGPRS = (512 // INLINE_WAVES) // 8 * 8
LIVE_BLOCK = 256                 # kLiveBlock
# kernel -> (VGPRs, static LDS bytes), pinned at what the build produces
PINNED = {
    "bounce_rays_linear_lds_kernel": (54, 0),
    "bounce_rays_shared_xy_lds_kernel": (54, 0),
    "bounce_rays_linear_scalar_kernel": (54, 0),
    "bounce_rays_bvh_kernel": (65, STACK_LDS),
    "bounce_rays_mesh_kernel": (68, STACK_LDS),
    "live_rays_count_kernel": (8, 4 * LIVE_BLOCK // 64),
    "live_rays_scan_kernel": (8, 2 * 4 * LIVE_BLOCK),
    "live_rays_scatter_kernel": (9, 4 * LIVE_BLOCK // 64),
}
STEP = sorted(k for k in PINNED if k.startswith("bounce_rays_"))
HIERARCHY = ("bounce_rays_bvh_kernel", "bounce_rays_mesh_kernel")
STAGED = ("bounce_rays_linear_lds_kernel", "bounce_rays_shared_xy_lds_kernel")


@pytest.fixture(scope="module")
def resources(tmp_path_factory):
    """{kernel: its figures} of ptmi_bounce.hip alone (tools/kernel_resources.py's compile and parse)"""
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    asm = kr.assembly(out_dir=str(tmp_path_factory.mktemp("isa")), units=[UNIT])[UNIT]
    ks = kr.kernels_of(open(asm).read())
    found = {}
    for (name, body, code), demangled in zip(ks, kr.demangle([k[0] for k in ks])):
        get = lambda k: int(re.search(k + r" (\d+)", body).group(1))   # noqa: E731
        found[demangled] = {"vgpr": get("next_free_vgpr"), "scratch": get("private_segment_fixed_size"), "lds": get("group_segment_fixed_size"),
                            "scratch_loads": len(re.findall(r"scratch_load", code)), "scratch_stores": len(re.findall(r"scratch_store", code)),
                            "sgpr_spill_lanes": len(re.findall(r"v_writelane_b32", code))}
    return found


def test_the_unit_holds_the_five_step_kernels_and_the_compaction_kernels(resources, pkg):
    assert sorted(resources) == sorted(PINNED)
    assert len(STEP) == 5 and len(PINNED) - len(STEP) == 3
    for name in resources:
        assert "refit" not in name and "mesh_build" not in name          # (other tests enumerate kernels by these substrings)
    assert UNIT in pkg._build.KERNEL_UNITS


@pytest.mark.parametrize("kernel", sorted(PINNED))
def test_registers_and_lds_are_pinned(resources, kernel):
    r = resources[kernel]
    assert (r["vgpr"], r["lds"]) == PINNED[kernel], (kernel, r)


@pytest.mark.parametrize("kernel", HIERARCHY)
def test_the_hierarchy_kernels_hold_the_stack_alone_under_128_registers(resources, kernel):
    r = resources[kernel]
    assert r["lds"] == STACK_LDS and r["vgpr"] <= 128, (kernel, r)


@pytest.mark.parametrize("kernel", STAGED)
def test_the_staged_kernels_keep_render_inlines_occupancy_budget(resources, kernel):
    r = resources[kernel]
    assert r["vgpr"] <= INLINE_VGPRS == 72 and r["lds"] == 0, (kernel, r)


@pytest.mark.parametrize("kernel", sorted(PINNED))
def test_no_kernel_has_scratch_or_spills(resources, kernel):
    r = resources[kernel]
    assert (r["scratch"], r["scratch_loads"], r["scratch_stores"], r["sgpr_spill_lanes"]) == (0, 0, 0, 0), (kernel, r)
