"""Register, scratch and LDS budgets of the ray-query kernels (csrc/ptmi_query.hip; compiled here, no GPU needed), pinned as
tests/test_bvh_kernel_resources.py and tests/test_mesh_kernel_resources.py pin the render kernels'.  One closest-hit and one any-hit kernel
per scene kind: linear, linear with shared-xy runs, BVH, mesh.  The hierarchies' kernels walk on check_hit_bvh's LDS stack -- one column of
PTMI_BVH_MAX_DEPTH words per lane, 6 KB per wave, shared by the any-hit walk, the sphere walk and the triangle walk -- so four waves per
SIMD is their ceiling, and they stay under the 128 VGPRs that ceiling allows.

Scratch: no kernel of the unit has any, nor a scratch load or store.  The mesh scene's literal fold (check_hit_mesh_exact), whose 16-byte frame
eval_check_hit_mesh_kernel carries (tests/test_mesh_kernel_resources.py), is inlined in this unit (PTMI_MESH_EXACT_INLINE) and calls
check_hit_exact as a leaf."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STACK_LDS = 24 * 64 * 4          # PTMI_BVH_MAX_DEPTH words per lane, 64 lanes: check_hit_bvh's stack, which the mesh walk shares
# kernel -> (VGPRs, static LDS bytes), pinned at what the build produces
PINNED = {
    "trace_rays_linear_kernel": (34, 0),
    "trace_rays_shared_xy_kernel": (34, 0),
    "trace_rays_bvh_kernel": (65, STACK_LDS),
    "trace_rays_mesh_kernel": (65, STACK_LDS),
    "occluded_linear_kernel": (33, 0),
    "occluded_shared_xy_kernel": (33, 0),
    "occluded_bvh_kernel": (65, STACK_LDS),
    "occluded_mesh_kernel": (65, STACK_LDS),
}


@pytest.fixture(scope="module")
def resources(tmp_path_factory):
    """{kernel: its figures} of ptmi_query.hip alone (tools/kernel_resources.py's compile and parse)"""
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    import re
    asm = kr.assembly(out_dir=str(tmp_path_factory.mktemp("isa")), units=["ptmi_query.hip"])["ptmi_query.hip"]
    ks = kr.kernels_of(open(asm).read())
    found = {}
    for (name, body, code), demangled in zip(ks, kr.demangle([k[0] for k in ks])):
        get = lambda k: int(re.search(k + r" (\d+)", body).group(1))   # noqa: E731
        found[demangled] = {"vgpr": get("next_free_vgpr"), "scratch": get("private_segment_fixed_size"), "lds": get("group_segment_fixed_size"),
                            "scratch_loads": len(re.findall(r"scratch_load", code)), "scratch_stores": len(re.findall(r"scratch_store", code)),
                            "sgpr_spill_lanes": len(re.findall(r"v_writelane_b32", code))}
    return found


def test_the_unit_holds_one_kernel_of_each_query_per_scene_kind(resources):
    assert sorted(resources) == sorted(PINNED)
    for name in resources:
        assert "refit" not in name and "mesh_build" not in name          # (other tests enumerate kernels by these substrings)


@pytest.mark.parametrize("kernel", sorted(PINNED))
def test_query_kernel_registers_and_lds_are_pinned(resources, kernel):
    r = resources[kernel]
    assert (r["vgpr"], r["lds"]) == PINNED[kernel], (kernel, r)
    assert r["vgpr"] <= 128 and r["lds"] <= STACK_LDS and r["sgpr_spill_lanes"] == 0, (kernel, r)


@pytest.mark.parametrize("kernel", sorted(PINNED))
def test_no_query_kernel_loads_or_stores_scratch(resources, kernel):
    r = resources[kernel]
    assert (r["scratch_loads"], r["scratch_stores"]) == (0, 0), (kernel, r)


@pytest.mark.parametrize("kernel", sorted(PINNED))
def test_no_query_kernel_has_scratch(resources, kernel):
    assert resources[kernel]["scratch"] == 0, (kernel, resources[kernel])
