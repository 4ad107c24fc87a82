"""Register, scratch and LDS budgets of the ray order's kernels (csrc/ptmi_ray_order.hip) and of the indexed ray queries'
(csrc/ptmi_query_indexed.hip; both compiled here, no GPU needed), in the style of tests/test_ray_query_kernel_resources.py.  The indexed
unit holds one closest-hit and one any-hit kernel per scene kind, as the plain unit does; a lane runs the plain kernels' per-ray functions
behind one more load, so the hierarchies' kernels keep check_hit_bvh's LDS stack -- 24 words per lane, 6 KB per wave, four waves per SIMD --
as their only LDS and stay under the 128 VGPRs that ceiling allows.  No kernel of either unit has scratch, nor a scratch load or store.
The bounds are the properties the design rests on, not the figures of one build."""
import importlib.util
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STACK_LDS = 24 * 64 * 4          # PTMI_BVH_MAX_DEPTH words per lane, 64 lanes
INDEXED = ["%s_indexed_%s_kernel" % (q, k) for q in ("trace_rays", "occluded") for k in ("linear", "shared_xy", "bvh", "mesh")]
ORDER = ["ray_order_box_kernel", "ray_order_keys_kernel", "ray_order_write_kernel"]
HIERARCHY = [k for k in INDEXED if "_bvh_" in k or "_mesh_" in k]


@pytest.fixture(scope="module")
def resources(tmp_path_factory):
    """{kernel: its figures} of the two units (tools/kernel_resources.py's compile and parse)"""
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    units = ["ptmi_query_indexed.hip", "ptmi_ray_order.hip"]
    asm = kr.assembly(out_dir=str(tmp_path_factory.mktemp("isa")), units=units)
    found = {}
    for unit in units:
        ks = kr.kernels_of(open(asm[unit]).read())
        for (name, body, code), demangled in zip(ks, kr.demangle([k[0] for k in ks])):
            get = lambda k: int(re.search(k + r" (\d+)", body).group(1))   # noqa: E731
            found[demangled] = {"unit": unit, "vgpr": get("next_free_vgpr"), "scratch": get("private_segment_fixed_size"), "lds": get("group_segment_fixed_size"),
                                "scratch_loads": len(re.findall(r"scratch_load", code)), "scratch_stores": len(re.findall(r"scratch_store", code)),
                                "sgpr_spill_lanes": len(re.findall(r"v_writelane_b32", code))}
    return found


def test_the_units_hold_these_kernels_and_no_name_other_tests_enumerate_by(resources, pkg):
    assert sorted(k for k, r in resources.items() if r["unit"] == "ptmi_query_indexed.hip") == sorted(INDEXED)
    assert sorted(k for k, r in resources.items() if r["unit"] == "ptmi_ray_order.hip") == sorted(ORDER)
    for name in resources:
        assert "refit" not in name and "mesh_build" not in name
    assert "ptmi_query_indexed.hip" in pkg._build.KERNEL_UNITS and "ptmi_ray_order.hip" in pkg._build.KERNEL_UNITS


@pytest.mark.parametrize("kernel", INDEXED + ORDER)
def test_no_kernel_of_either_unit_has_scratch(resources, kernel):
    r = resources[kernel]
    assert (r["scratch"], r["scratch_loads"], r["scratch_stores"], r["sgpr_spill_lanes"]) == (0, 0, 0, 0), (kernel, r)


@pytest.mark.parametrize("kernel", HIERARCHY)
def test_hierarchy_kernels_keep_four_waves_per_simd(resources, kernel):
    r = resources[kernel]
    assert r["vgpr"] <= 128 and r["lds"] == STACK_LDS, (kernel, r)


@pytest.mark.parametrize("kernel", [k for k in INDEXED if k not in HIERARCHY] + ORDER)
def test_the_other_kernels_hold_no_lds(resources, kernel):
    r = resources[kernel]
    assert r["lds"] == 0 and r["vgpr"] <= 128, (kernel, r)
