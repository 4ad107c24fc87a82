"""Register, scratch and LDS budgets of the nearest-primitive query's kernels (csrc/ptmi_nearest.hip; compiled here, no GPU needed), in the
style of tests/test_multi_hit_kernel_resources.py.  The unit holds one kernel per scene kind (linear, bvh, mesh).  A lane keeps its best
(key, idx) in two registers and asks the winner once more for its record; the hierarchies' kernels keep check_hit_bvh's LDS stack -- 24
words per lane -- as their only LDS and stay under the 128 VGPRs that four waves per SIMD allow; no kernel has scratch or a scalar spill."""
import importlib.util
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STACK_LDS = 24 * 64 * 4          # PTMI_BVH_MAX_DEPTH words per lane, 64 lanes
UNIT = "ptmi_nearest.hip"
KERNELS = ["nearest_%s_kernel" % k for k in ("linear", "bvh", "mesh")]
HIERARCHY = [k for k in KERNELS if "_bvh_" in k or "_mesh_" in k]


@pytest.fixture(scope="module")
def resources(tmp_path_factory):
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    asm = kr.assembly(out_dir=str(tmp_path_factory.mktemp("isa")), units=[UNIT])
    found = {}
    ks = kr.kernels_of(open(asm[UNIT]).read())
    for (name, body, code), demangled in zip(ks, kr.demangle([k[0] for k in ks])):
        get = lambda k: int(re.search(k + r" (\d+)", body).group(1))   # noqa: E731
        found[demangled] = {"vgpr": get("next_free_vgpr"), "scratch": get("private_segment_fixed_size"), "lds": get("group_segment_fixed_size"),
                            "dynamic_stack": get("uses_dynamic_stack"),
                            "scratch_loads": len(re.findall(r"scratch_load", code)), "scratch_stores": len(re.findall(r"scratch_store", code)),
                            "sgpr_spill_lanes": len(re.findall(r"v_writelane_b32", code))}
    print({k: (r["vgpr"], r["lds"]) for k, r in sorted(found.items())})
    return found


def test_the_unit_is_built_and_holds_exactly_these_kernels(resources, pkg):
    assert UNIT in pkg._build.KERNEL_UNITS and "ptmi_nearest.cpp" in pkg._build.HOST_SOURCES
    assert {"ptmi_nearest.h", "ptmi_nearest_device.h"} <= set(pkg._build.HEADERS)
    assert sorted(resources) == sorted(KERNELS)


@pytest.mark.parametrize("kernel", KERNELS)
def test_no_kernel_has_scratch_or_a_spill(resources, kernel):
    r = resources[kernel]
    assert (r["scratch"], r["scratch_loads"], r["scratch_stores"], r["sgpr_spill_lanes"], r["dynamic_stack"]) == (0, 0, 0, 0, 0), (kernel, r)
    assert r["vgpr"] <= 128, (kernel, r)


@pytest.mark.parametrize("kernel", KERNELS)
def test_static_lds_is_the_stack_column_alone(resources, kernel):
    assert resources[kernel]["lds"] == (STACK_LDS if kernel in HIERARCHY else 0), (kernel, resources[kernel])
