"""Register, scratch and LDS budgets of the kernels of the spatial sphere build (ptmi_bvh_lbvh.hip; compiled here, no GPU needed), through
tools/kernel_resources.py as tests/test_bvh_update_kernel_resources.py pins its siblings': no kernel touches scratch or a dynamic stack --
the f64 key arithmetic and the binary search stay in registers -- and the only LDS is the few words through which a workgroup's waves
add up and scan their counts."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_bvh_kernel_resources import resources  # noqa: E402,F401

# kernel -> (scratch bytes, static LDS bytes, scratch loads, scratch stores)
NEW = {
    "bvh_spatial_keys_kernel": (0, 0, 0, 0),
    "bvh_spatial_split_kernel": (0, 2 * 4 * 4, 0, 0),             # two sums over the workgroup's four waves
    "bvh_spatial_number_kernel": (0, 3 * 4 * 4, 0, 0),            # two sums and the scan's wave totals
    "bvh_spatial_finish_kernel": (0, 0, 0, 0),
}


@pytest.mark.parametrize("kernel", sorted(NEW))
def test_the_new_kernels_use_no_scratch_and_no_dynamic_stack(resources, kernel):  # noqa: F811
    assert kernel in resources, sorted(resources)
    r = resources[kernel]
    assert (r["scratch"], r["lds"], r["scratch_loads"], r["scratch_stores"]) == NEW[kernel], (kernel, r)
    assert r["vgpr"] <= 64 and r["sgpr_spill_lanes"] == 0, (kernel, r)            # the siblings' budget
    kr, out_dir = resources["__module__"], resources["__dir__"]
    text = open(os.path.join(out_dir, r["unit"].replace(".hip", ".s"))).read()
    body = [b for name, b, _ in kr.kernels_of(text) if name == r["mangled"]][0]
    assert ".amdhsa_uses_dynamic_stack 0" in body, kernel


def test_the_unit_holds_these_kernels_and_no_others(resources):  # noqa: F811
    assert sorted(k for k, r in resources.items() if isinstance(r, dict) and r.get("unit") == "ptmi_bvh_lbvh.hip") == sorted(NEW)
