"""Register, scratch and LDS budgets of the kernels that move and replace a BVH scene's spheres (ptmi_bvh_refit.hip, ptmi_bvh_build.hip;
compiled here, no GPU needed), through tools/kernel_resources.py as tests/test_mesh_refit_kernel_resources.py pins the mesh refit's: no
kernel touches scratch or a dynamic stack -- the f64 box and key arithmetic stays in registers -- the check kernels stage one chunk of
256 spheres (4 or 10 floats each) in LDS.  The mesh build's kernels, whose sort the sphere build shares through one launcher, keep the
resources they had."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_bvh_kernel_resources import resources  # noqa: E402,F401
from test_mesh_build_kernel_resources import PINNED as MESH_BUILD  # noqa: E402

# kernel -> (scratch bytes, static LDS bytes, scratch loads, scratch stores)
NEW = {
    "bvh_check_kernel<4>": (0, 256 * 4 * 4, 0, 0),
    "bvh_check_kernel<10>": (0, 256 * 10 * 4, 0, 0),
    "bvh_records_kernel<4>": (0, 0, 0, 0),
    "bvh_records_kernel<10>": (0, 0, 0, 0),
    "bvh_level_kernel<4>": (0, 0, 0, 0),
    "bvh_level_kernel<10>": (0, 0, 0, 0),
    "bvh_build_keys_kernel": (0, 0, 0, 0),
    "bvh_build_order_kernel": (0, 0, 0, 0),
}


@pytest.mark.parametrize("kernel", sorted(NEW))
def test_the_new_kernels_use_no_scratch_and_no_dynamic_stack(resources, kernel):  # noqa: F811
    assert kernel in resources, sorted(resources)
    r = resources[kernel]
    assert (r["scratch"], r["lds"], r["scratch_loads"], r["scratch_stores"]) == NEW[kernel], (kernel, r)
    assert r["vgpr"] <= 64 and r["sgpr_spill_lanes"] == 0, (kernel, r)
    kr, out_dir = resources["__module__"], resources["__dir__"]
    text = open(os.path.join(out_dir, r["unit"].replace(".hip", ".s"))).read()
    body = [b for name, b, _ in kr.kernels_of(text) if name == r["mangled"]][0]
    assert ".amdhsa_uses_dynamic_stack 0" in body, kernel


def test_the_units_hold_these_kernels_and_no_others(resources):  # noqa: F811
    assert sorted(k for k, r in resources.items() if isinstance(r, dict) and r.get("unit") in ("ptmi_bvh_refit.hip", "ptmi_bvh_build.hip")) == sorted(NEW)


@pytest.mark.parametrize("kernel", sorted(MESH_BUILD))
def test_the_mesh_build_kernels_keep_their_resources(resources, kernel):  # noqa: F811
    r = resources[kernel]
    assert (r["vgpr"], r["scratch"], r["lds"], r["scratch_loads"], r["scratch_stores"]) == MESH_BUILD[kernel], (kernel, r)
