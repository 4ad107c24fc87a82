"""Register, scratch and LDS budgets of the mesh refit's kernels (ptmi_mesh_refit.hip; compiled here, no GPU needed), through
tools/kernel_resources.py as tests/test_mesh_kernel_resources.py pins the mesh render kernels (whose pinned tuples that test keeps): no
refit kernel touches scratch -- the f64 box arithmetic and both children of a node stay in registers -- and the two kernels that read
vertices stage one chunk of 256 triangles' 9 floats (9 216 bytes) in LDS."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_bvh_kernel_resources import resources  # noqa: E402,F401

CHUNK_LDS = 256 * 9 * 4
# kernel -> (VGPRs, scratch bytes, static LDS bytes, scratch loads, scratch stores), pinned to what the compiler gives
PINNED = {
    "mesh_refit_check_kernel": (39, 0, CHUNK_LDS, 0, 0),
    "mesh_refit_records_kernel": (20, 0, CHUNK_LDS, 0, 0),
    "mesh_refit_level_kernel": (50, 0, 0, 0, 0),
}


@pytest.mark.parametrize("kernel", sorted(PINNED))
def test_refit_kernel_resources_are_pinned(resources, kernel):  # noqa: F811
    assert kernel in resources, sorted(resources)
    r = resources[kernel]
    got = (r["vgpr"], r["scratch"], r["lds"], r["scratch_loads"], r["scratch_stores"])
    assert got == PINNED[kernel], (kernel, got)


def test_the_refit_unit_holds_these_kernels_and_no_others(resources):  # noqa: F811
    assert sorted(k for k in resources if "refit" in k) == sorted(PINNED)
