"""Register, scratch and LDS budgets of the device mesh build's kernels (ptmi_mesh_build.hip; compiled here, no GPU needed), through
tools/kernel_resources.py as tests/test_mesh_refit_kernel_resources.py pins the refit's: no build kernel touches scratch -- the f64 key
arithmetic stays in registers -- the three kernels that read triangles stage one chunk of 256 triangles' 15 floats (15 360 bytes) in
LDS, the sort's histogram and scan hold 256 words, its scatter 256 running positions and 4 x 256 wave counts."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_bvh_kernel_resources import resources  # noqa: E402,F401

CHUNK_LDS = 256 * 15 * 4
# kernel -> (VGPRs, scratch bytes, static LDS bytes, scratch loads, scratch stores), pinned to what the compiler gives
PINNED = {
    "mesh_build_check_kernel": (41, 0, CHUNK_LDS, 0, 0),
    "mesh_build_keys_kernel": (26, 0, CHUNK_LDS, 0, 0),
    "mesh_build_sort_histogram_kernel": (8, 0, 256 * 4, 0, 0),
    "mesh_build_sort_scan_kernel": (11, 0, 256 * 4, 0, 0),
    "mesh_build_sort_scatter_kernel": (22, 0, 5 * 256 * 4, 0, 0),
    "mesh_build_order_kernel": (7, 0, 0, 0, 0),
    "mesh_build_scatter_kernel": (22, 0, CHUNK_LDS, 0, 0),
}


@pytest.mark.parametrize("kernel", sorted(PINNED))
def test_build_kernel_resources_are_pinned(resources, kernel):  # noqa: F811
    assert kernel in resources, sorted(resources)
    r = resources[kernel]
    got = (r["vgpr"], r["scratch"], r["lds"], r["scratch_loads"], r["scratch_stores"])
    assert got == PINNED[kernel], (kernel, got)


def test_the_build_unit_holds_these_kernels_and_no_others(resources):  # noqa: F811
    assert sorted(k for k in resources if "mesh_build" in k) == sorted(PINNED)
