"""Register, scratch and LDS budgets of the mesh scenes' kernels (compiled here, no GPU needed), pinned as
tests/test_bvh_kernel_resources.py pins the BVH ones.  Both hierarchies are walked on the one LDS stack of PTMI_BVH_MAX_DEPTH words per
lane; the only scratch of the Inline and Streams-chain kernels is the 16-byte frame of the literal fold (check_hit_mesh_exact, not
inlined: it calls check_hit_exact), and no traversal loop -- of the sphere walk or of the triangle walk -- touches scratch."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_bvh_kernel_resources import STACK_LDS, resources, traversal_loops  # noqa: E402,F401

PINNED = {
    "render_inline_mesh_kernel<8>": (105, 16, 2560 + STACK_LDS, 0, 0),         # 4 waves/SIMD by registers and by LDS (PTMI_BVH_WAVES)
    "render_inline_mesh_kernel<0>": (105, 16, 2560 + STACK_LDS, 0, 0),
    "render_streams_mesh_kernel<8>": (104, 16, 2816 + STACK_LDS, 0, 0),
    "render_streams_mesh_kernel<0>": (104, 16, 2816 + STACK_LDS, 0, 0),
    "render_streams_tree_mesh_kernel<8>": (113, 704, 5120 + STACK_LDS, 0, 4),  # the tree walk's deeper waiting children, as its twins
    "render_streams_tree_mesh_kernel<0>": (113, 704, 5120 + STACK_LDS, 0, 4),
    "eval_check_hit_mesh_kernel": (65, 16, STACK_LDS, 0, 0),
}


@pytest.mark.parametrize("kernel", sorted(PINNED))
def test_mesh_kernel_resources_are_pinned(resources, kernel):  # noqa: F811
    assert kernel in resources, sorted(resources)
    r = resources[kernel]
    got = (r["vgpr"], r["scratch"], r["lds"], r["scratch_loads"], r["scratch_stores"])
    assert got == PINNED[kernel], (kernel, got)


@pytest.mark.parametrize("unit, kernel", [("ptmi_inline", "render_inline_mesh_kernel<8>"), ("ptmi_streams_chain", "render_streams_mesh_kernel<8>"),
                                          ("ptmi_streams_tree", "render_streams_tree_mesh_kernel<8>"), ("ptmi_small", "eval_check_hit_mesh_kernel")])
def test_no_scratch_access_inside_either_traversal_loop(resources, unit, kernel):  # noqa: F811
    kr, out_dir = resources["__module__"], resources["__dir__"]
    text = open(os.path.join(out_dir, unit + ".s")).read()
    ks = kr.kernels_of(text)
    codes = {dem: code for (name, body, code), dem in zip(ks, kr.demangle([k[0] for k in ks]))}
    loops = traversal_loops(codes[kernel])
    assert len(loops) >= 2, (kernel, len(loops))                 # the sphere walk and the triangle walk
    for body in loops:
        assert any("ds_write_b32" in l for l in body) and any("ds_read_b32" in l for l in body), "the LDS stack is in the loop"
        assert not [l for l in body if "scratch_" in l], kernel
