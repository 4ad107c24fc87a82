"""Register, scratch and LDS budgets of the BVH scenes' kernels (compiled here, no GPU needed), pinned as tests/test_kernel_resources.py
pins the others.  The hierarchy's traversal stack lives in LDS (one column of PTMI_BVH_MAX_DEPTH words per lane), so the Inline and
Streams-chain kernels have no scratch at all, and in every BVH kernel the traversal loops hold no scratch access.  The tree walk keeps
its deeper waiting children in scratch, as its linear twin does, outside those loops."""
import importlib.util
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def resources(tmp_path_factory):
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    out_dir = str(tmp_path_factory.mktemp("isa"))
    found = mod.collect(out_dir=out_dir)
    found["__module__"], found["__dir__"] = mod, out_dir
    return found


STACK_LDS = 24 * 64 * 4          # PTMI_BVH_MAX_DEPTH words per lane, 64 lanes
# kernel -> (VGPRs, scratch bytes, static LDS bytes, scratch loads, scratch stores), pinned: a change of any of them is a change of the
# BVH kernels' occupancy and must be seen here
PINNED = {
    "render_inline_bvh_kernel<8>": (93, 0, 2560 + STACK_LDS, 0, 0),          # 5 waves/SIMD by registers; LDS (8.5 KB per wave) allows 4
    "render_inline_bvh_kernel<0>": (93, 0, 2560 + STACK_LDS, 0, 0),
    "render_streams_bvh_kernel<8>": (92, 0, 2816 + STACK_LDS, 0, 0),
    "render_streams_bvh_kernel<0>": (92, 0, 2816 + STACK_LDS, 0, 0),
    "render_streams_tree_bvh_kernel<8>": (97, 688, 5120 + STACK_LDS, 0, 4),  # scratch: the tree walk's deeper waiting children (below)
    "render_streams_tree_bvh_kernel<0>": (97, 688, 5120 + STACK_LDS, 0, 4),
    "eval_check_hit_kernel<true>": (65, 0, STACK_LDS, 0, 0),
}


@pytest.mark.parametrize("kernel", sorted(PINNED))
def test_bvh_kernel_resources_are_pinned(resources, kernel):
    assert kernel in resources, sorted(resources)
    r = resources[kernel]
    got = (r["vgpr"], r["scratch"], r["lds"], r["scratch_loads"], r["scratch_stores"])
    assert got == PINNED[kernel], (kernel, got)


def traversal_loops(code):
    """The traversal loops of a kernel, from the loop structure the compiler writes beside every block (`in Loop: Header=BBx_y`, `Parent
    Loop`): for every fetch of a node's last 16 bytes (`global_load_dwordx4 ... offset:48`), all lines of the innermost loop around it,
    nested loops (the leaf's sphere tests) included.  Blocks of one loop need not be contiguous."""
    blocks, parent, cur = [], {}, None
    for line in code.split("\n"):
        head = re.match(r"^\s*(?:\.L(BB\d+_\d+)|; %bb\.\d+):", line)
        if head:
            cur = {"name": head.group(1), "header": None, "lines": []}
            blocks.append(cur)
        if cur is None:
            continue
        m = re.search(r"in Loop: Header=(BB\d+_\d+)", line)
        if m:
            cur["header"] = m.group(1)
        if "Loop Header:" in line and cur["name"]:
            cur["header"] = cur["name"]
        m = re.search(r"Parent Loop (BB\d+_\d+)", line)
        if m and cur["name"]:
            parent[cur["name"]] = m.group(1)
        cur["lines"].append(line)

    def within(h, loop):
        while h is not None:
            if h == loop:
                return True
            h = parent.get(h)
        return False
    found = []
    for blk in blocks:
        if any("global_load_dwordx4" in l and "offset:48" in l for l in blk["lines"]):
            assert blk["header"], "node fetch outside any loop"
            found.append([l for b in blocks if within(b["header"], blk["header"]) for l in b["lines"]])
    return found


@pytest.mark.parametrize("unit, kernel", [("ptmi_inline", "render_inline_bvh_kernel<8>"), ("ptmi_streams_chain", "render_streams_bvh_kernel<8>"),
                                          ("ptmi_streams_tree", "render_streams_tree_bvh_kernel<8>"), ("ptmi_streams_tree", "render_streams_tree_bvh_kernel<0>")])
def test_no_scratch_access_inside_the_traversal_loop(resources, kernel, unit):
    """The stack is in LDS: no scratch load or store inside any traversal loop (the tree walk's scratch -- its deeper waiting children
    -- is touched outside them)."""
    kr, out_dir = resources["__module__"], resources["__dir__"]
    text = open(os.path.join(out_dir, unit + ".s")).read()
    ks = kr.kernels_of(text)
    codes = {dem: code for (name, body, code), dem in zip(ks, kr.demangle([k[0] for k in ks]))}
    loops = traversal_loops(codes[kernel])
    assert loops, kernel
    for body in loops:
        assert any("ds_write_b32" in l for l in body) and any("ds_read_b32" in l for l in body), "the LDS stack is in the loop"
        assert not [l for l in body if "scratch_" in l], kernel
