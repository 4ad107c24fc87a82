"""The main loop of render_inline_kernel<true, 8>, cross-compiled here (no GPU), read for two things a compiler update or an edit of
check_hit could quietly take back (csrc/ptmi_device.h, profiles/four_cycle_ab.txt):
  * a whole-wave vote costs no vector instructions beyond its condition's own compare: no `v_cndmask_b32_e64 v, 0, 1, mask` feeding a
    `v_cmp_ne_u32` -- how __any / __all and the ballot of a two-term condition come out -- outside the candidate and fallback blocks;
  * the part of the sphere test that every lane runs at every sphere that shares its predecessor's cx and cy is at most 9 VALU
    instructions: lz, tca, d2 (seven two-cycle operations) and the two compares whose masks one s_and_b64 joins; x = r2 - d2 is the
    candidate path's."""
import importlib.util
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def main_loop(tmp_path_factory):
    """[(label, role, [instructions])] of the blocks of the kernel's main loop, as tools/isa_other.py cuts and names them"""
    kr, io = _load("kernel_resources"), _load("isa_other")
    out_dir = str(tmp_path_factory.mktemp("isa"))
    kr.assembly(out_dir=out_dir, units=["ptmi_inline.hip"])
    name, body = io.kernel_body("render_inline_kernelILb1ELi8EE", out_dir)
    blocks = io.blocks_of(body)
    heads = [h[0] for h in io.LOOPS.values() if h]
    header = max(set(heads), key=heads.count)
    found = []
    for label, code in blocks:
        loops = io.LOOPS.get(label, [])
        if loops and loops[0] == header:
            b = {"code": code, "valu": sum(1 for i in code if i.startswith("v_"))}
            found.append((label, io.role_of(b, len(loops) > 1), code))
    assert len(found) > 50
    return found


def test_no_vote_goes_through_a_vector_register(main_loop):
    allowed = {"sphere_candidate", "sqrt_slow", "division_fallback", "sincos_reduce", "sincos_polynomial"}
    bad = []
    for label, role, code in main_loop:
        if role in allowed:
            continue
        for k, ins in enumerate(code):
            m = re.match(r"v_cndmask_b32_e64 (v\d+), 0, 1, ", ins)
            if m and any(re.match(r"v_cmp_ne_u32\S* .*\b0, %s\b" % m.group(1), later) for later in code[k + 1:k + 6]):
                bad.append((label, role, ins))
    assert not bad, bad


def test_a_shared_spheres_hot_path_is_nine_vector_instructions(main_loop):
    tests = [(label, code) for label, role, code in main_loop if role == "sphere_test"]
    assert len(tests) >= 4, [label for label, _ in tests]               # the staged walk's four spheres a trip at least
    for label, code in tests:
        branch = next(k for k, ins in enumerate(code) if ins.startswith("s_cbranch"))
        hot = [ins for ins in code[:branch] if ins.startswith("v_")]
        assert len(hot) <= 9, (label, hot)
        assert sum(ins.startswith("v_cmp_") for ins in hot) == 2 and not any(ins.startswith(("v_min_f32", "v_cndmask")) for ins in hot), (label, hot)
        assert any(ins.startswith("s_and_b64") for ins in code[:branch]), (label, code[:branch])
