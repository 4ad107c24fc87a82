"""The budgets of render_inline_kernel_plain (compiled here, no GPU needed): render Inline for a scene staged in LDS in which no sphere
shares its predecessor's cx and cy -- the launcher's choice when the scene's mask is 0 (csrc/ptmi_inline.hip, launch_linear).  It is the kernel
render_inline_kernel<true, .> was before the sharing, so it holds that kernel's row of tests/test_kernel_resources.py: 7 waves per SIMD."""
import pytest

from test_kernel_resources import resources  # noqa: F401  (the module's fixture: every kernel's resources, compiled once)

BUDGETS = {
    "render_inline_kernel_plain<8>": (72, 32, 2560, 4, 4),
    "render_inline_kernel_plain<0>": (72, 32, 2560, 4, 4),
}


@pytest.mark.parametrize("kernel", sorted(BUDGETS))
def test_the_plain_inline_kernel_stays_within_the_inline_budget(resources, kernel):  # noqa: F811
    assert kernel in resources, sorted(resources)
    vgpr, scratch, lds, loads, stores = BUDGETS[kernel]
    r = resources[kernel]
    assert r["vgpr"] <= vgpr and r["scratch"] <= scratch and r["lds"] <= lds, r
    assert r["scratch_loads"] <= loads and r["scratch_stores"] <= stores, r
