"""The path entries' face in the header and the binding (no GPU needed): include/ptmi.h declares ptmi_path_seeds_device,
ptmi_trace_paths_device and ptmi_trace_paths_indexed_device, binding.SYMBOLS types them, the section states the index-once rule and the
GLASS refusal, and Context.trace_paths / Context.path_seeds refuse tensors of the wrong dtype, contiguity or shape with ValueError before
anything reaches the library -- shown with tests/test_ray_query_binding.py's stand-ins."""
import os
import re

import pytest

from test_ray_query_binding import FakeTensor, NoLibrary

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ptmi_path_seeds_device", "ptmi_trace_paths_device", "ptmi_trace_paths_indexed_device")


@pytest.fixture()
def ctx(pkg):
    c = object.__new__(pkg.Context)          # no device: validation comes before the first use of the handle
    c._lib, c._h = NoLibrary(), None
    return c


def seeds(n=5, dtype="torch.int32", **kw):
    return FakeTensor((n, 4), dtype=dtype, **kw)


def test_the_header_declares_and_the_binding_types_the_three_entry_points(pkg):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ptmi.h")).read(), flags=re.S)
    flat = re.sub(r"\s+", " ", text)
    assert "int ptmi_path_seeds_device(ptmi_ctx *ctx, uint64_t seed0, uint64_t first_index, int n, uint32_t *d_seed );" in flat
    assert "int ptmi_trace_paths_device(ptmi_ctx *ctx, const float *d_rays , int n, int bounce_limit, int n_spp, float *d_color , uint32_t *d_seed );" in flat
    assert ("int ptmi_trace_paths_indexed_device(ptmi_ctx *ctx, const float *d_rays, int n, const int32_t *d_index, int m, int bounce_limit, int n_spp, "
            "float *d_color, uint32_t *d_seed);") in flat
    for name in NAMES:
        assert name in pkg.SYMBOLS
    assert [len(pkg.SYMBOLS[name][1]) for name in NAMES] == [5, 7, 9]
    assert not [n for n in pkg.SYMBOLS if n.startswith("ptmi_group_") and "path" in n]       # no group form
    assert "#define PTMI_VERSION 600 " in open(os.path.join(ROOT, "include", "ptmi.h")).read()
    assert text.index("int ptmi_occluded_indexed_device(") < text.index("int ptmi_path_seeds_device(") < text.index("int ptmi_eval_distance_to_sphere(")


def test_the_section_states_the_index_once_rule_the_glass_refusal_and_the_degenerate_arguments():
    text = open(os.path.join(ROOT, "include", "ptmi.h")).read()
    section = re.sub(r"\s+\*?\s*", " ", text[text.index("paths along a caller's rays"):text.index("int ptmi_path_seeds_device(")])
    for phrase in ("AT MOST ONCE", "a ray named twice is a race", "GLASS", "PTMI_ESTATE", "PTMI_EINVAL", "no host synchronisation", "4-byte alignment",
                   "color_i = new + color_i", "bounce_limit <= 0", "n_spp <= 0 or n == 0 is PTMI_OK", "m == 0 is PTMI_OK", "no group form",
                   "state planes, partition, camera and statistics are not touched", "an entry outside [0, n) is skipped"):
        assert phrase in section, phrase


BAD_RAYS = [FakeTensor((5, 6), dtype="torch.float64"), FakeTensor((5, 6), dtype="torch.int32"), FakeTensor((5, 6), contiguous=False),
            FakeTensor((5, 6), cuda=False), FakeTensor((30,)), FakeTensor((5, 3)), FakeTensor((6, 5)), FakeTensor((5, 6, 1))]


@pytest.mark.parametrize("rays", BAD_RAYS, ids=lambda t: "%s-%s" % (t.dtype, "x".join(map(str, t.shape))))
def test_rays_of_the_wrong_kind_are_refused(ctx, rays):
    with pytest.raises(ValueError):
        ctx.trace_paths(rays, seeds(), 4, color=FakeTensor((5, 3)))


def test_seeds_colour_and_index_of_the_wrong_kind_are_refused(ctx):
    rays, color = FakeTensor((5, 6)), FakeTensor((5, 3))
    for bad in (seeds(4), seeds(6), FakeTensor((5, 3), dtype="torch.int32"), FakeTensor((20,), dtype="torch.int32"), seeds(dtype="torch.float32"),
                seeds(dtype="torch.int64"), seeds(dtype="torch.int16"), seeds(contiguous=False), seeds(cuda=False), FakeTensor((4, 5), dtype="torch.int32")):
        with pytest.raises(ValueError):
            ctx.trace_paths(rays, bad, 4, color=color)
    for bad in (FakeTensor((4, 3)), FakeTensor((5, 4)), FakeTensor((15,)), FakeTensor((5, 3), dtype="torch.float64"), FakeTensor((5, 3), contiguous=False),
                FakeTensor((5, 3), cuda=False), FakeTensor((3, 5))):
        with pytest.raises(ValueError):
            ctx.trace_paths(rays, seeds(), 4, color=bad)
    for bad in (FakeTensor((5,)), FakeTensor((5,), dtype="torch.int64"), FakeTensor((5, 1), dtype="torch.int32"), FakeTensor((5,), dtype="torch.int32", contiguous=False),
                FakeTensor((5,), dtype="torch.int32", cuda=False)):
        with pytest.raises(ValueError):
            ctx.trace_paths(rays, seeds(), 4, color=color, index=bad)


def test_path_seeds_refuses_an_output_of_the_wrong_kind(ctx):
    for bad in (seeds(4), FakeTensor((5, 3), dtype="torch.int32"), seeds(dtype="torch.float32"), seeds(dtype="torch.int64"), seeds(contiguous=False), seeds(cuda=False)):
        with pytest.raises(ValueError):
            ctx.path_seeds(1, 5, out=bad)
    with pytest.raises(ValueError):
        ctx.path_seeds(1, -1, out=seeds())
    with pytest.raises(ValueError):
        ctx.path_seeds(1, 5, first_index=-2, out=seeds())


def test_well_formed_tensors_reach_the_library(ctx):
    """... and only they: the stand-in library is asked for the entry point once validation has passed; both 4-byte integer dtypes serve"""
    rays, color = FakeTensor((5, 6)), FakeTensor((5, 3))
    for dtype in ("torch.int32", "torch.uint32"):
        with pytest.raises(AssertionError, match="ptmi_trace_paths_device"):
            ctx.trace_paths(rays, seeds(dtype=dtype), 4, spp=2, color=color)
        with pytest.raises(AssertionError, match="ptmi_trace_paths_indexed_device"):
            ctx.trace_paths(rays, seeds(dtype=dtype), 4, color=color, index=FakeTensor((3,), dtype="torch.int32"))
        with pytest.raises(AssertionError, match="ptmi_path_seeds_device"):
            ctx.path_seeds(0x5EED1234, 5, first_index=7, out=seeds(dtype=dtype))
