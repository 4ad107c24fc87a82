"""The multi-hit query's face in the header and the binding (no GPU needed): include/ptmi.h declares ptmi_trace_rays_multi_device and
ptmi_trace_rays_multi_indexed_device behind the ray order's section and states the specification, binding.SYMBOLS types both, there is no
group form, and Context.trace_rays_multi refuses a wrong k and tensors of the wrong dtype, contiguity or shape with ValueError before
anything reaches the library -- shown with test_ray_query_binding.py's stand-ins."""
import os
import re

import pytest

from test_ray_query_binding import FakeTensor, NoLibrary

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ptmi_trace_rays_multi_device", "ptmi_trace_rays_multi_indexed_device")


@pytest.fixture()
def ctx(pkg):
    c = object.__new__(pkg.Context)          # no device: validation comes before the first use of the handle
    c._lib, c._h = NoLibrary(), None
    return c


def header():
    return open(os.path.join(ROOT, "include", "ptmi.h")).read()


def test_the_header_declares_and_the_binding_types_the_two_entry_points(pkg):
    text = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", header(), flags=re.S))
    assert "#define PTMI_MULTI_HIT_MAX 16" in text
    assert ("int ptmi_trace_rays_multi_device(ptmi_ctx *ctx, const float *d_rays , const float *d_t_max , int n, int k, float *d_t , "
            "int32_t *d_idx , int32_t *d_count );") in text
    assert ("int ptmi_trace_rays_multi_indexed_device(ptmi_ctx *ctx, const float *d_rays, const float *d_t_max, int n, const int32_t *d_index, "
            "int m, int k, float *d_t, int32_t *d_idx, int32_t *d_count);") in text
    for name in NAMES:
        assert name in pkg.SYMBOLS
    assert len(pkg.SYMBOLS[NAMES[0]][1]) == 8 and len(pkg.SYMBOLS[NAMES[1]][1]) == 10
    assert not [n for n in pkg.SYMBOLS if n.startswith("ptmi_group_") and "multi" in n]       # no group form
    assert pkg.MULTI_HIT_MAX == pkg.binding.MULTI_HIT_MAX == 16
    assert "#define PTMI_VERSION 600 " in header()                                           # the version other tests pin is not moved


def test_the_section_sits_behind_the_ray_order_and_states_the_specification():
    text = header()
    assert text.index("ray order and ray queries through an index") < text.index("multi-hit: the k nearest hits") < text.index("paths along a caller's rays")
    section = text[text.index("multi-hit: the k nearest hits"):text.index("int ptmi_trace_rays_multi_device(")]
    for phrase in ("one binary32 compare", "ALL primitives", "at most one hit", "entry point only", "min(k, |H|)", "ascending by (t, j)",
                   "lower primitive index first", "t = 0 and idx = -1", "NaN or non-positive t_max", "ptmi_trace_rays_device's (t, idx)",
                   "ptmi_occluded_device", "outside [0, n) is skipped", "left untouched", "PTMI_ESTATE", "PTMI_EINVAL", "k < 1", "PTMI_ELIMIT",
                   "PTMI_MULTI_HIT_MAX", "d_t_max may be NULL", "n == 0 or m == 0 is PTMI_OK", "no group form"):
        assert phrase in section, phrase


BAD_RAYS = [FakeTensor((5, 6), dtype="torch.float64"), FakeTensor((5, 6), dtype="torch.int32"), FakeTensor((5, 6), contiguous=False),
            FakeTensor((5, 6), cuda=False), FakeTensor((30,)), FakeTensor((5, 3)), FakeTensor((6, 5)), FakeTensor((5, 6, 1))]


def good(n=5, k=4):
    return FakeTensor((n, k)), FakeTensor((n, k), dtype="torch.int32"), FakeTensor((n,), dtype="torch.int32")


@pytest.mark.parametrize("rays", BAD_RAYS, ids=lambda t: "%s-%s" % (t.dtype, "x".join(map(str, t.shape))))
def test_rays_of_the_wrong_kind_are_refused(ctx, rays):
    with pytest.raises(ValueError):
        ctx.trace_rays_multi(rays, 4, out=good())


@pytest.mark.parametrize("k", [0, -1, 17, 1 << 20, 2.0, "4", None, True])
def test_a_k_outside_the_limits_or_of_another_type_is_refused(ctx, k):
    with pytest.raises(ValueError):
        ctx.trace_rays_multi(FakeTensor((5, 6)), k, out=good())


def test_outputs_t_max_and_index_of_the_wrong_kind_are_refused(ctx):
    rays = FakeTensor((5, 6))
    t, idx, count = good()
    for out in ((FakeTensor((5, 3)), idx, count), (FakeTensor((4, 4)), idx, count), (FakeTensor((20,)), idx, count), (t, FakeTensor((5, 4)), count),
                (t, FakeTensor((5, 4), dtype="torch.int64"), count), (t, idx, FakeTensor((5,))), (t, idx, FakeTensor((5, 1), dtype="torch.int32")),
                (t, idx, FakeTensor((4,), dtype="torch.int32")), (FakeTensor((5, 4), contiguous=False), idx, count),
                (t, FakeTensor((5, 4), dtype="torch.int32", contiguous=False), count), (t, idx, FakeTensor((5,), dtype="torch.int32", cuda=False)),
                (t, idx), (t, idx, count, count)):
        with pytest.raises(ValueError):
            ctx.trace_rays_multi(rays, 4, out=out)
    with pytest.raises(ValueError):
        ctx.trace_rays_multi(rays, 5, out=(t, idx, count))                      # rows of another k
    for t_max in (FakeTensor((4,)), FakeTensor((5, 1)), FakeTensor((5,), dtype="torch.float64"), FakeTensor((5,), contiguous=False), FakeTensor((5,), cuda=False)):
        with pytest.raises(ValueError):
            ctx.trace_rays_multi(rays, 4, t_max=t_max, out=(t, idx, count))
    for index in (FakeTensor((3,)), FakeTensor((3, 1), dtype="torch.int32"), FakeTensor((3,), dtype="torch.int32", contiguous=False),
                  FakeTensor((3,), dtype="torch.int32", cuda=False)):
        with pytest.raises(ValueError):
            ctx.trace_rays_multi(rays, 4, out=(t, idx, count), index=index)


def test_well_formed_tensors_reach_the_library(ctx):
    """... and only they: the stand-in library is asked for the entry point once validation has passed"""
    rays = FakeTensor((5, 6))
    for k in (1, 4, 16):
        with pytest.raises(AssertionError, match="ptmi_trace_rays_multi_device"):
            ctx.trace_rays_multi(rays, k, out=good(5, k))
        with pytest.raises(AssertionError, match="ptmi_trace_rays_multi_device"):
            ctx.trace_rays_multi(rays, k, t_max=FakeTensor((5,)), out=good(5, k))
        with pytest.raises(AssertionError, match="ptmi_trace_rays_multi_indexed_device"):
            ctx.trace_rays_multi(rays, k, out=good(5, k), index=FakeTensor((3,), dtype="torch.int32"))
