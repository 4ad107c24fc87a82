"""The stepped path entries' face in the header and the binding (no GPU needed): include/ptmi.h declares ptmi_bounce_rays_device,
ptmi_bounce_rays_indexed_device, ptmi_live_rays_bytes, ptmi_live_rays_device and ptmi_live_rays in a section behind "paths along a caller's
rays"; the section states the at-most-once and in-place rules; binding.SYMBOLS types them; there is no group form; and
Context.bounce_rays / Context.live_rays refuse tensors of the wrong dtype, shape, contiguity or residence with ValueError before anything
reaches the library -- shown with tests/test_ray_query_binding.py's stand-ins."""
import ctypes as C
import os
import re

import pytest

from test_abi import header_symbols
from test_ray_query_binding import FakeTensor, NoLibrary

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ptmi_bounce_rays_device", "ptmi_bounce_rays_indexed_device", "ptmi_live_rays_bytes", "ptmi_live_rays_device", "ptmi_live_rays")


@pytest.fixture()
def ctx(pkg):
    c = object.__new__(pkg.Context)          # no device: validation comes before the first use of the handle
    c._lib, c._h = NoLibrary(), None
    return c


def i32(*shape, **kw):
    return FakeTensor(shape, dtype="torch.int32", **kw)


def test_the_header_declares_and_the_binding_types_the_entry_points(pkg):
    raw = open(os.path.join(ROOT, "include", "ptmi.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    flat = re.sub(r"\s+", " ", text)
    assert ("int ptmi_bounce_rays_device(ptmi_ctx *ctx, float *d_rays , int n, float *d_throughput , float *d_radiance , uint32_t *d_seed , "
            "float *d_t, int32_t *d_idx, float *d_hit );") in flat
    assert ("int ptmi_bounce_rays_indexed_device(ptmi_ctx *ctx, float *d_rays, int n, const int32_t *d_index, int m, float *d_throughput, float *d_radiance, "
            "uint32_t *d_seed, float *d_t, int32_t *d_idx, float *d_hit);") in flat
    assert "size_t ptmi_live_rays_bytes(int count);" in flat
    assert ("int ptmi_live_rays_device(ptmi_ctx *ctx, const float *d_throughput , int n, const int32_t *d_index , int m, int32_t *d_live , int32_t *d_count , "
            "void *d_work, size_t work_bytes);") in flat
    assert "int ptmi_live_rays(const float *throughput, int n, const int32_t *index, int m, int32_t *live, int32_t *count);" in flat
    assert "#define PTMI_LIVE_RAYS_MAX (1 << 22)" in flat and pkg.binding.LIVE_RAYS_MAX == 1 << 22
    assert "#define PTMI_VERSION 600 " in raw
    for name in NAMES:
        assert name in pkg.SYMBOLS
    assert [len(pkg.SYMBOLS[name][1]) for name in NAMES] == [9, 11, 1, 9, 6]
    assert pkg.SYMBOLS["ptmi_live_rays_bytes"][0] is C.c_size_t and pkg.SYMBOLS["ptmi_live_rays_device"][1][-1] is C.c_size_t
    assert sorted(pkg.SYMBOLS) == header_symbols()
    assert not [n for n in pkg.SYMBOLS if n.startswith("ptmi_group_") and ("bounce" in n or "live_rays" in n)]       # no group form
    # behind the paths section, before the point queries
    assert text.index("int ptmi_trace_paths_indexed_device(") < text.index("int ptmi_bounce_rays_device(") < text.index("int ptmi_live_rays(") \
        < text.index("int ptmi_eval_distance_to_sphere(")
    assert raw.index("paths along a caller's rays") < raw.index("stepped paths: one bounce at a time")


def test_the_section_states_the_rules():
    text = open(os.path.join(ROOT, "include", "ptmi.h")).read()
    section = re.sub(r"\s+\*?\s*", " ", text[text.index("stepped paths: one bounce at a time"):text.index("int ptmi_bounce_rays_device(")])
    for phrase in ("AT MOST ONCE", "a ray named twice is a race", "IN PLACE: d_live may be the same array as d_index", "stable and deterministic", "GLASS",
                   "PTMI_ESTATE", "PTMI_EINVAL", "PTMI_ELIMIT", "no host synchronisation", "no device allocation", "4-byte alignment", "8-byte aligned",
                   "exactly one prepareRay", "a NaN throughput is not nearZero", "ray, radiance and seed keep every bit", "t 0, idx -1, six zeros",
                   "n == 0 or m == 0 is PTMI_OK", "Zero candidates is PTMI_OK", "There is no group form", "It needs no scene",
                   "none of which waits on another workgroup", "state planes, partition, camera and statistics are not touched",
                   "an entry outside [0, n) is skipped", "may each be NULL"):
        assert phrase in section, phrase


def state(n=5):
    return dict(rays=FakeTensor((n, 6)), seeds=i32(n, 4), throughput=FakeTensor((n, 3)), radiance=FakeTensor((n, 3)))


BAD = {
    "rays": [FakeTensor((5, 6), dtype="torch.float64"), i32(5, 6), FakeTensor((5, 6), contiguous=False), FakeTensor((5, 6), cuda=False), FakeTensor((30,)),
             FakeTensor((5, 3)), FakeTensor((6, 5)), FakeTensor((5, 6, 1))],
    "seeds": [i32(4, 4), i32(6, 4), i32(5, 3), i32(20), FakeTensor((5, 4)), FakeTensor((5, 4), dtype="torch.int64"), FakeTensor((5, 4), dtype="torch.int16"),
              i32(5, 4, contiguous=False), i32(5, 4, cuda=False)],
    "throughput": [FakeTensor((4, 3)), FakeTensor((5, 4)), FakeTensor((15,)), FakeTensor((5, 3), dtype="torch.float64"), FakeTensor((5, 3), contiguous=False),
                   FakeTensor((5, 3), cuda=False), FakeTensor((3, 5))],
}
BAD["radiance"] = BAD["throughput"]


@pytest.mark.parametrize("which", sorted(BAD))
def test_bounce_rays_refuses_state_of_the_wrong_kind(ctx, which):
    for bad in BAD[which]:
        with pytest.raises(ValueError):
            ctx.bounce_rays(**dict(state(), **{which: bad}))


def test_bounce_rays_refuses_an_index_and_outputs_of_the_wrong_kind(ctx):
    for bad in (FakeTensor((5,)), FakeTensor((5,), dtype="torch.int64"), i32(5, 1), i32(5, contiguous=False), i32(5, cuda=False)):
        with pytest.raises(ValueError):
            ctx.bounce_rays(index=bad, **state())
    t, idx, hit = FakeTensor((5,)), i32(5), FakeTensor((5, 6))
    for bad in ((t, idx), (t, idx, hit, hit), (FakeTensor((4,)), idx, hit), (t, FakeTensor((5,)), hit), (t, idx, FakeTensor((5, 3))), (i32(5), idx, hit),
                (t, idx, FakeTensor((5, 6), cuda=False)), (t, i32(5, contiguous=False), hit), (None, None, FakeTensor((6, 5)))):
        with pytest.raises(ValueError):
            ctx.bounce_rays(out=bad, **state())


def test_live_rays_refuses_tensors_of_the_wrong_kind(ctx):
    good = FakeTensor((5, 3))
    for bad in BAD["throughput"][1:]:
        with pytest.raises(ValueError):
            ctx.live_rays(bad)
    for bad in (FakeTensor((5,)), FakeTensor((5,), dtype="torch.int64"), i32(5, 1), i32(5, contiguous=False), i32(5, cuda=False)):
        with pytest.raises(ValueError):
            ctx.live_rays(good, index=bad)
    work = FakeTensor((4096,), dtype="torch.uint8")
    for bad in (i32(4), i32(6), FakeTensor((5,)), i32(5, cuda=False), i32(5, contiguous=False)):
        with pytest.raises(ValueError):
            ctx.live_rays(good, out=bad, work=work)
    with pytest.raises(ValueError):                                        # one entry per CANDIDATE
        ctx.live_rays(good, index=i32(3), out=i32(5), work=work)
    for bad in (i32(2), FakeTensor((1,)), i32(1, cuda=False), i32(1, 1)):
        with pytest.raises(ValueError):
            ctx.live_rays(good, count=bad, out=i32(5), work=work)
    for bad in (FakeTensor((4096,)), FakeTensor((4096,), dtype="torch.uint8", cuda=False), FakeTensor((64, 64), dtype="torch.uint8")):
        with pytest.raises(ValueError):
            ctx.live_rays(good, out=i32(5), work=bad)


def test_well_formed_tensors_reach_the_library(ctx):
    """... and only they: the stand-in library is asked for the entry point once validation has passed; both 4-byte integer dtypes serve"""
    for dtype in ("torch.int32", "torch.uint32"):
        st = dict(state(), seeds=FakeTensor((5, 4), dtype=dtype))
        with pytest.raises(AssertionError, match="ptmi_bounce_rays_device"):
            ctx.bounce_rays(**st)
        with pytest.raises(AssertionError, match="ptmi_bounce_rays_device"):
            ctx.bounce_rays(out=(None, i32(5), None), **st)
        with pytest.raises(AssertionError, match="ptmi_bounce_rays_indexed_device"):
            ctx.bounce_rays(index=i32(3), out=(FakeTensor((5,)), i32(5), FakeTensor((5, 6))), **st)
    with pytest.raises(AssertionError, match="ptmi_live_rays_bytes"):
        ctx.live_rays(FakeTensor((5, 3)), index=i32(3), out=i32(3), count=i32(1), work=FakeTensor((4096,), dtype="torch.uint8"))
