"""The Streams ray entries' face in the header and the binding (no GPU needed): include/ptmi.h declares ptmi_trace_streams_bytes,
ptmi_trace_streams_device and ptmi_trace_streams_indexed_device, binding.SYMBOLS types them, the section states the contract, the workspace
and d_lost rules and the refusals, and Context.trace_streams refuses tensors of the wrong dtype, contiguity, shape or device with ValueError
before anything reaches the library -- shown with tests/test_ray_query_binding.py's stand-ins."""
import os
import re

import pytest

from test_ray_query_binding import FakeTensor, NoLibrary

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ptmi_trace_streams_bytes", "ptmi_trace_streams_device", "ptmi_trace_streams_indexed_device")


@pytest.fixture()
def ctx(pkg):
    c = object.__new__(pkg.Context)          # no device: validation comes before the first use of the handle
    c._lib, c._h = NoLibrary(), None
    return c


def seeds(n=5, dtype="torch.int32", **kw):
    return FakeTensor((n, 4), dtype=dtype, **kw)


def work(n=1 << 14, **kw):
    kw.setdefault("dtype", "torch.uint8")
    return FakeTensor((n,), **kw)


def test_the_header_declares_and_the_binding_types_the_three_entry_points(pkg):
    raw = open(os.path.join(ROOT, "include", "ptmi.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    flat = re.sub(r"\s+", " ", text)
    assert "size_t ptmi_trace_streams_bytes(int count);" in flat
    assert ("int ptmi_trace_streams_device(ptmi_ctx *ctx, const float *d_rays , int n, int n_spp, float *d_color , uint32_t *d_seed , uint64_t *d_lost , "
            "void *d_work, size_t work_bytes);") in flat
    assert ("int ptmi_trace_streams_indexed_device(ptmi_ctx *ctx, const float *d_rays, int n, const int32_t *d_index, int m, int n_spp, "
            "float *d_color, uint32_t *d_seed, uint64_t *d_lost, void *d_work, size_t work_bytes);") in flat
    for name in NAMES:
        assert name in pkg.SYMBOLS
    assert [len(pkg.SYMBOLS[name][1]) for name in NAMES] == [1, 9, 11]
    assert not [n for n in pkg.SYMBOLS if n.startswith("ptmi_group_") and "streams" in n and "trace" in n]       # no group form
    assert "#define PTMI_VERSION 600 " in raw
    # the new section stands after the stepped paths and before the point queries; the Inline sections keep their GLASS refusal
    assert text.index("int ptmi_live_rays(") < text.index("size_t ptmi_trace_streams_bytes(") < text.index("int ptmi_eval_distance_to_sphere(")
    assert raw.index("stepped paths: one bounce at a time") < raw.index("render Streams along a caller's rays") < raw.index("point queries (the reference's")
    assert "render Inline cannot split rays" in raw[raw.index("paths along a caller's rays"):raw.index("int ptmi_path_seeds_device(")]


def test_the_section_states_the_contract_the_workspace_and_the_refusals():
    text = open(os.path.join(ROOT, "include", "ptmi.h")).read()
    section = text[text.index("render Streams along a caller's rays"):text.index("size_t ptmi_trace_streams_bytes(")]
    section = re.sub(r"\s+", " ", re.sub(r"\n \*", "\n", section))          # (the comment's margin goes, a product's star stays)
    for phrase in ("no bounce limit", "PTMI_OPT_STREAM_STEP_CAP", "PTMI_OPT_STREAMS_SEED_RULE", "no host synchronisation", "no device allocation", "4-byte alignment",
                   "dispatch order and ptmi_stats are not touched", "acc = acc + emittance * throughput", "pixel_seed = the seed cur carried INTO this hit",
                   "waits on a stack of 16", "dropped and counted", "cut and counted (truncated)", "updateSeed", "PTMI_SEED_AUTO gives PTMI_SEED_FROM_RESULT without GLASS",
                   "PTMI_FORM_PIXEL", "all seven planes bit for bit", "one call of n_spp samples equals n_spp calls of one", "8-byte aligned", "ADDED to",
                   "one atomic add per wave", "16-byte aligned", "ptmi_trace_streams_bytes(lanes)", "without GLASS it is ignored and may be NULL",
                   "lanes is m with an index, else n", "an entry outside [0, n) is skipped", "AT MOST ONCE", "PTMI_ESTATE", "PTMI_EINVAL",
                   "explicit PTMI_SEED_FROM_RESULT", "n == 0, m == 0 or n_spp <= 0 is PTMI_OK and touches nothing", "no group form"):
        assert phrase in section, phrase


BAD_RAYS = [FakeTensor((5, 6), dtype="torch.float64"), FakeTensor((5, 6), dtype="torch.int32"), FakeTensor((5, 6), contiguous=False),
            FakeTensor((5, 6), cuda=False), FakeTensor((30,)), FakeTensor((5, 3)), FakeTensor((6, 5)), FakeTensor((5, 6, 1))]


@pytest.mark.parametrize("rays", BAD_RAYS, ids=lambda t: "%s-%s" % (t.dtype, "x".join(map(str, t.shape))))
def test_rays_of_the_wrong_kind_are_refused(ctx, rays):
    with pytest.raises(ValueError):
        ctx.trace_streams(rays, seeds(), color=FakeTensor((5, 3)), work=work())


def test_seeds_colour_index_lost_and_work_of_the_wrong_kind_are_refused(ctx):
    rays, color = FakeTensor((5, 6)), FakeTensor((5, 3))
    for bad in (seeds(4), seeds(6), FakeTensor((5, 3), dtype="torch.int32"), FakeTensor((20,), dtype="torch.int32"), seeds(dtype="torch.float32"),
                seeds(dtype="torch.int64"), seeds(dtype="torch.int16"), seeds(contiguous=False), seeds(cuda=False), FakeTensor((4, 5), dtype="torch.int32")):
        with pytest.raises(ValueError):
            ctx.trace_streams(rays, bad, color=color, work=work())
    for bad in (FakeTensor((4, 3)), FakeTensor((5, 4)), FakeTensor((15,)), FakeTensor((5, 3), dtype="torch.float64"), FakeTensor((5, 3), contiguous=False),
                FakeTensor((5, 3), cuda=False), FakeTensor((3, 5))):
        with pytest.raises(ValueError):
            ctx.trace_streams(rays, seeds(), color=bad, work=work())
    for bad in (FakeTensor((5,)), FakeTensor((5,), dtype="torch.int64"), FakeTensor((5, 1), dtype="torch.int32"), FakeTensor((5,), dtype="torch.int32", contiguous=False),
                FakeTensor((5,), dtype="torch.int32", cuda=False)):
        with pytest.raises(ValueError):
            ctx.trace_streams(rays, seeds(), color=color, index=bad, work=work())
    for bad in (FakeTensor((2,), dtype="torch.int32"), FakeTensor((2,), dtype="torch.float64"), FakeTensor((1,), dtype="torch.int64"), FakeTensor((3,), dtype="torch.int64"),
                FakeTensor((2, 1), dtype="torch.int64"), FakeTensor((2,), dtype="torch.int64", contiguous=False), FakeTensor((2,), dtype="torch.int64", cuda=False)):
        with pytest.raises(ValueError):
            ctx.trace_streams(rays, seeds(), color=color, lost=bad, work=work())
    for bad in (work(dtype="torch.float32"), work(dtype="torch.int8"), FakeTensor((4, 4096), dtype="torch.uint8"), work(contiguous=False), work(cuda=False)):
        with pytest.raises(ValueError):
            ctx.trace_streams(rays, seeds(), color=color, work=bad)


def test_well_formed_tensors_reach_the_library(ctx):
    """... and only they: the stand-in library is asked for the entry point once validation has passed; both 4-byte integer dtypes serve.
    Without a workspace the binding first asks how large one must be."""
    rays, color, lost = FakeTensor((5, 6)), FakeTensor((5, 3)), FakeTensor((2,), dtype="torch.int64")
    for dtype in ("torch.int32", "torch.uint32"):
        with pytest.raises(AssertionError, match="ptmi_trace_streams_device"):
            ctx.trace_streams(rays, seeds(dtype=dtype), spp=2, color=color, lost=lost, work=work())
        with pytest.raises(AssertionError, match="ptmi_trace_streams_indexed_device"):
            ctx.trace_streams(rays, seeds(dtype=dtype), color=color, index=FakeTensor((3,), dtype="torch.int32"), work=work())
    with pytest.raises(AssertionError, match="ptmi_trace_streams_bytes"):
        ctx.trace_streams(rays, seeds(), color=color)
    with pytest.raises(AssertionError, match="ptmi_trace_streams_bytes"):
        ctx.trace_streams_bytes(64)
    # nothing to do: no call at all
    assert ctx.trace_streams(rays, seeds(), spp=0, color=color) is color
    assert ctx.trace_streams(rays, seeds(), color=color, index=FakeTensor((0,), dtype="torch.int32")) is color
