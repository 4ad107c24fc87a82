"""The ray queries' face in the header and the binding (no GPU needed): include/ptmi.h declares ptmi_trace_rays_device and
ptmi_occluded_device, binding.SYMBOLS types them, and Context.trace_rays / Context.occluded refuse tensors of the wrong dtype, contiguity
or shape with ValueError before anything reaches the library -- shown with a stand-in that has a tensor's is_cuda, is_contiguous, dtype,
shape, numel and data_ptr."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ptmi_trace_rays_device", "ptmi_occluded_device")


class FakeTensor:
    def __init__(self, shape, dtype="torch.float32", cuda=True, contiguous=True):
        self.shape, self.dtype, self.is_cuda, self._contiguous = tuple(shape), dtype, cuda, contiguous
        self.device = "cuda:0"

    def is_contiguous(self):
        return self._contiguous

    def numel(self):
        n = 1
        for s in self.shape:
            n *= s
        return n

    def data_ptr(self):
        return 0x1000


class NoLibrary:
    """Stands where the library handle would: any call through it is a test failure"""

    def __getattr__(self, name):
        raise AssertionError("the binding called %s with arguments it should have refused" % name)


@pytest.fixture()
def ctx(pkg):
    c = object.__new__(pkg.Context)          # no device: validation comes before the first use of the handle
    c._lib, c._h = NoLibrary(), None
    return c


def test_the_header_declares_and_the_binding_types_the_two_entry_points(pkg):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ptmi.h")).read(), flags=re.S)
    assert "int ptmi_trace_rays_device(ptmi_ctx *ctx, const float *d_rays, int n, float *d_t, int32_t *d_idx, float *d_hit );" in text
    assert "int ptmi_occluded_device(ptmi_ctx *ctx, const float *d_rays, const float *d_t_max, int n, int32_t *d_occluded);" in text
    for name in NAMES:
        assert name in pkg.SYMBOLS
    assert len(pkg.SYMBOLS["ptmi_trace_rays_device"][1]) == 6 and len(pkg.SYMBOLS["ptmi_occluded_device"][1]) == 5
    assert not [n for n in pkg.SYMBOLS if n.startswith("ptmi_group_") and ("trace_rays" in n or "occluded" in n)]       # no group form


def test_the_header_states_order_lifetime_and_refusals():
    text = open(os.path.join(ROOT, "include", "ptmi.h")).read()
    section = text[text.index("ray queries on the device"):text.index("int ptmi_trace_rays_device(")]
    for phrase in ("ptmi_set_stream", "no host synchronisation", "keeps every array alive", "ordered behind the query", "PTMI_ESTATE", "PTMI_EINVAL",
                   "n == 0 is PTMI_OK", "ptmi_group_member", "4-byte alignment"):
        assert phrase in section, phrase


BAD_RAYS = [FakeTensor((5, 6), dtype="torch.float64"), FakeTensor((5, 6), dtype="torch.int32"), FakeTensor((5, 6), contiguous=False),
            FakeTensor((5, 6), cuda=False), FakeTensor((30,)), FakeTensor((5, 3)), FakeTensor((6, 5)), FakeTensor((5, 6, 1))]


@pytest.mark.parametrize("rays", BAD_RAYS, ids=lambda t: "%s-%s" % (t.dtype, "x".join(map(str, t.shape))))
def test_rays_of_the_wrong_kind_are_refused(ctx, rays):
    with pytest.raises(ValueError):
        ctx.trace_rays(rays, out=(FakeTensor((5,)), FakeTensor((5,), dtype="torch.int32")))
    with pytest.raises(ValueError):
        ctx.occluded(rays, FakeTensor((5,)), out=FakeTensor((5,), dtype="torch.int32"))


def test_outputs_and_t_max_of_the_wrong_kind_are_refused(ctx):
    rays, t, idx, hit = FakeTensor((5, 6)), FakeTensor((5,)), FakeTensor((5,), dtype="torch.int32"), FakeTensor((5, 6))
    for out in ((FakeTensor((4,)), idx), (t, FakeTensor((5,))), (t, FakeTensor((5,), dtype="torch.uint32")), (t, idx, FakeTensor((5, 3))),
                (t, idx, FakeTensor((5, 6), contiguous=False)), (FakeTensor((5,), cuda=False), idx), (t,), (t, idx, hit, hit)):
        with pytest.raises(ValueError):
            ctx.trace_rays(rays, out=out)
    for t_max in (FakeTensor((4,)), FakeTensor((6,)), FakeTensor((5, 1)), FakeTensor((5,), dtype="torch.float64"), FakeTensor((5,), contiguous=False),
                  FakeTensor((5,), cuda=False)):
        with pytest.raises(ValueError):
            ctx.occluded(rays, t_max, out=idx)
    for out in (FakeTensor((5,)), FakeTensor((4,), dtype="torch.int32"), FakeTensor((5,), dtype="torch.int32", contiguous=False)):
        with pytest.raises(ValueError):
            ctx.occluded(rays, t, out=out)


def test_well_formed_tensors_reach_the_library(ctx):
    """... and only they: the stand-in library is asked for the entry point once validation has passed"""
    rays, t, idx, hit = FakeTensor((5, 6)), FakeTensor((5,)), FakeTensor((5,), dtype="torch.int32"), FakeTensor((5, 6))
    with pytest.raises(AssertionError, match="ptmi_trace_rays_device"):
        ctx.trace_rays(rays, out=(t, idx, hit))
    with pytest.raises(AssertionError, match="ptmi_occluded_device"):
        ctx.occluded(rays, t, out=idx)
