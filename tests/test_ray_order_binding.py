"""The ray order's and the indexed queries' face in the header and the binding (no GPU needed): include/ptmi.h declares the entries in a
section of their own behind the plain queries, binding.SYMBOLS types every one of them as declared, and the Python wrappers --
binding.ray_order / ray_order_keys on numpy arrays, Context.ray_order and the index= keyword of Context.trace_rays / Context.occluded on
device tensors -- refuse a wrong dtype, shape or contiguity with ValueError before anything reaches the library (the stand-ins of
tests/test_ray_query_binding.py)."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
from test_ray_query_binding import FakeTensor, NoLibrary  # noqa: E402

DECLARED = {
    "ptmi_ray_order_bytes": "size_t ptmi_ray_order_bytes(int n);",
    "ptmi_ray_order_device": "int ptmi_ray_order_device(ptmi_ctx *ctx, const float *d_rays, int n, int32_t *d_order, void *d_work, size_t work_bytes);",
    "ptmi_ray_order": "int ptmi_ray_order(const float *rays, int n, int32_t *order);",
    "ptmi_ray_order_keys": "int ptmi_ray_order_keys(const float *rays, int n, uint64_t *keys);",
    "ptmi_trace_rays_indexed_device": "int ptmi_trace_rays_indexed_device(ptmi_ctx *ctx, const float *d_rays, int n, const int32_t *d_index, int m, "
                                      "float *d_t, int32_t *d_idx, float *d_hit );",
    "ptmi_occluded_indexed_device": "int ptmi_occluded_indexed_device(ptmi_ctx *ctx, const float *d_rays, const float *d_t_max, int n, const int32_t *d_index, int m, "
                                    "int32_t *d_occluded);",
}


@pytest.fixture()
def ctx(pkg):
    c = object.__new__(pkg.Context)          # no device: validation comes before the first use of the handle
    c._lib, c._h = NoLibrary(), None
    return c


def test_the_header_declares_and_the_binding_types_every_entry(pkg):
    text = open(os.path.join(ROOT, "include", "ptmi.h")).read()
    assert "#define PTMI_RAY_ORDER_MAX (1 << 22)" in text and pkg.binding.RAY_ORDER_MAX == 1 << 22
    flat = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", text, flags=re.S))
    for name, declaration in DECLARED.items():
        assert declaration in flat, name
        res, args = pkg.SYMBOLS[name]
        params = declaration[declaration.index("(") + 1:declaration.rindex(")")].split(",")
        assert len(args) == len(params), name
        for arg, param in zip(args, params):           # a pointer for a pointer, an int for an int, a size_t for a size_t
            want = C.c_void_p if "*" in param else (C.c_size_t if "size_t" in param else C.c_int)
            assert arg is want, (name, param)
        assert res is (C.c_size_t if declaration.startswith("size_t") else C.c_int), name
    assert not [n for n in pkg.SYMBOLS if n.startswith("ptmi_group_") and ("ray_order" in n or "indexed" in n)]       # no group form
    assert pkg.load_library().ptmi_version() == 600


def test_the_new_section_stands_behind_the_plain_queries_and_states_the_rules():
    text = open(os.path.join(ROOT, "include", "ptmi.h")).read()
    plain = text.index("int ptmi_occluded_device(")
    start = text.index("ray order and ray queries through an index")
    assert plain < start < text.index("#define PTMI_RAY_ORDER_MAX") < text.index("point queries (the reference's unit-test surface)")
    section = text[start:text.index("#define PTMI_RAY_ORDER_MAX")]
    for phrase in ("permutation of 0 .. n - 1", "(key, original index)", "rays alone", "no PTMI_ESTATE", "8-byte aligned",
                   "no host synchronisation", "PTMI_ELIMIT", "n == 0 is PTMI_OK", "outside [0, n) is skipped", "left untouched", "written twice",
                   "m == 0 is PTMI_OK", "no group form", "csrc/ptmi_ray_order.h"):
        assert phrase in section, phrase


BAD_HOST_RAYS = [np.zeros((5, 6), np.float64), np.zeros((5, 6), np.int32), np.zeros(30, np.float32), np.zeros((5, 3), np.float32), np.zeros((6, 5), np.float32),
                 np.zeros((5, 6, 1), np.float32), np.zeros((5, 12), np.float32)[:, ::2], np.zeros((6, 5), np.float32).T]


@pytest.mark.parametrize("rays", BAD_HOST_RAYS, ids=lambda a: "%s-%s-%s" % (a.dtype, "x".join(map(str, a.shape)), "c" if a.flags.c_contiguous else "strided"))
def test_host_rays_of_the_wrong_kind_are_refused(pkg, rays):
    with pytest.raises(ValueError):
        pkg.binding.ray_order(rays)
    with pytest.raises(ValueError):
        pkg.binding.ray_order_keys(rays)


def test_device_tensors_of_the_wrong_kind_are_refused(ctx):
    rays, t, idx, hit, occ = FakeTensor((5, 6)), FakeTensor((5,)), FakeTensor((5,), dtype="torch.int32"), FakeTensor((5, 6)), FakeTensor((5,), dtype="torch.int32")
    bad_index = [FakeTensor((3,)), FakeTensor((3,), dtype="torch.int64"), FakeTensor((3, 1), dtype="torch.int32"), FakeTensor((3,), dtype="torch.int32", contiguous=False),
                 FakeTensor((3,), dtype="torch.int32", cuda=False), np.zeros(3, np.int32), [0, 1, 2]]
    for index in bad_index:
        with pytest.raises(ValueError):
            ctx.trace_rays(rays, out=(t, idx, hit), index=index)
        with pytest.raises(ValueError):
            ctx.occluded(rays, t, out=occ, index=index)
    good = FakeTensor((3,), dtype="torch.int32")
    with pytest.raises(ValueError):
        ctx.trace_rays(FakeTensor((5, 3)), out=(t, idx), index=good)
    with pytest.raises(ValueError):
        ctx.trace_rays(rays, out=(t, FakeTensor((4,), dtype="torch.int32")), index=good)
    with pytest.raises(ValueError):
        ctx.occluded(rays, t, out=FakeTensor((5,)), index=good)


class SizeOnly:
    """Answers ptmi_ray_order_bytes as the header defines it; any other call is a test failure"""

    def __getattr__(self, name):
        if name == "ptmi_ray_order_bytes":
            return lambda n: 24 * n + 1024 * ((n + 4095) // 4096) + 24 if n > 0 else 0
        raise AssertionError("the binding called %s with arguments it should have refused" % name)


def test_ray_order_refuses_bad_rays_out_and_work(pkg):
    c = object.__new__(pkg.Context)
    c._lib, c._h = SizeOnly(), None
    rays, out = FakeTensor((5, 6)), FakeTensor((5,), dtype="torch.int32")
    need = 24 * 5 + 1024 + 24
    work = FakeTensor((need,), dtype="torch.uint8")
    for bad in (FakeTensor((5, 6), dtype="torch.float64"), FakeTensor((30,)), FakeTensor((5, 6), contiguous=False), FakeTensor((5, 6), cuda=False)):
        with pytest.raises(ValueError):
            c.ray_order(bad, out=out, work=work)
    for bad in (FakeTensor((5,)), FakeTensor((4,), dtype="torch.int32"), FakeTensor((5, 1), dtype="torch.int32"), FakeTensor((5,), dtype="torch.int32", contiguous=False)):
        with pytest.raises(ValueError):
            c.ray_order(rays, out=bad, work=work)
    for bad in (FakeTensor((need,), dtype="torch.float32"), FakeTensor((need - 1,), dtype="torch.uint8"), FakeTensor((need, 1), dtype="torch.uint8"),
                FakeTensor((need,), dtype="torch.uint8", contiguous=False), FakeTensor((need,), dtype="torch.uint8", cuda=False)):
        with pytest.raises(ValueError):
            c.ray_order(rays, out=out, work=bad)
    with pytest.raises(AssertionError, match="ptmi_ray_order_device"):
        c.ray_order(rays, out=out, work=work)


def test_well_formed_tensors_reach_the_indexed_entries_and_none_reaches_the_plain_ones(ctx):
    rays, t, idx, hit = FakeTensor((5, 6)), FakeTensor((5,)), FakeTensor((5,), dtype="torch.int32"), FakeTensor((5, 6))
    index = FakeTensor((3,), dtype="torch.int32")
    with pytest.raises(AssertionError, match="ptmi_trace_rays_indexed_device"):
        ctx.trace_rays(rays, out=(t, idx, hit), index=index)
    with pytest.raises(AssertionError, match="ptmi_occluded_indexed_device"):
        ctx.occluded(rays, t, out=idx, index=index)
    with pytest.raises(AssertionError, match="called ptmi_trace_rays_device"):
        ctx.trace_rays(rays, out=(t, idx, hit))
    with pytest.raises(AssertionError, match="called ptmi_occluded_device"):
        ctx.occluded(rays, t, out=idx)
