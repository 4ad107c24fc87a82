"""The nearest-primitive query's face in the header and the binding (no GPU needed): include/ptmi.h declares ptmi_nearest_device,
ptmi_nearest_indexed_device and the host twin ptmi_nearest behind the multi-hit section and states the specification, binding.SYMBOLS types
all three, there is no group form, Context.nearest refuses tensors of the wrong dtype, contiguity or shape with ValueError before anything
reaches the library -- shown with test_ray_query_binding.py's stand-ins -- and binding.nearest, the host twin, refuses what it must and
answers a scene whose answers are known."""
import os
import re

import numpy as np
import pytest

from test_ray_query_binding import FakeTensor, NoLibrary

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ptmi_nearest_device", "ptmi_nearest_indexed_device", "ptmi_nearest")


@pytest.fixture()
def ctx(pkg):
    c = object.__new__(pkg.Context)          # no device: validation comes before the first use of the handle
    c._lib, c._h = NoLibrary(), None
    return c


def header():
    return open(os.path.join(ROOT, "include", "ptmi.h")).read()


def test_the_header_declares_and_the_binding_types_the_three_entry_points(pkg):
    text = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", header(), flags=re.S))
    assert ("int ptmi_nearest_device(ptmi_ctx *ctx, const float *d_points , const float *d_r_max , int n, float *d_dist , int32_t *d_idx , "
            "float *d_point );") in text
    assert ("int ptmi_nearest_indexed_device(ptmi_ctx *ctx, const float *d_points, const float *d_r_max, int n, const int32_t *d_index, int m, "
            "float *d_dist, int32_t *d_idx, float *d_point);") in text
    assert ("int ptmi_nearest(const ptmi_sphere *spheres, int n_spheres, const ptmi_plane *planes, int n_planes, const ptmi_triangle *triangles, "
            "int n_triangles, const float *points, const float *r_max, int n, float *dist, int32_t *idx, float *point);") in text
    for name in NAMES:
        assert name in pkg.SYMBOLS
    assert [len(pkg.SYMBOLS[n][1]) for n in NAMES] == [7, 9, 12]
    assert not [n for n in pkg.SYMBOLS if n.startswith("ptmi_group_") and "nearest" in n]       # no group form
    assert "#define PTMI_VERSION 600 " in header()                                             # the version other tests pin is not moved
    bump = header()[header().index("Added without a version bump"):header().index("---- error codes")]
    for name in NAMES:
        assert name in bump, name


def test_the_section_sits_behind_multi_hit_and_states_the_specification():
    text = header()
    assert text.index("multi-hit: the k nearest hits") < text.index("the nearest-primitive query: the primitive nearest") < text.index("paths along a caller's rays")
    section = text[text.index("the nearest-primitive query: the primitive nearest"):text.index("int ptmi_nearest_device(")]
    for phrase in ("one binary32 compare", "spheres, then planes, then triangles", "at equal keys the lower index", "NaN or +inf key", "NaN or non-positive r_max",
                   "NEGATIVE BEHIND THE SURFACE", "dist 0, idx -1", "RELATIVE TO THE POINT", "(cx + r, cy, cz)", "zero or non-finite", "triangle of zero area",
                   "outside [0, n) is skipped", "left untouched", "PTMI_ESTATE", "PTMI_EINVAL", "d_r_max and d_point may be NULL", "n == 0 or m == 0 is PTMI_OK",
                   "HOST TWIN", "ptmi_set_scene_mesh refuses", "2^40", "no group form"):
        assert phrase in section, phrase


BAD_POINTS = [FakeTensor((5, 3), dtype="torch.float64"), FakeTensor((5, 3), dtype="torch.int32"), FakeTensor((5, 3), contiguous=False),
              FakeTensor((5, 3), cuda=False), FakeTensor((15,)), FakeTensor((5, 6)), FakeTensor((3, 5)), FakeTensor((5, 3, 1))]


def good(n=5, point=True):
    out = (FakeTensor((n,)), FakeTensor((n,), dtype="torch.int32"))
    return out + (FakeTensor((n, 3)),) if point else out


@pytest.mark.parametrize("points", BAD_POINTS, ids=lambda t: "%s-%s" % (t.dtype, "x".join(map(str, t.shape))))
def test_points_of_the_wrong_kind_are_refused(ctx, points):
    with pytest.raises(ValueError):
        ctx.nearest(points, out=good())


def test_outputs_r_max_and_index_of_the_wrong_kind_are_refused(ctx):
    points = FakeTensor((5, 3))
    dist, idx, at = good()
    for out in ((FakeTensor((4,)), idx, at), (FakeTensor((5, 1)), idx, at), (FakeTensor((5,), dtype="torch.float64"), idx, at), (dist, FakeTensor((5,)), at),
                (dist, FakeTensor((5,), dtype="torch.int64"), at), (dist, idx, FakeTensor((5, 6))), (dist, idx, FakeTensor((15,))), (dist, idx, FakeTensor((4, 3))),
                (dist, idx, FakeTensor((5, 3), dtype="torch.int32")), (FakeTensor((5,), contiguous=False), idx, at), (dist, idx, FakeTensor((5, 3), cuda=False)),
                (dist,), (dist, idx, at, at)):
        with pytest.raises(ValueError):
            ctx.nearest(points, out=out)
    for r_max in (FakeTensor((4,)), FakeTensor((5, 1)), FakeTensor((5,), dtype="torch.float64"), FakeTensor((5,), contiguous=False), FakeTensor((5,), cuda=False)):
        with pytest.raises(ValueError):
            ctx.nearest(points, r_max=r_max, out=(dist, idx, at))
    for index in (FakeTensor((3,)), FakeTensor((3, 1), dtype="torch.int32"), FakeTensor((3,), dtype="torch.int32", contiguous=False),
                  FakeTensor((3,), dtype="torch.int32", cuda=False)):
        with pytest.raises(ValueError):
            ctx.nearest(points, out=(dist, idx, at), index=index)


def test_well_formed_tensors_reach_the_library(ctx):
    """... and only they: the stand-in library is asked for the entry point once validation has passed"""
    points = FakeTensor((5, 3))
    for point in (False, True):
        with pytest.raises(AssertionError, match="ptmi_nearest_device"):
            ctx.nearest(points, out=good(5, point))
        with pytest.raises(AssertionError, match="ptmi_nearest_device"):
            ctx.nearest(points, r_max=FakeTensor((5,)), out=good(5, point))
        with pytest.raises(AssertionError, match="ptmi_nearest_indexed_device"):
            ctx.nearest(points, out=good(5, point), index=FakeTensor((3,), dtype="torch.int32"))


# ---- the host twin ---------------------------------------------------------------------------------------------------------------

def scene(pkg):
    W = pkg.world
    s = np.array([W.sphere((0.0, 0.0, 0.0), 1.0, (0.5, 0.5, 0.5), 0.0, W.MATTE, 1.0), W.sphere((10.0, 0.0, 0.0), 2.0, (0.5, 0.5, 0.5), 0.0, W.MATTE, 1.0)],
                 dtype=pkg.binding.SPHERE_DTYPE)
    p = np.array([W.plane((0.0, -5.0, 0.0), (0.0, 2.0, 0.0), (0.5, 0.5, 0.5), 0.0, W.MATTE, 1.0)], dtype=pkg.binding.PLANE_DTYPE)
    t = np.zeros(1, pkg.binding.TRIANGLE_DTYPE)
    t["v0"], t["v1"], t["v2"] = (0.0, 0.0, 20.0), (4.0, 0.0, 20.0), (0.0, 4.0, 20.0)
    t["color"], t["brdf_tag"], t["brdf_param"] = 0.5, W.MATTE, 1.0
    return s, p, t


def test_the_twin_answers_a_scene_whose_answers_are_known(pkg):
    s, p, t = scene(pkg)
    pts = np.array([[3.0, 0.0, 0.0], [0.0, 0.5, 0.0], [0.0, 0.0, 0.0], [10.0, 0.0, 0.5], [0.0, -4.0, 0.0], [0.0, -7.0, 0.0], [1.0, 1.0, 23.0], [1.0, 1.0, 16.0],
                    [-3.0, 0.0, 20.0], [np.nan, 0.0, 0.0]], np.float32)
    dist, idx, at = pkg.binding.nearest(s, p, t, pts, point=True)
    assert idx.tolist() == [0, 0, 0, 1, 2, 2, 3, 3, 3, -1]
    assert dist.tolist() == [2.0, -0.5, -1.0, -1.5, 1.0, -2.0, 3.0, -4.0, 3.0, 0.0]       # behind a triangle's front (+z here): negative
    assert at.tolist() == [[1, 0, 0], [0, 1, 0], [1, 0, 0], [10, 0, 2], [0, -5, 0], [0, -5, 0], [1, 1, 20], [1, 1, 20], [0, 0, 20], [0, 0, 0]]
    d2, i2 = pkg.binding.nearest(s, p, t, pts, r_max=np.array([2.0, 0.5, 1.5, np.nan, 0.0, -1.0, 3.5, 4.0, np.inf, 1.0], np.float32))
    assert i2.tolist() == [-1, -1, 0, -1, -1, -1, 3, -1, 3, -1] and d2.tolist() == [0.0, 0.0, -1.0, 0.0, 0.0, 0.0, 3.0, 0.0, 3.0, 0.0]
    assert pkg.binding.nearest(s, None, None, pts[:1])[1].tolist() == [0] and pkg.binding.nearest(None, p, None, pts[:1])[0].tolist() == [5.0]
    empty = pkg.binding.nearest(s, p, t, np.zeros((0, 3), np.float32), point=True)
    assert [a.shape for a in empty] == [(0,), (0,), (0, 3)]


def test_the_twin_refuses_what_it_must(pkg):
    s, p, t = scene(pkg)
    pts = np.zeros((4, 3), np.float32)
    for bad in (np.zeros((4, 3)), np.zeros((4, 6), np.float32), np.zeros(12, np.float32), np.zeros((3, 4), np.float32).T):
        with pytest.raises(ValueError):
            pkg.binding.nearest(s, p, t, bad)
    for r_max in (np.zeros(3, np.float32), np.zeros(4), np.zeros((4, 1), np.float32)):
        with pytest.raises(ValueError):
            pkg.binding.nearest(s, p, t, pts, r_max=r_max)
    with pytest.raises(pkg.PtmiError) as e:
        pkg.binding.nearest(None, None, None, pts)                                         # an empty scene
    assert e.value.code == pkg.binding.PTMI_EINVAL
    flat = t.copy()
    flat["v2"][0, 0] = np.inf
    with pytest.raises(pkg.PtmiError) as e:
        pkg.binding.nearest(s, p, flat, pts)                                               # what ptmi_set_scene_mesh refuses in a triangle
    assert e.value.code == pkg.binding.PTMI_EINVAL
    wild = s.copy()
    wild["radius"][1] = np.inf
    with pytest.raises(pkg.PtmiError):
        pkg.binding.nearest(wild, p, t, pts)                                               # ... and in a sphere, once there are triangles
    odd = p.copy()
    odd["brdf_tag"][0] = 99
    with pytest.raises(pkg.PtmiError) as e:
        pkg.binding.nearest(s, odd, t, pts)                                                # ... and an unknown tag, of a plane too
    assert e.value.code == pkg.binding.PTMI_EINVAL
    assert pkg.binding.nearest(wild, p, None, pts)[1].tolist() == [0] * 4                  # a linear scene takes it: the sphere is no candidate
