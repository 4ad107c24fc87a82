"""The CPU half of the caller-owned-planes tests: the arena arithmetic of tests/caller_planes.py puts every plane where it says, the guard
check reports a single foreign word (which is what makes the device's guard checks mean something), and present_reference is the
graphics loop's arithmetic -- equal to the expression tests/test_gpu_boundary.py uses on finite inputs, and right at every rounding
boundary by exact rational arithmetic."""
import os
import sys
from fractions import Fraction

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import caller_planes as cp  # noqa: E402

SHAPES = [(97, 61), (64, 48), (1, 1), (9, 2), (800, 600)]
LAYOUTS = [("ALIGNED", cp.ALIGNED, None), ("ODD", cp.ODD, cp.ORDER), ("ODD as numbered", cp.ODD, None), ("one plane", (3,), None)]


@pytest.mark.parametrize("w,h", SHAPES)
@pytest.mark.parametrize("name,misalign,order", LAYOUTS)
def test_every_plane_gets_the_alignment_asked_for_and_its_guards(w, h, name, misalign, order):
    n = w * h
    lay = cp.arena_layout(n, w, misalign, order)
    assert lay.guard == max(256, 2 * w)
    for base in (0x7F0000001000, 0x7F0000001004, 0x7F0000001008, 0x7F000000100C, 0x10, 4):
        off = lay.offsets(base)
        for k, o in enumerate(off):
            assert (base + 4 * o) % 16 == 4 * misalign[k], (name, base, k)
        spans = sorted((o, o + n) for o in off)
        assert spans[0][0] >= lay.guard and lay.total - spans[-1][1] >= lay.guard
        for (_, end), (start, _) in zip(spans, spans[1:]):
            assert start - end >= lay.guard                                # a guard band of its own between any two planes
        mask = lay.guard_mask(base)
        assert mask.size == lay.total and int((~mask).sum()) == len(misalign) * n      # planes do not overlap each other
        if order is not None:
            assert [k for _, k in sorted((o, k) for k, o in enumerate(off))] == list(order)
    with pytest.raises(ValueError):
        lay.offsets(0x1002)
    with pytest.raises(ValueError):
        cp.arena_layout(n, w, misalign, [0] * len(misalign) if len(misalign) > 1 else [1])


@pytest.mark.parametrize("shift", [0, 1, 2, 3])
def test_guards_intact_reports_one_planted_element_before_and_after_each_plane(shift):
    """A numpy arena whose first element lies `shift` elements past a 16-byte boundary.  One foreign word directly before and one directly
    after every plane, one at a time and all together: guards_intact names exactly the planted indices.  Words written INTO planes are
    not reported."""
    w, h = 37, 23
    n = w * h
    lay = cp.arena_layout(n, w, cp.ODD, cp.ORDER)
    raw = np.zeros(lay.total + 8, np.uint32)
    first = ((-raw.ctypes.data) % 16) // 4 + shift
    buf = raw[first:first + lay.total]
    assert buf.ctypes.data % 16 == 4 * shift
    cp.fill_guards(buf, lay)
    off = lay.offsets(buf.ctypes.data)
    assert cp.guards_intact(buf, lay).size == 0
    assert buf[0] == cp.GUARD_WORD and buf[5] == cp.GUARD_WORD ^ 5
    for o in off:
        buf[o:o + n] = 0xDEADBEEF                                           # a plane's own elements are not guards
    assert cp.guards_intact(buf, lay).size == 0
    planted = []
    for k, o in enumerate(off):
        for index in (o - 1, o + n):
            kept = buf[index]
            buf[index] = kept ^ np.uint32(1 << (k + 1))
            assert cp.guards_intact(buf, lay).tolist() == [index], "plane %s, planted index %d" % (cp.NAMES[k], index)
            buf[index] = kept
            planted.append(index)
    for index in planted:
        buf[index] = 0
    assert cp.guards_intact(buf, lay).tolist() == sorted(planted), "planted indices %r" % (sorted(planted),)
    for index in (0, lay.total - 1):                                        # the buffer's first and last element are guards too
        buf[index] = 7
    assert cp.guards_intact(buf, lay).tolist() == sorted(planted + [0, lay.total - 1])


def boundary_expression(r, g, b, iters):
    """tests/test_gpu_boundary.py::test_present_matches_graphics_loop_arithmetic, its expression as it stands there"""
    want = np.stack([r, g, b], -1) / np.float32(iters)
    with np.errstate(invalid="ignore"):
        clamped = np.where(want > 0, np.minimum(want, np.float32(1.0)), np.float32(0.0)).astype(np.float32)
    want8 = (clamped * np.float32(255.0) + np.float32(0.5)).astype(np.uint32).astype(np.uint8)
    return want.astype(np.float32), want8


@pytest.mark.parametrize("iters", [1, 7, 1000])
def test_present_reference_is_the_existing_tests_expression_on_finite_inputs(iters):
    r, g, b = cp.present_inputs(64 * 48, iters)
    finite = np.isfinite(r) & np.isfinite(g) & np.isfinite(b)
    assert finite.sum() == r.size - 9
    r, g, b = r[finite], g[finite], b[finite]
    rgb, rgba = cp.present_reference(r, g, b, iters)
    want, want8 = boundary_expression(r, g, b, iters)
    assert np.array_equal(rgb.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(rgba[..., :3], want8) and np.all(rgba[..., 3] == 255)
    assert rgba[..., :3].min() == 0 and rgba[..., :3].max() == 255


def test_present_reference_on_non_finite_inputs_and_zeros():
    vals = np.array([np.inf, -np.inf, np.nan, -0.0, 0.0, 1e-40, -1.0, 3.0, 1.0], np.float32)
    rgb, rgba = cp.present_reference(vals, vals[::-1], vals, 2)
    assert rgba[:, 0].tolist() == [255, 0, 0, 0, 0, 0, 0, 255, 128]
    assert rgba[:, 1].tolist() == rgba[::-1, 0].tolist() and np.all(rgba[:, 3] == 255)
    assert np.isnan(rgb[2, 0]) and rgb[0, 0] == np.inf and rgb[1, 0] == -np.inf and np.signbit(rgb[3, 0]) and rgb[5, 0] == np.float32(1e-40) / np.float32(2)


def round_binary32(x):
    """the binary32 nearest a non-negative Fraction, ties to even, as a Fraction (denormals included; no overflow here)"""
    if x == 0:
        return Fraction(0)
    e = x.numerator.bit_length() - x.denominator.bit_length()
    if Fraction(2) ** e > x:
        e -= 1
    e = max(e, -126)
    ulp = Fraction(2) ** (e - 23)
    q, rem = divmod(x, ulp)
    if rem * 2 > ulp or (rem * 2 == ulp and q % 2 == 1):
        q += 1
    return q * ulp


@pytest.mark.parametrize("iters", [1, 7, 1000])
def test_present_reference_puts_every_rounding_boundary_where_exact_arithmetic_does(iters):
    """The inputs on both sides of (k + 0.5) / 255 * iterations, as binary32 values.  Every operation of the device's chain -- the division,
    the multiplication by 255, the addition of 0.5 -- is the exact rational result rounded to binary32; the byte is the floor of the last.
    It is k or k + 1, and both occur for every k below 255."""
    v = cp.rounding_boundaries(iters)
    _, rgba = cp.present_reference(v, v, v, iters)
    got = rgba[:, 0].astype(int)
    want = []
    for x in v.tolist():
        q = round_binary32(Fraction(x) / iters)
        q = min(q, Fraction(1))
        want.append(int(round_binary32(round_binary32(q * 255) + Fraction(1, 2))))
    assert got.tolist() == want
    ks = np.repeat(np.arange(256), 5)
    assert np.all((got == ks) | (got == np.minimum(ks + 1, 255)))
    for k in range(255):
        assert set(got[5 * k:5 * k + 5]) == {k, k + 1}, k


def test_present_inputs_hold_what_they_promise():
    for n, iters in ((64 * 48, 7), (61 * 7, 1000), (18, 1), (1, 7)):
        r, g, b = cp.present_inputs(n, iters)
        assert r.dtype == g.dtype == b.dtype == np.float32 and r.size == g.size == b.size == n
        stack = np.stack([r, g, b])
        for k, value in enumerate((np.inf, -np.inf, np.nan)):
            for channel in range(3):
                at = 3 * k + channel
                if at < n:
                    assert (np.isnan(stack[channel, at]) if value != value else stack[channel, at] == value)
                    assert np.all(np.isfinite(np.delete(stack[:, at], channel)))
    r, g, b = cp.present_inputs(64 * 48, 7)
    special = cp.special_values(7)
    assert special.size == 1280 + 20
    for plane in (r, g, b):
        assert set(special.view(np.uint32).tolist()) <= set(plane.view(np.uint32).tolist())
    assert np.any(np.signbit(r) & (r == 0)) and np.any((np.abs(r) > 0) & (np.abs(r) < np.float32(1.1754944e-38)))
