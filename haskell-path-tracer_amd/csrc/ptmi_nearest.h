// ptmi_nearest.h -- the arithmetic of the NEAREST-PRIMITIVE QUERY (ptmi_nearest_device, ptmi_nearest): a primitive's signed distance from
// a point and the nearest location on it, and the lower bound of a box's distance, ONE definition for the host twin (ptmi_nearest.cpp),
// the kernels (ptmi_nearest.hip through ptmi_nearest_device.h) and the CPU restatement of the walk (tests/cxx/nearest_traverse.cpp): the
// device equals the twin bit for bit because it runs the twin's operations.  Every operation is a binary32 operation rounded on its own
// (the build passes -ffp-contract=off), square roots and divisions correctly rounded.
//
// EVERYTHING IS RELATIVE TO THE POINT p: a primitive's coordinates meet p in one subtraction each (exact up to 2^-24 of the difference)
// and nothing else ever sees an absolute coordinate, so every intermediate is bounded by FAR, the distance from p to the farthest point
// of the primitive, and every rounding by a small multiple of 2^-24 FAR -- at an offset of 10^6 as at the origin.
//
// THE KEY of a primitive is |s|, s its signed distance.  A key that is a NaN or +inf never qualifies: `key < lim` is false for it under
// every lim, +inf included.  No function here branches on "is this a candidate": what is none has such a key.
//   * SPHERE (c, r2): e = p - c, L = sqrt((ex ex + ey ey) + ez ez), r = sqrt(r2), s = L - r -- the distance to the surface, negative
//     inside.  The nearest location is c + e (r / L), and (cx + r, cy, cz) at the centre.  r2 < 0 or a non-finite word: a NaN or inf key.
//   * PLANE (pos, dir): e = p - pos, ln = sqrt((dx dx + dy dy) + dz dz), s = ((ex dx + ey dy) + ez dz) / ln: dir as stored, divided by its
//     length here.  The nearest location is p - dir (s / ln).  A direction whose ln is not a positive finite number (zero, non-finite, or
//     so long or so short that its square leaves binary32) gives s = NaN: no candidate.
//   * TRIANGLE (v0, v1, v2): A = v0 - p, B = v1 - p, C = v2 - p meet the point; the EDGES are formed from the vertices themselves,
//     v1 - v0, v2 - v0, v2 - v1, v0 - v2 -- a difference of neighbours, rounded by 2^-24 of the edge and not of the way to p -- and the
//     normal is formed HERE from them: m = cross(v1 - v0, v2 - v0) with every component a difference of products by Kahan's algorithm
//     (w = c d, e = fma(-c, d, w), f = fma(a, b, -w), f + e: within 1.5 units in the last place however much the products cancel --
//     each fma one operation, rounded once, written as such on host and device), scaled by its largest component and then by its
//     length: n.  The record's stored normal, an f32 cross product without compensation, is noise on a needle and degrees off on a
//     sliver; it is read only for "is this a triangle of zero area" (NaN).  h = dot(A, n), q = n h the foot of p on the plane, and
//     w0, w1, w2 PTMI_TRIANGLE_TEST's edge functions of q in these coordinates.  The key is |h| when w0, w1, w2 are all >= 0 (the foot
//     is inside or on an edge) and the nearest location is p + q; otherwise the least of the three segment distances
//     |A + (v1 - v0) clamp(t, 0, 1)| (the first least of v0v1, v1v2, v2v0) and the location on that edge.  s is negative when h > 0
//     (p behind the front).
//     Why the error is proportional to FAR whatever the shape: A, B, C are the vertices within 2^-24 FAR.  n is the normal of the
//     triangle with the edges as computed, within 2^-21 per component (Kahan's algorithm removes the cancellation of a thin triangle's
//     cross product, which would turn the plane about its long axis by 2^-23 x aspect x the products' size).  What remains is the
//     edges' own rounding, 2^-24 of their length, which turns a thin triangle's plane about its long axis by up to 2^-22 x aspect; a
//     foot that is inside lies within the triangle's height of that axis, so there |h| moves by 2^-22 of a side, and dot(A, n) is the
//     plane's distance within 2^-20 FAR.  The edge functions do cancel on a thin triangle, but only misjudge a foot within 2^-21 FAR of
//     an edge's line, and there the two forms of the key differ by no more.  So
//         D - 2^-19 FAR <= key <= D + 2^-19 FAR,   D the triangle's true distance,
//     the left half of which is what the hierarchy's pruning needs (ptmi_nearest_device.h).  THE SIGN is the true plane's wherever |h|
//     exceeds that error plus 2^-22 x aspect x the foot's distance from v0: everywhere that matters on a well-shaped triangle, however
//     far p is from a small one (a normal formed from B - A would tilt there), and nowhere on a needle of aspect 10^7, whose plane
//     binary32 edges do not determine.  A record with a NaN normal (zero area) is
//     never asked: every loop over records skips it, in a leaf (where a refit can leave one) as in the enumerations.  A kept triangle whose m is 0 or not finite here has a NaN n, fails
//     every edge function and is its three edges.
#pragma once

#include "ptmi_core.h"

namespace ptmi {

struct Nearest {
    float s;        // the signed distance; the key is |s|
    V3 at;          // the nearest location on the primitive (absolute coordinates)
};

PTMI_HD float nearest_length(V3 v) { return __builtin_sqrtf(dot(v, v)); }

PTMI_HD Nearest nearest_sphere(V3 c, float r2, V3 p)
{
    const V3 e = p - c;
    const float L = nearest_length(e);
    const float r = __builtin_sqrtf(r2);
    Nearest a;
    a.s = L - r;
    a.at = L > 0.0f ? c + scale_r(e, r / L) : mk(c.x + r, c.y, c.z);
    return a;
}

PTMI_HD Nearest nearest_plane(V3 pos, V3 dir, V3 p)
{
    const V3 e = p - pos;
    const float ln = nearest_length(dir);
    const bool usable = ln > 0.0f && ln < __builtin_inff();
    Nearest a;
    a.s = usable ? dot(e, dir) / ln : __builtin_nanf("");
    a.at = p - scale_r(dir, a.s / ln);
    return a;
}

// The nearest location to the origin of the segment that starts at A (relative to p) and runs along d (the edge, formed from the vertices
// themselves).  t = -dot(A, d) / dot(d, d), clamped into [0, 1]; a NaN (an edge whose squared length underflowed to 0) is taken as 0
PTMI_HD V3 nearest_on_segment(V3 A, V3 d)
{
    const float t = -dot(A, d) / dot(d, d);
    const float tc = !(t > 0.0f) ? 0.0f : (t > 1.0f ? 1.0f : t);
    return A + scale_r(d, tc);
}

// a b - c d within 1.5 units in the last place (Kahan; Jeannerod, Louvet, Muller 2013)
PTMI_HD float nearest_diff_of_products(float a, float b, float c, float d)
{
    const float w = c * d;
    const float e = __builtin_fmaf(-c, d, w);
    const float f = __builtin_fmaf(a, b, -w);
    return f + e;
}

PTMI_HD Nearest nearest_triangle(V3 v0, V3 v1, V3 v2, V3 p)
{
    const V3 A = v0 - p, B = v1 - p, C = v2 - p;
    const V3 E1 = v1 - v0, E2 = v2 - v0, E12 = v2 - v1, E20 = v0 - v2;          // the edges, from the vertices themselves
    const V3 m = mk(nearest_diff_of_products(E1.y, E2.z, E1.z, E2.y), nearest_diff_of_products(E1.z, E2.x, E1.x, E2.z),
                    nearest_diff_of_products(E1.x, E2.y, E1.y, E2.x));
    const float big = __builtin_fmaxf(__builtin_fmaxf(__builtin_fabsf(m.x), __builtin_fabsf(m.y)), __builtin_fabsf(m.z));
    const V3 u = div_r(m, big);
    const V3 n = div_r(u, nearest_length(u));
    const float h = dot(A, n);
    const V3 q = scale_r(n, h);
    const float w0 = dot(cross(E1, q - A), n);
    const float w1 = dot(cross(E12, q - B), n);
    const float w2 = dot(cross(E20, q - C), n);
    V3 best = q;
    float key = __builtin_fabsf(h);
    if (!(w0 >= 0.0f && w1 >= 0.0f && w2 >= 0.0f)) {
        best = nearest_on_segment(A, E1);
        key = nearest_length(best);
        const V3 g1 = nearest_on_segment(B, E12);
        const float k1 = nearest_length(g1);
        if (k1 < key) { key = k1; best = g1; }
        const V3 g2 = nearest_on_segment(C, E20);
        const float k2 = nearest_length(g2);
        if (k2 < key) { key = k2; best = g2; }
    }
    Nearest a;
    a.s = h > 0.0f ? -key : key;
    a.at = p + best;
    return a;
}

// THE BOX LOWER BOUND.  For the box (c, hb) -- centre and half extent, as a node stores it -- g = max(|c - p| - hb, 0) per axis is the gap
// between p and the box, lb = sqrt((gx gx + gy gy) + gz gz) its distance and p1 = sum(|c - p| + hb) the L1 length of the way to its
// farthest corner, which bounds FAR of every primitive inside.  The bound returned is lb LOWERED by the margin
//         m = 2^-16 p1 + 2^-60
// for two roundings (the stored boxes truly contain their primitives, so nothing else needs covering):
//   * of the keys under the box: key >= D - 2^-19 FAR (above; a sphere's L - r within 2^-20 FAR), D >= the box's true
//     distance, FAR <= p1;
//   * of lb itself: three subtractions |c - p| (2^-24 |c - p| each), three of hb, the squares, their sum and the root, at most
//     2^-21 p1 above the true distance.
// Together a key under the box is never below lb - 2.5 x 2^-20 p1; 2^-16 p1 is twenty-five times that and costs only speed.  2^-60 covers
// squares that underflow (below 2^-126 a product is rounded to a multiple of 2^-149, a root of it moves by at most 2^-75): the argument
// needs no product to overflow, which |coordinate - p| <= 2^40 guarantees -- the admission rule of the walk.
constexpr float kNearestMargin = 0x1p-16f, kNearestMarginFloor = 0x1p-60f;

PTMI_HD float nearest_box_bound(V3 c, V3 hb, V3 p, float margin)
{
    const float ax = __builtin_fabsf(c.x - p.x), ay = __builtin_fabsf(c.y - p.y), az = __builtin_fabsf(c.z - p.z);
    const float gx = __builtin_fmaxf(ax - hb.x, 0.0f), gy = __builtin_fmaxf(ay - hb.y, 0.0f), gz = __builtin_fmaxf(az - hb.z, 0.0f);
    const float p1 = ((ax + hb.x) + (ay + hb.y)) + (az + hb.z);
    const float lb = __builtin_sqrtf((gx * gx + gy * gy) + gz * gz);
    return lb - (margin * p1 + (margin > 0.0f ? kNearestMarginFloor : 0.0f));
}

// (key, j) below (best_key, best_j), lexicographically, and key < lim: the one rule by which a candidate replaces the best so far
PTMI_HD bool nearest_better(float key, int j, float lim, float best_key, int best_j)
{
    return (key < lim) & ((key < best_key) | ((key == best_key) & (j < best_j)));
}

}  // namespace ptmi
