"""checkHit on triangles in plain float64, as geometry defines it: the reference the triangle test (PTMI_TRIANGLE_TEST,
csrc/ptmi_mesh_device.h; restated in tests/cxx/mesh_traverse.c) is held to.  Nothing here calls the project's arithmetic.  The inputs are
f32 values taken as exact; float64 carries them with a relative error of 1e-16 against f32's 6e-8, so float64 is the truth, and a value
within 1e-9 (relative) of a decision boundary is decided again in rationals (fractions.Fraction) for that ray / triangle pair.

For a ray (o, d) and a triangle (v0, v1, v2):  N = (v1 - v0) x (v2 - v0),  n^ = N / |N|,  denom = d . n^,  t* = (v0 - o) . n^ / denom,
p* = o + d t*,  and s_k (k = 0, 1, 2) the signed distance of p* from the line of edge E_k (E_0 = v1 - v0 at v0, E_1 = v2 - v1 at v1,
E_2 = v0 - v2 at v2) within the plane, positive inside:  s_k = (p* - v_k) . m_k,  m_k = n^ x E_k / |E_k|.
A hit needs denom <= 1e-6 (the f32 constant), t* >= 0 and every s_k >= 0 (edges and vertices are inside); a triangle of zero area is never
hit; the smallest t wins, the lower index at equal t.

f32 cannot decide a case on a boundary, so each ray gets two sets:
  P (possible): denom <= 1e-6 + d_denom,  t* >= -tau,  every s_k >= -delta_k
  D (decisive): denom <= 1e-6 - d_denom,  t* >=  tau,  every s_k >=  delta_k              (D is a subset of P)
and an answer (just, idx, t) is checked by check_answers below (rules 1 to 3 of its docstring); normals by normal_errors (rule 4).

THE BOUNDS (Triangles, classify): a forward analysis of the f32 operations, u = 2^-24, first order in u, every term a product of
u, a small integer and magnitudes of the inputs and of the float64 truth.  Nothing in them was fitted to any output.
  1. The stored normal.  e1 = fl(v1 - v0), e2 = fl(v2 - v0): relative u per component.  A component of fl(e1 x e2) is fl(fl(a b) - fl(c d)):
     each product carries 2 u from its operands and u of its own, the difference u of its result, so with A = |e1| x~ |e2| (the cross
     product of the absolute values with + for -: A_x = |e1y e2z| + |e1z e2y|)  |dN| <= 3 u |A| + u |N| <= 4 u |A|.  The direction of N is
     then off by kappa = 4 u |A| / |N| -- this is the cancellation of a needle: |A| stays |e1| |e2| while |N| shrinks with the sine of the
     angle.  nn = fl(N . N) is relative 3 u, its root 1.5 u + u, each division u: 3.5 u on the length.  Together
         nu = |n_f - n^| <= 4 u (|A| / |N| + 1).
     (kappa is the sine of the angle; below 1/4 the chord is within 1 % of it.)  What follows uses nu as an exact bound on
     |n_f - n^|, not to first order, so it holds while nu is small against 1: a triangle with SAFETY nu >= 1/2, or with |N|^2 outside
     [2^-120, 2^120] (f32 under- or overflow of nn), is UNCONSTRAINED: its f32 normal says nothing about its plane, it is never in D
     and, unless its area is zero in f32 as well, in P for every ray.  Zero area means two bitwise equal vertices (then fl(e1 x e2) is
     exactly 0: fl(a b) - fl(b a)); a triangle whose exact N is 0 without that is unconstrained.
  2. denom_f = fl(d . n_f): the normal's error gives |d| nu, the three-term dot product gamma_3 sum |d_i n_i| <= 3 u |d|:
         d_denom = |d| (nu + 3 u).
  3. t.  In exact arithmetic the perturbed normal gives t' = (v0 - o) . n_f / d . n_f, the ray's meeting with the plane through v0 tilted
     by nu:  t' - t* = (v0 - p*) . (n_f - n^) / (d . n_f)   (as (v0 - p*) . n^ = 0), at most nu |p* - v0| / (|denom| - d_denom): the tilt
     counts over the distance from v0 to the hit, NOT over |v0 - o|.  The rounding of the numerator is u |w| for fl(v0 - o) (w = v0 - o)
     and 3 u |w| for the dot product, that of the denominator 3 u |d| (scaled by t), the division u t:
         tau = (nu |p* - v0| + 4 u |w| + 3 u |t*| |d|) / (|denom| - d_denom) + u |t*|,     infinite where |denom| <= d_denom.
     (ptmi_mesh_device.h claims "off its plane by 3 eps t + 4 eps |v0 - o|": the last two terms of the numerator, before the division
     by |denom| that turns a distance off the plane into a distance along the ray -- tau scales with 1 / |denom|.  The tilt term is
     missing there; it is what a needle adds.)
  4. p_f = fl(o + fl(d t_f)): u |d| t for the product and u |p| for the sum per component,  rho = u (|d| |t*| + |p*|)  (the claim:
     eps (|o| + |p|), the same size).  So p_f - p* = d (t_f - t*) + r, |r| <= rho, and  dq = |p_f - p*| <= |d| tau + rho.
  5. The edge functions w_k = fl((fl(E_k) x fl(p_f - v_k)) . n_f), against |E_k| s_k, divided by |E_k| (a distance):
       * p_f moved along the ray by t_f - t* moves WITHIN the plane by (d . m_k)(t_f - t*): at grazing incidence the f32 decision at an edge
         is uncertain by |d . m_k| tau, far more than the rounding of w_k itself; plus rho;
       * (E x q*) is parallel to n^, and n_f - n^ is perpendicular to n^ up to nu^2 / 2 + 3.5 u:  |q_k| (nu^2 + 4 u), q_k = p* - v_k;
         for the moved part dq the full nu applies: dq nu;
       * rounding: u on each component of E and q, u per product, u per difference: 4 u |A(E, q)| <= 4 sqrt(3) u |E| |q|, and
         3 u |E| |q| for the dot product: 10 u |q_k|  (the claim: 8 eps |p - v_k|).
         delta_k = |d . m_k| tau + rho + (|q_k| + dq)(nu^2 + 14 u) + dq nu.
  6. Where |denom| <= d_denom the f32 t says nothing (tau is infinite), but an accepted p_f still passed the edge functions and lies in
     the plane through v0 across n_f: it is a point of the triangle tilted about v0 by at most nu -- within r (1 + 2 nu) of the centroid
     c, r = max |v_k - c| -- or outside an edge's line by no more than that edge function's rounding, e = 14 u |q_k| (item 5).  Outside two
     lines that meet at the angle theta, by e each, a point is at most e / sin(theta / 2) beyond their corner; with |q_k| <= 2 r + ov that
     is ov <= k (2 r + ov), k = 14 u / sin(theta_min / 2) (theta_min the triangle's smallest angle: what a needle makes small), so
     ov <= 2 r k / (1 - k) while k < 1 (otherwise nothing is excluded).  p_f itself is o + d t_f up to rho <= u (|o| + 2 |p_f|).  A ray
     whose LINE passes farther from c than  r (1 + 2 nu) + ov + u (|o| + 2 (|c| + r (1 + 2 nu) + ov))  cannot be answered by that
     triangle: it is not in P.  (This only matters for thin triangles, whose nu makes many rays "grazing".)
  SAFETY = 2, chosen once: every bound above is multiplied by it (nu inside the others too).  It stands for what a first-order analysis
  drops -- products of (1 + u) factors, nu u cross terms, and the use of the truth's |t*|,
  |p*|, |q_k| where the f32 values (within the same bounds of them) appear.  f32 underflow is not modelled beyond item 1's range check:
  a product that underflows errs by 2^-149 absolutely, below every bound here for coordinates above 2^-60.
"""
import os
from concurrent.futures import ThreadPoolExecutor
from fractions import Fraction

import numpy as np

U = 2.0 ** -24
SAFETY = 2.0
NORMAL_LIMIT = 0.5
DENOM_MAX = float(np.float32(1e-6))
THREADS = max(1, min(16, os.cpu_count() or 1))
INF = np.inf


class Triangles:
    """Per-triangle float64 truth and bounds (item 1 above) for (n, 3, 3) f32 vertices"""

    def __init__(self, vertices):
        v32 = np.ascontiguousarray(vertices, np.float32).reshape(-1, 3, 3)
        v = v32.astype(np.float64)
        self.v = v
        e1, e2 = v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]
        N = np.cross(e1, e2)
        a1, a2 = np.abs(e1), np.abs(e2)
        A = np.stack([a1[:, 1] * a2[:, 2] + a1[:, 2] * a2[:, 1], a1[:, 2] * a2[:, 0] + a1[:, 0] * a2[:, 2],
                      a1[:, 0] * a2[:, 1] + a1[:, 1] * a2[:, 0]], 1)
        NN = np.einsum("ij,ij->i", N, N)
        same = np.all(v32[:, 0] == v32[:, 1], 1) | np.all(v32[:, 0] == v32[:, 2], 1) | np.all(v32[:, 1] == v32[:, 2], 1)
        self.zero_area = same                                          # never hit, by f32 and by geometry alike
        with np.errstate(divide="ignore", invalid="ignore"):
            length = np.sqrt(NN)
            self.nhat = np.where(NN[:, None] > 0, N / length[:, None], 0.0)
            self.nu = np.where(NN > 0, 4.0 * U * (np.linalg.norm(A, axis=1) / length + 1.0), INF)
        self.unconstrained = ~same & ((SAFETY * self.nu >= NORMAL_LIMIT) | (NN < 2.0 ** -120) | (NN > 2.0 ** 120))
        self.nu = np.where(self.unconstrained | same, 0.0, self.nu)   # (unused for those; kept finite for the array arithmetic)
        self.raw_nu = np.where(NN > 0, 4.0 * U * (np.linalg.norm(A, axis=1) / np.where(length > 0, length, 1.0) + 1.0), INF)
        E = np.stack([v[:, 1] - v[:, 0], v[:, 2] - v[:, 1], v[:, 0] - v[:, 2]], 1)      # (n, 3 edges, 3)
        El = np.linalg.norm(E, axis=2)
        Eh = E / np.where(El > 0, El, 1.0)[:, :, None]
        self.m = np.cross(self.nhat[:, None, :], Eh)                   # inward in-plane normals of the edges
        self.c = np.einsum("nkj,nkj->nk", v, self.m)                   # v_k . m_k
        self.v0n = np.einsum("ij,ij->i", v[:, 0], self.nhat)
        self.vv = np.einsum("nkj,nkj->nk", v, v)                       # |v_k|^2
        self.cen = v.mean(1)
        self.rb = np.linalg.norm(v - self.cen[:, None, :], axis=2).max(1)
        self.cc = np.einsum("ij,ij->i", self.cen, self.cen)
        cosines = [-np.einsum("ij,ij->i", Eh[:, k], Eh[:, (k + 1) % 3]) for k in range(3)]         # of the angle at v_(k+1)
        half_sine = np.sqrt(np.maximum(0.5 * (1.0 - np.max(cosines, 0)), 0.0))                      # sin(theta_min / 2)
        with np.errstate(divide="ignore", invalid="ignore"):
            k6 = SAFETY * 14.0 * U / half_sine
            self.overshoot = np.where(k6 < 1.0, 2.0 * self.rb * k6 / (1.0 - k6), INF)              # item 6's ov (infinite: nothing excluded)
        self.n = len(v)


def _norm_from(oo, ov, vv):
    return np.sqrt(np.maximum(oo - 2.0 * ov + vv, 0.0))


def _classify_chunk(tr, rays, answer_k):
    """One chunk of rays against every triangle -> (the per-ray figures classify() documents, the rays x triangles arrays behind them)"""
    o, d = rays[:, :3], rays[:, 3:]
    R = len(rays)
    dl = np.linalg.norm(d, axis=1)[:, None]
    ol = np.linalg.norm(o, axis=1)[:, None]
    oo = ol * ol
    nu = (SAFETY * tr.nu)[None, :]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        denom = d @ tr.nhat.T
        num = tr.v0n[None, :] - o @ tr.nhat.T
        d_denom = dl * (nu + SAFETY * 3.0 * U)
        room = np.abs(denom) - d_denom
        ok = (room > 0) & ~tr.unconstrained[None, :] & ~tr.zero_area[None, :]
        t = np.where(ok, num / np.where(ok, denom, 1.0), 0.0)
        od, dd = np.einsum("ij,ij->i", o, d)[:, None], dl * dl
        q = [_norm_from(oo + 2.0 * t * od + t * t * dd, (o @ tr.v[:, k].T) + t * (d @ tr.v[:, k].T), tr.vv[None, :, k]) for k in range(3)]
        w = _norm_from(oo, o @ tr.v[:, 0].T, tr.vv[None, :, 0])
        at = np.abs(t)
        pl = np.minimum(ol + at * dl, np.sqrt(tr.vv[None, :, 0]) + q[0])
        tau = np.where(ok, (nu * q[0] + SAFETY * U * (4.0 * w + 3.0 * at * dl)) / np.where(ok, room, 1.0) + SAFETY * U * at, INF)
        rho = SAFETY * U * (dl * at + pl)
        dq = dl * tau + rho
        front_p = ~tr.zero_area[None, :] & (tr.unconstrained[None, :] | (denom <= DENOM_MAX + d_denom))
        front_d = ok & (denom <= DENOM_MAX - d_denom)
        oc = o @ tr.cen.T
        along = ((d @ tr.cen.T) - od) / dl
        body = tr.rb[None, :] * (1.0 + 2.0 * nu) + tr.overshoot[None, :]
        reach = body + SAFETY * U * (ol + 2.0 * (np.sqrt(tr.cc)[None, :] + body))
        passes = ~(oo - 2.0 * oc + tr.cc[None, :] - along * along > reach * reach) | tr.unconstrained[None, :]       # item 6
        in_p = front_p & (t >= -tau) & passes
        in_d = front_d & (t >= tau)
        near = np.zeros((R, tr.n), bool)
        edge_ratio = np.full((R, tr.n), -INF)
        for k in range(3):
            s = (o @ tr.m[:, k].T) + t * (d @ tr.m[:, k].T) - tr.c[None, :, k]
            delta = np.abs(d @ tr.m[:, k].T) * tau + rho + (q[k] + dq) * (nu * nu / SAFETY + SAFETY * 14.0 * U) + dq * nu
            delta = np.where(ok, delta, INF)
            in_p &= ~(s < -delta)
            in_d &= s >= delta
            scale = q[k] + np.abs(s) + delta
            near |= ok & ((np.abs(s - delta) <= 1e-9 * scale) | (np.abs(s + delta) <= 1e-9 * scale))
            edge_ratio = np.maximum(edge_ratio, np.where(ok & (delta > 0), -s / np.where(ok & (delta > 0), delta, 1.0), -INF))
        near |= ok & ((np.abs(t - tau) <= 1e-9 * (at + tau)) | (np.abs(t + tau) <= 1e-9 * (at + tau)))
        near |= ok & (np.abs(np.abs(denom - DENOM_MAX) - d_denom) <= 1e-9 * d_denom)
        in_d &= in_p
    return _reduce(in_p, in_d, t, tau, edge_ratio, answer_k), (near, in_p, in_d, t, tau, edge_ratio, passes)


def _reduce(in_p, in_d, t, tau, edge_ratio, answer_k):
    """The per-ray figures classify() documents, from the memberships of P and D (rays x triangles)"""
    R, T = in_p.shape
    out = {}
    upper = np.where(in_d, t + tau, INF)                              # a decisive triangle is accepted by f32 no later than this
    out["d_upper"] = upper.min(1)
    td = np.where(in_d, t, INF)
    kd = td.argmin(1)
    out["t_d"], out["k_d"] = td.min(1), np.where(in_d.any(1), kd, -1)
    lower = np.where(in_p, t - tau, INF)                              # a possible triangle is accepted by f32 no earlier than this
    lower[np.arange(R), kd] = INF
    up_kd = np.take_along_axis(upper, kd[:, None], 1)[:, 0]
    out["unique"] = in_d.any(1) & (lower.min(1) > up_kd)               # rule 3's premise
    out["n_p"], out["n_d"] = in_p.sum(1), in_d.sum(1)
    out["p_not_d"] = (in_p & ~in_d).any(1)
    k = np.clip(answer_k, 0, max(T - 1, 0))[:, None]
    out["ans_in_p"] = np.take_along_axis(in_p, k, 1)[:, 0]
    out["ans_t"], out["ans_tau"] = np.take_along_axis(t, k, 1)[:, 0], np.take_along_axis(tau, k, 1)[:, 0]
    out["ans_edge_ratio"] = np.take_along_axis(edge_ratio, k, 1)[:, 0]
    return out


def exact_pair(ray, tri):
    """One ray / triangle pair in rationals -> (dN, t, [W_k], N): what is rational of the module's first paragraph, dN = d . N = denom |N|,
    t = (v0 - o) . N / dN (None when dN is 0) and W_k = (E_k x (p - v_k)) . N = s_k |E_k| |N|."""
    F = [Fraction(float(x)) for x in np.asarray(ray, np.float32)]
    o, d = F[:3], F[3:]
    v = [[Fraction(float(x)) for x in row] for row in np.asarray(tri, np.float32).reshape(3, 3)]
    sub = lambda a, b: [a[i] - b[i] for i in range(3)]  # noqa: E731
    dot = lambda a, b: a[0] * b[0] + a[1] * b[1] + a[2] * b[2]  # noqa: E731
    cross = lambda a, b: [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]  # noqa: E731
    N = cross(sub(v[1], v[0]), sub(v[2], v[0]))
    dN = dot(d, N)
    if dN == 0:
        return dN, None, None, N
    t = dot(sub(v[0], o), N) / dN
    p = [o[i] + d[i] * t for i in range(3)]
    W = [dot(cross(sub(v[(k + 1) % 3], v[k]), sub(p, v[k])), N) for k in range(3)]
    return dN, t, W, N


def _resolve_pair(tr, ray, j, in_p, in_d):
    """The pair's membership of P and D with the float64 values of denom, t* and s_k replaced by correctly rounded rationals (the bounds
    keep their float64 values: they are bounds, and a 1e-16 change of one is nothing next to SAFETY)."""
    if tr.unconstrained[j] or tr.zero_area[j]:
        return in_p, in_d
    dN, t, W, N = exact_pair(ray, tr.v[j])
    if t is None:
        return in_p, False
    NN = float(N[0] * N[0] + N[1] * N[1] + N[2] * N[2])
    nl = NN ** 0.5
    o, d = ray[:3].astype(np.float64), ray[3:].astype(np.float64)
    dl, ol = float(np.linalg.norm(d)), float(np.linalg.norm(o))
    nu = SAFETY * tr.nu[j]
    denom, tf = float(dN) / nl, float(t)
    d_denom = dl * (nu + SAFETY * 3.0 * U)
    room = abs(denom) - d_denom
    if not room > 0:
        return denom <= DENOM_MAX + d_denom, False
    p = o + d * tf
    q = [float(np.linalg.norm(p - tr.v[j, k])) for k in range(3)]
    w = float(np.linalg.norm(tr.v[j, 0] - o))
    tau = (nu * q[0] + SAFETY * U * (4.0 * w + 3.0 * abs(tf) * dl)) / room + SAFETY * U * abs(tf)
    rho = SAFETY * U * (dl * abs(tf) + min(ol + abs(tf) * dl, float(np.linalg.norm(tr.v[j, 0])) + q[0]))
    dq = dl * tau + rho
    p_ok, d_ok = denom <= DENOM_MAX + d_denom and tf >= -tau, denom <= DENOM_MAX - d_denom and tf >= tau
    for k in range(3):
        El = float(np.linalg.norm(tr.v[j, (k + 1) % 3] - tr.v[j, k]))
        s = float(W[k]) / (El * nl) if El > 0 else 0.0
        delta = abs(float(d @ tr.m[j, k])) * tau + rho + (q[k] + dq) * (nu * nu / SAFETY + SAFETY * 14.0 * U) + dq * nu
        p_ok, d_ok = p_ok and not s < -delta, d_ok and s >= delta
    return p_ok, d_ok and p_ok


def classify(vertices, rays, answer_k=None, chunk_pairs=1 << 19):
    """rays (n, 6) f32, finite, against the triangles -> dict of per-ray arrays:
      n_p, n_d: the sizes of P and D;  p_not_d: P \\ D is not empty;  t_d, k_d: min t* over D (inf) and its triangle (-1)
      d_upper: min over D of t* + tau (inf): f32 accepts something no later than this
      unique: D's nearest element is the only member of P that f32 can accept at or before its own latest acceptance
      ans_in_p, ans_t, ans_tau, ans_edge_ratio: for triangle answer_k[ray]: membership of P, t*, tau, and max_k -s_k / delta_k
      resolved: how many pairs were decided again in rationals"""
    tr = vertices if isinstance(vertices, Triangles) else Triangles(vertices)
    rays = np.ascontiguousarray(rays, np.float32)
    assert np.all(np.isfinite(rays)), "exact_mesh takes finite rays"
    r64 = rays.astype(np.float64)
    n = len(rays)
    ak = np.zeros(n, np.int64) if answer_k is None else np.asarray(answer_k, np.int64)
    step = max(1, chunk_pairs // max(tr.n, 1))
    starts = list(range(0, n, step))

    def one(a):
        out, (near, in_p, in_d, t, tau, edge_ratio, passes) = _classify_chunk(tr, r64[a:a + step], ak[a:a + step])
        rows, cols = np.nonzero(near)
        if rows.size:                                 # decide those pairs again in rationals, then redo every figure of the chunk
            for i, j in zip(rows, cols):
                in_p[i, j], in_d[i, j] = _resolve_pair(tr, rays[a + i], j, in_p[i, j], in_d[i, j])
                in_p[i, j] &= passes[i, j]             # (item 6 is no boundary of the three: it stands)
                in_d[i, j] &= in_p[i, j]
            out = _reduce(in_p, in_d, t, tau, edge_ratio, ak[a:a + step])
        out["resolved"] = int(rows.size)
        return out

    with ThreadPoolExecutor(THREADS) as pool:
        parts = list(pool.map(one, starts))
    res = {k: np.concatenate([p[k] for p in parts]) for k in parts[0] if k != "resolved"} if parts else {}
    res["resolved"] = sum(p["resolved"] for p in parts)
    return res


def check_answers(vertices, rays, answer, first_triangle=0, what=""):
    """An answer (t, idx, just) of the code under test (a miss: just 0) for finite rays, against the rules:
      1. just, and the primitive is triangle k:  k is in P;  |t - t*_k| <= tau_k;  t <= min over D of (t* + tau) -- nothing that is
         decisively hit lies decisively nearer.  (A sphere or plane answer, idx < first_triangle: the last clause only.)
      2. not just: D is empty.
      3. D's nearest element is the only member of P f32 can accept that early (classify's `unique`): the answer is that triangle.
    -> a dict of figures: the three shares that keep the check from passing vacuously and the largest error-to-bound ratios."""
    t, idx, just = (np.asarray(x) for x in answer)
    just = just.astype(bool)
    k = np.where(just & (idx >= first_triangle), idx - first_triangle, 0)
    c = classify(vertices, rays, k)
    on_tri = just & (idx >= first_triangle)
    t64 = t.astype(np.float64)

    def fail(mask, rule):
        bad = np.flatnonzero(mask)
        assert bad.size == 0, "%s: rule %s fails for %d of %d rays, e.g. ray %d %r: answer (%r, %d, %d); P %d, D %d, t_D %r, t*_k %r, tau_k %r" % (
            what, rule, bad.size, len(t), bad[0], rays[bad[0]].tolist(), t[bad[0]], idx[bad[0]], just[bad[0]], c["n_p"][bad[0]],
            c["n_d"][bad[0]], c["t_d"][bad[0]], c["ans_t"][bad[0]], c["ans_tau"][bad[0]])

    fail(on_tri & ~c["ans_in_p"], "1 (the triangle is in P)")
    fail(on_tri & ~(np.abs(t64 - c["ans_t"]) <= c["ans_tau"]), "1 (|t - t*| <= tau)")
    fail(just & ~(t64 <= c["d_upper"]), "1 (nothing decisive lies decisively nearer)")
    fail(~just & (c["n_d"] > 0), "2 (Nothing, but D is not empty)")
    fail(c["unique"] & ~(on_tri & (k == c["k_d"])) & ~(just & (idx < first_triangle)), "3 (the one decisive candidate)")
    finite = on_tri & np.isfinite(c["ans_tau"]) & (c["ans_tau"] > 0)
    n = max(len(t), 1)
    return {"rays": len(t), "share_d": float(np.mean(c["n_d"] > 0)), "share_p_not_d": float(np.mean(c["p_not_d"])),
            "share_nothing": float(np.sum(~just & (c["n_p"] == 0)) / n),
            "t_ratio": float(np.max(np.abs(t64 - c["ans_t"])[finite] / c["ans_tau"][finite])) if finite.any() else 0.0,
            "edge_ratio": float(max(0.0, np.max(c["ans_edge_ratio"][finite]))) if finite.any() else 0.0,
            "unique": int(c["unique"].sum()), "resolved": c["resolved"], "classes": c}


def assert_shares(fig, what=""):
    assert fig["share_d"] >= 0.30, "%s: only %.1f %% of the rays have a decisive hit" % (what, 100 * fig["share_d"])
    assert fig["share_p_not_d"] >= 0.05, "%s: only %.1f %% of the rays have an undecidable candidate" % (what, 100 * fig["share_p_not_d"])
    assert fig["share_nothing"] >= 0.01, "%s: only %.2f %% of the rays are answered Nothing with an empty P" % (what, 100 * fig["share_nothing"])


def normal_errors(vertices, stored_normals):
    """Rule 4: the stored normals (n, 3) f32 (NaN for zero area) against n^ -> (error, bound, constrained) per triangle; the bound is
    SAFETY nu (item 1), asserted by the caller where `constrained`"""
    tr = vertices if isinstance(vertices, Triangles) else Triangles(vertices)
    got = np.asarray(stored_normals, np.float64).reshape(-1, 3)
    err = np.linalg.norm(got - tr.nhat, axis=1)
    return err, SAFETY * tr.raw_nu, ~tr.unconstrained & ~tr.zero_area, tr
