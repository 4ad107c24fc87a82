"""The render path in plain numpy float64, vectorised over pixels, written from the reference's TEXT: what the oracle (oracle/pt_oracle.c)
and the device are held to where the suite otherwise only shows that they agree with each other.  Nothing here imports the oracle or the
package's arithmetic; scene records, dtypes and cameras are world.py's (data), the float64 triangle is tests/exact_mesh.py's.

What is restated, and from where (paths relative to the reference root; every function names its lines again):
  render, both algorithms      src/Scene/Trace.hs:135-200        primaryRays                 src/Scene/Trace.hs:205-262
  traceStep, numNewRays        src/Scene/Trace.hs:272-331        traceInline, calcNextRay    src/Scene/Trace.hs:344-435
  checkHit, infinite, epsilon  src/Scene/Trace.hs:443-456        distanceTo, hit, normal     src/Scene/Intersection.hs:29-64
  anglesToDirection/Quaternion src/Util.hs:48-67                 genVec                      src/Util.hs:114-118
  mapScene, expMinWith         src/Util.hs:156-178
Dependencies of the reference that are not in its tree, by their PUBLISHED definitions (SURVEY.md and oracle/pt_oracle.c's header name the
same readings):
  linear:  dot (V3 a b c) (V3 d e f) = a d + b e + c f;  cross;  quadrance v = dot v v;  Quaternion product
           q1 q2 = (s1 s2 - v1 . v2,  v1 x v2 + s1 v2 + s2 v1);  rotate q v = vector part of q (0, v) conj(q);
           nearZero (Float) a = |a| <= 1e-6;  nearZero (V3) = nearZero . quadrance;
           normalize v = v when nearZero l or nearZero (1 - l), else v / sqrt l, l = quadrance v.
  sfc-random-accelerate: PractRand's sfc32 -- tmp = a + b + counter; counter += 1; a = b ^ (b >> 9); b = c + (c << 3);
           c = rotl(c, 21) + tmp; output tmp -- seeded (a, b, c), counter 1, 15 outputs discarded;  random @Float = mwc-random's
           wordToFloat: the word as an Int32 i, fromIntegral i * 2^-32 + 0.5 + 2^-33 in f32.  That f32 value IS the draw (part of the
           generator's definition, computed here in f32 exactly, then widened); everything after it is float64.
GLASS and triangles are this project's extensions: GLASS as the formula block above glass_children (oracle/pt_oracle.c) and the same
wording in include/ptmi.h define it, a triangle as include/ptmi.h defines it (a bounded one-sided plane).

PER PIXEL the reference returns the float64 colour the call adds, the exact final generator state, the primitives hit, `decided`, and an
error bound for the colour.

DECIDED.  f32 cannot take the float64 branch where an operand is within its own f32 uncertainty of the boundary.  A pixel is undecided
when any branch on its path has such a margin: a primitive's hit-or-miss tests (sphere: tca < 0, d2 > r^2, t < 0; plane and triangle:
denom > 1e-6, t < 0, the edge functions) for the nearest primitive or for one that could be nearer, nearest against runner-up (a tie that
is exact in float64 is resolved by the fold's order, in f32 too for bitwise equal primitives, and counts as decided), nearZero of the
throughput, Glossy's max 0, GLASS's k < 0.  normalize's own nearZero (1 - l) is no branch of the path: either side returns a vector within
|1 - 1 / sqrt l| <= 5.1e-7 of the other, which the bound carries as an error (NORMALIZE_SKIP) wherever |1 - l| <= 2e-6.

THE BOUND: a forward analysis, first order in u = 2^-24, of every f32 step, carried along the path with the path's own amplification;
each quantity below is a bound on a Euclidean norm (vectors) or an absolute value, in terms of the float64 path's own magnitudes only.
Nothing was fitted to any output of the oracle or the device.  Carried per ray: eo, ed (origin, direction), dS (the scalar throughput S;
the colour part C of the throughput C S is a product of inputs and only rounds).
  rounding:  a sum or product of f32 values errs by u relative; an n-term dot product by n u |a| |b|; constants (pi, 1 / (2 pi), 0.002) by u.
  draws:     rv = x * 2 - 1 is exact for x >= 1/2 and rounds by at most u / 2 below.
  angles:    a = k rv (k = pi or 1 - p):  da = |k| u / 2 + 2 u |a|;  a half angle is exact;  sin / cos in f32 of an f32 argument: u
             (one unit in the last place of a value below 1);  e = da / 2 + u per sine and cosine.
  quaternion each component is a sum of two triple products x y z of them:  e (|y z| + |x z| + |x y|) + 2 u |x y z| each, u for the sum;
             |dq| is the norm of the four.
  rotate     q (0, v) conj q:  (2 |dq| + 12 u) |v| + dv   (two quaternion products, about six roundings a component).
  sphere     l = c - o: dl = eo + u |l|;  tca = l . d: dtca = dl |d| + |l| ed + 3 u |l| |d|;  |l|^2: dll = 2 |l| dl + 3 u |l|^2;
             m = r^2 - |l|^2 + tca^2: dm = dll + 2 |tca| dtca + u tca^2 + u |d2| + u r^2;  t = tca - sqrt m:
             dt = |1 - tca / thc| dtca + (dm - 2 |tca| dtca) / (2 thc) + u thc + u |t|.   This is where a path amplifies: 1 / thc grows
             towards a sphere's limb.
  own surface a ray that leaves a primitive starts 0.002 off it, and whether it meets that primitive again turns on that offset.  The
             ray's error moved the hit point ALONG the surface, not off it: across the surface it has just left the origin errs by `off`
             only -- the rounding of t and of o + d t (dt with eo = ed = 0), dp^2 / r on a sphere, 0.002 ed' of the new direction -- and
             that is what enters dll (sphere), dnum (plane) and tau (triangle) for that one primitive.
  plane      denom = d . n: ed |n| + 3 u |d| |n|;  num = (p0 - o) . n: (eo + u |w|) |n| + 3 u |w| |n|, w = p0 - o;
             dt = (dnum + |t| ddenom) / |denom| + u |t|.
  triangle   exact_mesh's items 2 to 5 with its nu, tau and delta_k, plus the ray's own error: ddenom += ed; tau's numerator += eo + |t| ed;
             delta_k += eo + |t| ed (the lateral shift of the hit point).
  hit point  p = o + d t:  dp = eo + |t| ed + |d| dt + u (|p| + |d| |t|).
  normal     sphere: (dp + u r) / r + 3 u + NORMALIZE_SKIP;  plane: 0 (an input);  triangle: nu.
  Matte      next = rotate q n: e_rot + dn;  b = p / pi (next . n): db = (p / pi) (|n| dnext + |next| dn + 3 u |next| |n|) + 3 u |b|.
  Glossy     a = d . n: da = ed |n| + |d| dn + 3 u |d| |n|;  refl = d - 2 a n: ed + 2 da |n| + 2 |a| dn + 4 u (|d| + 2 |a| |n|);
             next = rotate q refl;  b = max 0 (next . refl): |refl| dnext + |next| drefl + 3 u |next| |refl|.
  GLASS      dn and refl as Glossy; k = 1 - eta^2 (1 - cosi^2): dk = eta^2 2 |cosi| da + 6 u;  m = 1 - cosi: da + u;
             R: (1 - r0) (5 m^4 dm + 6 u |m|^5) + 4 u;  refr = eta d + (eta cosi - sqrt k) n:
             eta ed + (eta da + dk / (2 sqrt k) + 3 u) |n| + |eta cosi - sqrt k| dn + 3 u |refr|.
  next ray   origin p + next * 0.002:  eo' = dp + 0.002 ed' + u (|p| + 0.004 |next|).
  throughput S' = S f, f = b / (2 pi):  df = db / (2 pi) + 3 u |f|;  dS' = |f| dS + |S| df + 3 u |S'|  (the colour's two roundings included).
  a term     E C S added to the pixel (E = colour * illuminance):  |E C| (dS + 3 u |S|).
  the sums   f32 accumulation of n added terms in the kernel's own order:  (n - 1) 2^-24 sum |term|   (ACCUMULATION); n counts every f32
             addition into the pixel, `new + old` of each sample included.  The stream form adds a pixel's terms in NO defined order:
             the same expression with the stream form's term count bounds every order (UNORDERED; n is then the number of hits).
  SAFETY = 2 multiplies every bound and every margin, for what first order drops -- the project's precedent (exact_mesh.py).
A fused a * b + c rounds once where this analysis counts two roundings, so the bound holds for contracted arithmetic as well.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import exact_mesh  # noqa: E402

U = 2.0 ** -24
SAFETY = 2.0
NEAR_ZERO = float(np.float32(1e-6))            # linear's nearZero, and the plane's denom > 1e-6: the f32 constant
EPSILON = 0.002                                # Trace.hs:455-456
NORMALIZE_SKIP = 5.1e-7
MATTE, GLOSSY, GLASS = 0, 1, 2
INLINE, STREAMS_KEEP, STREAMS_FROM_RESULT, TREE = "inline", "streams_keep", "streams_from_result", "tree"
_M32 = np.uint32(0xFFFFFFFF)


# ---- the generator (integers; published algorithm) -------------------------------------------------------------------------------------
def sfc32_step(state):
    """One sfc32 step on four uint32 arrays -> (output, new state)"""
    a, b, c, n = state
    with np.errstate(over="ignore"):
        tmp = a + b + n
        n2 = n + np.uint32(1)
        a2 = b ^ (b >> np.uint32(9))
        b2 = c + (c << np.uint32(3))
        c2 = ((c << np.uint32(21)) | (c >> np.uint32(11))) + tmp
    return tmp, (a2, b2, c2, n2)


def sfc32_seed(a, b, c):
    """PractRand's three-word seeding: counter 1, 15 outputs discarded (A2).  render() takes its start planes as data, so this is exercised
    by tests/test_render_exact.py's test_the_generator_is_the_oracles alone"""
    state = tuple(np.asarray(x, np.uint32) for x in (a, b, c)) + (np.ones_like(np.asarray(a, np.uint32)),)
    for _ in range(15):
        _, state = sfc32_step(state)
    return state


def random_float(state):
    """random @Float = wordToFloat, in f32 operation for operation, widened -> (float64 array, new state)"""
    word, state = sfc32_step(state)
    i = word.view(np.int32).astype(np.float32)
    x = (i * np.float32(2.0 ** -32) + np.float32(0.5)) + np.float32(2.0 ** -33)
    return x.astype(np.float64), state


def gen_vec(state):
    """Util.hs:114-118: three draws, each x * 2 - 1"""
    out = []
    for _ in range(3):
        x, state = random_float(state)
        out.append(x * 2.0 - 1.0)
    return np.stack(out, -1), state


# ---- vectors -------------------------------------------------------------------------------------------------------------------------------
def dot(a, b):
    return a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2]


def norm(a):
    return np.sqrt(dot(a, a))


def near_zero(x):
    return np.abs(x) <= NEAR_ZERO


def normalize(v):
    """linear's normalize -> (vector, whether |1 - l| is close enough to 1e-6 for f32 to branch the other way)"""
    l = dot(v, v)
    keep = near_zero(l) | near_zero(1.0 - l)
    with np.errstate(divide="ignore", invalid="ignore"):
        out = np.where(keep[..., None], v, v / np.sqrt(l)[..., None])
    return out, np.abs(1.0 - l) <= 2.0 * NEAR_ZERO


def angles_to_quaternion(angles):
    """Util.hs:55-67: (roll, pitch, yaw) -> (w, (x, y, z))"""
    roll, pitch, yaw = angles[..., 0], angles[..., 1], angles[..., 2]
    cy, sy = np.cos(yaw * 0.5), np.sin(yaw * 0.5)
    cp, sp = np.cos(pitch * 0.5), np.sin(pitch * 0.5)
    cr, sr = np.cos(roll * 0.5), np.sin(roll * 0.5)
    w = cy * cp * cr + sy * sp * sr
    v = np.stack([cy * cp * sr - sy * sp * cr, sy * cp * sr + cy * sp * cr, sy * cp * cr - cy * sp * sr], -1)
    return w, v


def _qmul(s1, v1, s2, v2):
    return s1 * s2 - dot(v1, v2), np.cross(v1, v2) + s1[..., None] * v2 + s2[..., None] * v1


def rotate(q, v):
    """linear's rotate: the vector part of q (0, v) conj(q)"""
    w, qv = q
    s, x = _qmul(w, qv, np.zeros_like(w), v)
    return _qmul(s, x, w, -qv)[1]


def rotation_error(k, angles):
    """|d(rotate q v)| / |v| for q = anglesToQuaternion (k rv), without dv (module docstring: angles, quaternion, rotate), with the
    magnitudes of q's own six sines and cosines"""
    da = abs(k) * U / 2.0 + 2.0 * U * np.abs(angles)
    e = da / 2.0 + U                                                          # of each sine and cosine
    c, s = np.abs(np.cos(angles * 0.5)), np.abs(np.sin(angles * 0.5))
    (cr, cp, cy), (sr, sp, sy), (er, ep, ey) = (c[..., i] for i in range(3)), (s[..., i] for i in range(3)), (e[..., i] for i in range(3))

    def term(x, y, z):                                                         # a triple product of three of them, each off by its e
        return ey * y * z + ep * x * z + er * x * y + 2.0 * U * x * y * z
    comps = [term(cy, cp, cr) + term(sy, sp, sr), term(cy, cp, sr) + term(sy, sp, cr), term(sy, cp, sr) + term(cy, sp, cr),
             term(sy, cp, cr) + term(cy, sp, sr)]
    comps = [x + U for x in comps]                                             # the sum or difference of the two
    dq = np.sqrt(sum(x * x for x in comps))
    return 2.0 * dq + 12.0 * U


# ---- the scene -----------------------------------------------------------------------------------------------------------------------------
class Scene:
    """spheres ++ planes ++ triangles as float64 arrays (the f32 records taken as exact); primitive index in that order (Util.hs:156-158)"""

    def __init__(self, spheres, planes, triangles=None):
        s, p = np.asarray(spheres).reshape(-1), np.asarray(planes).reshape(-1)
        self.ns, self.np_ = len(s), len(p)
        self.s_pos, self.s_rad = s["position"].astype(np.float64).reshape(-1, 3), s["radius"].astype(np.float64)
        self.p_pos, self.p_nor = p["position"].astype(np.float64).reshape(-1, 3), p["direction"].astype(np.float64).reshape(-1, 3)
        parts = [s, p]
        self.tr = None
        self.nt = 0
        if triangles is not None and len(triangles):
            t = np.asarray(triangles).reshape(-1)
            self.tr = exact_mesh.Triangles(np.stack([t["v0"], t["v1"], t["v2"]], 1))
            assert not self.tr.unconstrained.any(), "a triangle whose f32 normal says nothing about its plane has no place in a render test"
            self.nt = len(t)
            parts.append(t)
        self.n = self.ns + self.np_ + self.nt
        self.color = np.concatenate([x["color"].astype(np.float64).reshape(-1, 3) for x in parts])
        self.illuminance = np.concatenate([x["illuminance"].astype(np.float64) for x in parts])
        self.tag = np.concatenate([x["brdf_tag"].astype(np.int64) for x in parts])
        self.param = np.concatenate([x["brdf_param"].astype(np.float64) for x in parts])
        self.kind = np.concatenate([np.zeros(self.ns, int), np.ones(self.np_, int), np.full(self.nt, 2)])


HIT, MISS, MAYBE = 1, 0, 2


def _status(yes, no):
    return np.where(yes, HIT, np.where(no, MISS, MAYBE))


def check_hit(scene, o, d, eo, ed, prev=None, eoff=None):
    """checkHit (Trace.hs:443-447) as the literal fold (Util.hs:171-178: `valA <= valB` keeps the earlier primitive; a miss has the key
    `infinite`), over spheres (Intersection.hs:39-48), planes (:57-62) and triangles, for rays (N, 3) with error bounds eo, ed (N,);
    prev (N,): the primitive the ray has just left (-1: none), eoff (N,): how far off THAT surface the origin's error can be (see `off`)
    -> dict: idx (-1: Nothing), t, p, n (hit's position and normal, Intersection.hs:29-32, :50, :64), dp, dn, off, decided"""
    N = len(o)
    T = np.full((N, scene.n), np.inf)                 # the key of every primitive (inf: Nothing)
    LO = np.full((N, scene.n), np.inf)                # the earliest f32 can accept it (inf: it certainly cannot)
    DT = np.zeros((N, scene.n))
    DTR = np.zeros((N, scene.n))                      # ... of which rounding alone (the ray taken as exact)
    ST = np.zeros((N, scene.n), np.int8)
    D = norm(d)[:, None]
    eo_, ed_ = eo[:, None], ed[:, None]
    # EO: the origin's error ACROSS each primitive's surface.  It is eo for every primitive but the one the ray has just left.  For that one
    # the f32 origin is p32 + next32 * 0.002 with p32 the f32 hit point, which f32 FOUND on that surface: whatever error the incoming ray
    # carried moved p32 along the surface (it is where the erring ray meets it), and off it only by the rounding of that one intersection
    # (`off`: dt with eo = ed = 0, the rounding of o + d t, and dp^2 / r for a sphere's curvature under a lateral shift of dp).  So across
    # that surface the origin errs by eoff = off + 0.002 ed' + the rounding of the sum, never by more than eo (the minimum below), and this
    # narrows only the own-surface test -- whether a ray that starts 0.002 off a surface meets it again -- which full eo (grown along the
    # path) would leave undecided at every bounce.  It enters where the across-surface component enters: dll (sphere), dnum (plane), tau
    # (triangle); the lateral part of the sphere's dtca keeps the full eo.  Too small an eoff would call a pixel decided that f32 takes
    # the other way: that shows as a FAILING pixel (wrong seed or colour), never as a hidden one.
    EO = np.repeat(eo_, scene.n, 1)
    if prev is not None:
        has = prev >= 0
        EO[np.flatnonzero(has), prev[has]] = np.minimum(eoff[has], eo[has])
    S = SAFETY
    with np.errstate(all="ignore"):
        if scene.ns:                                                                  # Intersection.hs:39-48
            sl = slice(0, scene.ns)
            l = scene.s_pos[None, :, :] - o[:, None, :]
            tca = dot(l, d[:, None, :])
            ll = dot(l, l)
            d2 = ll - tca * tca
            rad2 = scene.s_rad[None, :] ** 2
            thc = np.sqrt(rad2 - d2)
            t = np.minimum(tca - thc, tca + thc)
            miss = (tca < 0) | (d2 > rad2) | (t < 0)
            L = np.sqrt(ll)

            def sphere_dt(eo_lat, eo_rad, ed_):
                dtca = (eo_lat + U * L) * D + L * ed_ + 3.0 * U * L * D
                dll = 2.0 * L * (eo_rad + U * L) + 3.0 * U * ll       # |l|^2 feels the origin's error along l only
                dm = dll + 2.0 * np.abs(tca) * dtca + U * tca * tca + U * np.abs(d2) + U * rad2
                # t = tca - sqrt (r^2 - |l|^2 + tca^2):  dt / dtca = 1 - tca / thc, which cancels for a ray that starts on the sphere
                dt = np.abs(1.0 - tca / thc) * dtca + (dm - 2.0 * np.abs(tca) * dtca) / (2.0 * thc) + U * thc + U * np.abs(t)
                return dtca, dm, dt
            dtca, dm, dt = sphere_dt(eo_, EO[:, sl], ed_)
            m = rad2 - d2
            inside, outside = m > S * dm, m < -S * dm
            yes = (tca > S * dtca) & inside & (t > S * dt)
            no = (tca < -S * dtca) | outside | (inside & (t < -S * dt))
            T[:, sl] = np.where(miss | np.isnan(t), np.inf, t)
            ST[:, sl] = _status(yes, no)
            DT[:, sl] = np.where(yes, dt, 0.0)
            DTR[:, sl] = np.where(yes, sphere_dt(0.0, 0.0, 0.0)[2], 0.0)
            est = tca - S * dtca - np.sqrt(np.maximum(m, 0.0) + S * dm)
            LO[:, sl] = np.where(yes, t - S * dt, np.where(no, np.inf, np.maximum(est, 0.0)))
        if scene.np_:                                                                 # Intersection.hs:57-62
            sl = slice(scene.ns, scene.ns + scene.np_)
            nor = scene.p_nor[None, :, :]
            Nn = norm(scene.p_nor)[None, :]
            denom = dot(d[:, None, :], nor)
            wv = scene.p_pos[None, :, :] - o[:, None, :]
            num = dot(wv, nor)
            t = num / denom
            miss = (denom > NEAR_ZERO) | (t < 0)
            W = norm(wv)

            def plane_dt(eo_across, ed_):
                ddenom = ed_ * Nn + 3.0 * U * D * Nn
                dnum = (eo_across + U * W) * Nn + 3.0 * U * W * Nn
                return ddenom, (dnum + np.abs(t) * ddenom) / np.abs(denom) + U * np.abs(t)
            ddenom, dt = plane_dt(EO[:, sl], ed_)
            front, back = denom < NEAR_ZERO - S * ddenom, denom > NEAR_ZERO + S * ddenom
            yes = front & (t > S * dt)
            no = back | (t < -S * dt)
            T[:, sl] = np.where(miss | np.isnan(t), np.inf, t)
            ST[:, sl] = _status(yes, no)
            DT[:, sl] = np.where(yes, dt, 0.0)
            DTR[:, sl] = np.where(yes, plane_dt(0.0, 0.0)[1], 0.0)
            lo = np.where(np.isfinite(t) & np.isfinite(dt), np.maximum(t - S * dt, 0.0), 0.0)
            LO[:, sl] = np.where(yes, t - S * dt, np.where(no, np.inf, lo))
        if scene.nt:                                                                  # include/ptmi.h's triangle, exact_mesh's float64 form
            sl = slice(scene.ns + scene.np_, scene.n)
            tr = scene.tr
            nu = tr.nu[None, :]
            denom = d @ tr.nhat.T
            t = (tr.v0n[None, :] - o @ tr.nhat.T) / denom
            p = o[:, None, :] + d[:, None, :] * t[:, :, None]
            s_k = [(o @ tr.m[:, k].T) + t * (d @ tr.m[:, k].T) - tr.c[None, :, k] for k in range(3)]
            miss = (denom > NEAR_ZERO) | (t < 0) | (s_k[0] < 0) | (s_k[1] < 0) | (s_k[2] < 0) | tr.zero_area[None, :]
            q = [norm(p - tr.v[None, :, k, :]) for k in range(3)]
            W = norm(tr.v[None, :, 0, :] - o[:, None, :])

            def triangle_dt(eo_across, ed_):
                ddenom = D * (nu + 3.0 * U) + ed_                                     # item 2
                room = np.abs(denom) - S * ddenom
                tau = np.where(room > 0, (nu * q[0] + U * (4.0 * W + 3.0 * np.abs(t) * D) + eo_across + np.abs(t) * ed_) / room
                               + U * np.abs(t), np.inf)                              # item 3
                return ddenom, tau
            ddenom, tau = triangle_dt(EO[:, sl], ed_)
            lateral = eo_ + np.abs(t) * ed_
            rho = U * (D * np.abs(t) + norm(p))                                       # item 4
            dq = D * tau + rho + lateral
            front, back = denom < NEAR_ZERO - S * ddenom, denom > NEAR_ZERO + S * ddenom
            yes = front & (t > S * tau)
            no = back | (t < -S * tau) | tr.zero_area[None, :]
            for k in range(3):                                                         # item 5
                delta = np.abs(d @ tr.m[:, k].T) * tau + rho + (q[k] + dq) * (nu * nu + 14.0 * U) + dq * nu + lateral
                yes &= s_k[k] > S * delta
                no |= s_k[k] < -S * delta
            yes &= ~no
            T[:, sl] = np.where(miss | np.isnan(t), np.inf, t)
            ST[:, sl] = _status(yes, no)
            DT[:, sl] = np.where(yes, tau, 0.0)
            DTR[:, sl] = np.where(yes, triangle_dt(0.0, 0.0)[1], 0.0)
            lo = np.where(np.isfinite(t) & np.isfinite(tau), np.maximum(t - S * tau, 0.0), 0.0)
            LO[:, sl] = np.where(yes, t - S * tau, np.where(no, np.inf, lo))
    # The fold (Util.hs:171-178) over finite keys and `infinite`: `valA <= valB` keeps the earlier of two equal keys, so what it returns is
    # the FIRST of the smallest keys, which is argmin.  The two differ only for a NaN key, which the fold would carry (every comparison with
    # it is false) and which is written as a miss above.  A key is NaN only for 0 / 0 -- a plane or triangle with denom exactly 0 and the
    # origin in its plane; a sphere's NaN (the root of a negative) is a miss by d2 > r^2 already.  Such a primitive is MAYBE with LO = 0
    # (neither `yes` nor `no` holds of a NaN), so `others.min` below is 0 and the pixel is undecided: nothing is asserted of its colour or seed.
    idx = T.argmin(1)
    rows = np.arange(N)
    t = T[rows, idx]
    just = np.isfinite(t)
    dt, dtr = DT[rows, idx], DTR[rows, idx]
    others = LO.copy()
    others[rows, idx] = np.inf
    others[(T == t[:, None]) & (ST == HIT)] = np.inf   # a tie exact in float64: the fold's order decides, here and in f32
    decided = np.where(just, (ST[rows, idx] == HIT) & (others.min(1) > t + SAFETY * dt), (ST == MISS).all(1))
    idx = np.where(just, idx, -1)
    tt = np.where(just, t, 0.0)
    p = o + d * tt[:, None]                            # Intersection.hs:32
    Dn = D[:, 0]
    dp = eo + np.abs(tt) * ed + Dn * dt + U * (norm(p) + Dn * np.abs(tt))
    n = np.zeros((N, 3))
    dn = np.zeros(N)
    k = np.clip(idx, 0, None)
    sph = just & (idx < scene.ns)
    # off: how far from the surface it was found on the f32 hit point can be.  The ray's own error moves the point ALONG the surface (on a
    # sphere of radius r it leaves the tangent plane by dp^2 / r); across it only the rounding of t and of o + d t counts
    off = Dn * dtr + U * (norm(p) + Dn * np.abs(tt))
    if sph.any():                                      # Intersection.hs:50
        nn, close = normalize(p[sph] - scene.s_pos[k[sph]])
        n[sph] = nn
        rad = scene.s_rad[k[sph]]
        dn[sph] = (dp[sph] + U * rad) / rad + 3.0 * U + np.where(close, NORMALIZE_SKIP, 0.0)
        off[sph] += dp[sph] ** 2 / rad
    pla = just & (idx >= scene.ns) & (idx < scene.ns + scene.np_)
    n[pla] = scene.p_nor[k[pla] - scene.ns]            # Intersection.hs:64
    tri = just & (idx >= scene.ns + scene.np_)
    if tri.any():
        kt = k[tri] - scene.ns - scene.np_
        n[tri], dn[tri] = scene.tr.nhat[kt], scene.tr.nu[kt]
    return {"idx": idx, "t": tt, "p": p, "n": n, "dp": dp, "dn": dn, "off": off, "decided": decided}


# ---- primary rays -----------------------------------------------------------------------------------------------------------------------------
def primary_rays(camera, w, h):
    """primaryRays (Trace.hs:205-262) with the run-time width and height for 800 and 600 (screenAspect, screenSize: Util.hs:186-200;
    forwardVector, upVector: Util.hs:96-102; screenPixels: Util.hs:209-210) -> (origin (3,), directions (h * w, 3), bound on |d(direction)|).
    The bound: the camera's quaternion (angles are inputs: e_trig = 2 u) and rotate give dcdir; tan of an angle with 3 u relative error,
    amplified by theta (1 + tan^2) / tan and two units of tan's own, gives the relative errors rt of screenDistance and 2 rt + u of
    screenHalfWidth; center = pos + cdir dist rounds by u |center| and centerOffset = center - pos inherits it (a cancellation:
    |pos| may exceed the offset); cross, normalize and the divisions round by a few u each; the point on the virtual plane sums three vectors,
    and rayDir = normalize (point - pos) divides the absolute error by |point - pos| >= screenDistance."""
    cam = np.asarray(camera)
    pos = cam["position"].astype(np.float64).reshape(3)
    rot = cam["rotation"].astype(np.float64).reshape(3)
    fov = float(cam["fov"])
    angle = (fov * np.pi / 180.0) / 2.0
    dist = 1.0 / np.tan(angle)
    half_width = np.tan(angle) * dist
    cdir = rotate(angles_to_quaternion(rot), np.array([0.0, 0.0, -1.0]))            # Util.hs:48-50
    aspect = float(w) / float(h)
    center = pos + cdir * dist
    center_offset = center - pos
    right = normalize(np.cross(center_offset, np.array([0.0, 1.0, 0.0])))[0] / half_width
    top = np.cross(cdir, right) / aspect
    ys, xs = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    sx = xs.reshape(-1) / float(w) * 2.0 + (-1.0)                                    # rasterPos / screenSize * 2 + V2 (-1) 1, screenSize = (W, -H)
    sy = ys.reshape(-1) / float(-h) * 2.0 + 1.0
    point = center[None, :] + right[None, :] * sx[:, None] + top[None, :] * sy[:, None]
    d, close = normalize(point - pos[None, :])
    dcdir = rotation_error(0.0, rot)                                                 # the angles are inputs: no da beyond 2 u |a|
    t = np.tan(angle)
    rt = 3.0 * U * angle * (1.0 + t * t) / t + 3.0 * U
    dcenter = dist * (dcdir + rt) + 2.0 * U * (norm(pos) + dist)                     # of center and of centerOffset
    cross_len = norm(np.cross(center_offset, np.array([0.0, 1.0, 0.0])))
    skip = NORMALIZE_SKIP if abs(1.0 - cross_len ** 2) <= 2.0 * NEAR_ZERO else 0.0
    dright = (norm(right)) * (dcenter / max(cross_len, 1e-300) + 8.0 * U + 2.0 * rt + skip)
    dtop = norm(top) * (dcdir + dright / norm(right) + 6.0 * U)
    dpoint = dcenter + U * norm(center) + (dright + 4.0 * U * norm(right)) * np.abs(sx) + (dtop + 4.0 * U * norm(top)) * np.abs(sy) \
        + 3.0 * U * norm(point)
    ed = (dpoint + U * (norm(point) + norm(pos))) / norm(point - pos[None, :]) + 4.0 * U + np.where(close, NORMALIZE_SKIP, 0.0)
    return pos, d, ed


# ---- materials ---------------------------------------------------------------------------------------------------------------------------------
def _matte_glossy(scene, prim, hit, d, ed, rv):
    """calcNextRay's match (Trace.hs:403-429) for rays that hit `prim` -> (next, dnext, b, db, decided)"""
    n, dn = hit["n"], hit["dn"]
    p = scene.param[prim]
    is_matte = scene.tag[prim] == MATTE
    Nn, Dn = norm(n), norm(d)
    # Matte (Trace.hs:407-412)
    am = np.pi * rv
    next_m = rotate(angles_to_quaternion(am), n)
    dnext_m = rotation_error(np.pi, am) * Nn + dn
    b_m = p / np.pi * dot(next_m, n)
    db_m = (p / np.pi) * (Nn * dnext_m + norm(next_m) * dn + 3.0 * U * norm(next_m) * Nn) + 3.0 * U * np.abs(b_m)
    # Glossy (Trace.hs:419-429)
    a = dot(d, n)
    da = ed * Nn + Dn * dn + 3.0 * U * Dn * Nn
    refl = d - (2.0 * a)[:, None] * n
    drefl = ed + 2.0 * da * Nn + 2.0 * np.abs(a) * dn + 4.0 * U * (Dn + 2.0 * np.abs(a) * Nn)
    ag = (1.0 - p)[:, None] * rv
    next_g = rotate(angles_to_quaternion(ag), refl)
    Rn = norm(refl)
    dnext_g = rotation_error(1.0, ag) * Rn + drefl
    dot_g = dot(next_g, refl)
    ddot_g = Rn * dnext_g + norm(next_g) * drefl + 3.0 * U * norm(next_g) * Rn
    b_g = np.maximum(0.0, dot_g)
    decided = is_matte | (np.abs(dot_g) > SAFETY * ddot_g)
    m = is_matte[:, None]
    return (np.where(m, next_m, next_g), np.where(is_matte, dnext_m, dnext_g), np.where(is_matte, b_m, b_g),
            np.where(is_matte, db_m, ddot_g), decided)


def _glass(scene, prim, hit, d, ed):
    """GLASS, from its prose definition (include/ptmi.h; the formula block above glass_children in oracle/pt_oracle.c):
    dn = d . n, cosi = -dn, eta = 1 / ior, k = 1 - eta^2 (1 - cosi^2); reflection = d - (2 dn) n; r0 = ((1 - ior) / (1 + ior))^2,
    m = 1 - cosi, R = r0 + (1 - r0) m^5; k < 0 (total internal reflection): R = 1 and the refraction is the reflection; else
    refraction = eta d + (eta cosi - sqrt k) n.  Child 0 takes the reflection and R, child 1 the refraction and 1 - R.
    -> (refl, drefl, refr, drefr, R, dR, tir, decided)"""
    n, dn_ = hit["n"], hit["dn"]
    ior = scene.param[prim]
    Nn, Dn = norm(n), norm(d)
    a = dot(d, n)
    da = ed * Nn + Dn * dn_ + 3.0 * U * Dn * Nn
    cosi = -a
    eta = 1.0 / ior
    k = 1.0 - (eta * eta) * (1.0 - cosi * cosi)
    dk = eta * eta * 2.0 * np.abs(cosi) * da + 6.0 * U
    refl = d - (2.0 * a)[:, None] * n
    drefl = ed + 2.0 * da * Nn + 2.0 * np.abs(a) * dn_ + 4.0 * U * (Dn + 2.0 * np.abs(a) * Nn)
    r0 = ((1.0 - ior) / (1.0 + ior)) ** 2
    m = 1.0 - cosi
    R = r0 + (1.0 - r0) * (((m * m) * (m * m)) * m)
    dR = (1.0 - r0) * (5.0 * m ** 4 * (da + U) + 6.0 * U * np.abs(m) ** 5) + 4.0 * U
    tir = k < 0
    with np.errstate(invalid="ignore", divide="ignore"):
        root = np.sqrt(k)
        coef = eta * cosi - root
        refr = eta[:, None] * d + coef[:, None] * n
        drefr = eta * ed + (eta * da + dk / (2.0 * root) + 3.0 * U) * Nn + np.abs(coef) * dn_ + 3.0 * U * norm(refr)
    refr = np.where(tir[:, None], refl, refr)
    drefr = np.where(tir, drefl, drefr)
    R = np.where(tir, 1.0, R)
    dR = np.where(tir, 0.0, dR)
    return refl, drefl, refr, drefr, R, dR, tir, np.abs(k) > SAFETY * dk


# ---- render ------------------------------------------------------------------------------------------------------------------------------------
class _Rays:
    FIELDS = ("pix", "o", "d", "eo", "ed", "S", "dS", "C", "seed", "depth", "first", "prev", "eoff")

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def take(self, mask):
        out = {}
        for f in self.FIELDS:
            v = getattr(self, f)
            out[f] = tuple(x[mask] for x in v) if f == "seed" else v[mask]
        return _Rays(**out)

    @staticmethod
    def concat(parts):
        out = {}
        for f in _Rays.FIELDS:
            if f == "seed":
                out[f] = tuple(np.concatenate([p.seed[i] for p in parts]) for i in range(4))
            else:
                out[f] = np.concatenate([getattr(p, f) for p in parts])
        return _Rays(**out)


def accumulation_bound(n_additions, abs_sum):
    """ACCUMULATION and UNORDERED (module docstring): (n - 1) 2^-24 sum |term| for n added terms, in whatever order"""
    return np.maximum(n_additions - 1, 0)[:, None] * U * abs_sum


STAT_NAMES = ("three_hits", "matte", "glossy", "glass_both", "tir", "sphere", "plane", "triangle", "near_zero_end", "miss_end")


def render(scene, camera, w, h, mode, limit, n_spp, seeds, max_hits=32):
    """`render` (Trace.hs:135-200) applied n_spp times to zero colour and the generator planes `seeds` (four uint32 arrays of h * w).
    mode INLINE: traceInline `limit` (Trace.hs:344-383) -- nearZero or a miss zeroes the throughput, otherwise emittance is added and
      THEN the throughput updated (:381-383); the seed is the one the last live bounce left.
    mode STREAMS_*: the chain of traceSteps (Trace.hs:141-191, :272-331) for a pixel's one ray -- EVERY hit adds (computeResult, :317-321),
      a ray goes on unless nearZero throughput or a miss (numNewRays, :329-331), no bounce limit (`limit` is a cap that must not bind);
      FROM_RESULT: the pixel keeps the seed of its latest result's ray (combine new old), KEEP: its own; updateSeed draws once (:190-191).
    mode TREE: the same with GLASS: a hit gives two children (child 1's seed one draw further), rays at step >= `limit` are not traced
      (the step cap), seeds as KEEP.
    -> dict: colour (n, 3), bound (n, 3), seeds (4 arrays), decided (n), hits (n, n_spp, max_hits; -1 fills; the first ray of a tree),
       stats {name: bool (n)}, n_terms (n), truncated (rays the cap cut)"""
    n_px = w * h
    pos, prim_d, prim_ed = primary_rays(camera, w, h)
    pix_seed = tuple(np.array(s, np.uint32).reshape(-1).copy() for s in seeds)
    colour, err, abs_sum = np.zeros((n_px, 3)), np.zeros((n_px, 3)), np.zeros((n_px, 3))
    n_terms = np.zeros(n_px, np.int64)
    decided = np.ones(n_px, bool)
    hits = np.full((n_px, n_spp, max_hits), -1, np.int32)
    stats = {k: np.zeros(n_px, bool) for k in STAT_NAMES}
    truncated = 0
    c6 = NEAR_ZERO

    def mark(name, pix):
        stats[name][pix] = True

    for s in range(n_spp):
        rays = _Rays(pix=np.arange(n_px), o=np.repeat(pos[None, :], n_px, 0), d=prim_d.copy(), eo=np.zeros(n_px), ed=prim_ed.copy(),
                     S=np.ones(n_px), dS=np.zeros(n_px), C=np.ones((n_px, 3)), seed=tuple(x.copy() for x in pix_seed),
                     depth=np.zeros(n_px, np.int64), first=np.ones(n_px, bool),
                     prev=np.full(n_px, -1), eoff=np.zeros(n_px))   # first: the lineage of child 0s, what `hits` records
        step = 0
        while len(rays.pix) and step < limit:
            hit = check_hit(scene, rays.o, rays.d, rays.eo, rays.ed, rays.prev, rays.eoff)
            just = hit["idx"] >= 0
            thr = rays.C * rays.S[:, None]
            Q = dot(thr, thr)
            dQ = 2.0 * np.abs(rays.S) * rays.dS * dot(rays.C, rays.C) + 4.0 * U * Q
            nz = near_zero(Q)
            nz_decided = np.abs(Q - c6) > SAFETY * dQ
            prim = np.clip(hit["idx"], 0, None)
            # (Inline: `nearZero throughput || isNothing nextHit` -- where nearZero certainly holds the hit decides nothing)
            np.logical_and.at(decided, rays.pix, hit["decided"] | (nz & nz_decided if mode == INLINE else False))
            if mode == INLINE:                                         # prepareRay (Trace.hs:362-366)
                adds = just & ~nz
                alive = adds
                np.logical_and.at(decided, rays.pix, nz_decided)
                mark("near_zero_end", rays.pix[nz])
                mark("miss_end", rays.pix[~nz & ~just])
                dead = ~alive
                for i in range(4):
                    pix_seed[i][rays.pix[dead]] = rays.seed[i][dead]
            else:                                                      # traceStep (Trace.hs:272-294)
                adds = just
                alive = just & ~nz
                np.logical_and.at(decided, rays.pix[just], nz_decided[just])
                mark("near_zero_end", rays.pix[just & nz])
                mark("miss_end", rays.pix[~just])
                if mode == STREAMS_FROM_RESULT:
                    for i in range(4):
                        pix_seed[i][rays.pix[just]] = rays.seed[i][just]
            # computeResult / computeRay: emittance * throughput (Trace.hs:318-321, :377-382)
            E = scene.color[prim] * scene.illuminance[prim][:, None]
            term = E * thr
            dterm = np.abs(E * rays.C) * (rays.dS + 3.0 * U * np.abs(rays.S))[:, None]
            ap = rays.pix[adds]
            np.add.at(colour, ap, term[adds])
            np.add.at(err, ap, dterm[adds])
            np.add.at(abs_sum, ap, np.abs(term[adds]))
            np.add.at(n_terms, ap, 1)
            rec = adds & rays.first
            if step < max_hits:
                hits[rays.pix[rec], s, step] = hit["idx"][rec]
            kind = scene.kind[prim]
            for name, kk in (("sphere", 0), ("plane", 1), ("triangle", 2)):
                mark(name, rays.pix[adds & (kind == kk)])
            mark("three_hits", rays.pix[adds & (rays.depth >= 2)])
            # the next rays (calcNextRay, Trace.hs:394-435; GLASS)
            live = rays.take(alive)
            lh = {k: v[alive] for k, v in hit.items()}
            lprim = prim[alive]
            if not len(live.pix):
                rays = live
                step += 1
                continue
            rv, seed2 = gen_vec(live.seed)                             # drawn before the match on the BRDF (Trace.hs:402)
            tag = scene.tag[lprim]
            glass = tag == GLASS
            assert mode == TREE or not glass.any(), "GLASS needs the ray tree"
            nxt, dnext, b, db, dec = _matte_glossy(scene, lprim, lh, live.d, live.ed, rv)
            np.logical_and.at(decided, live.pix[~glass], dec[~glass])
            mark("matte", live.pix[tag == MATTE])
            mark("glossy", live.pix[tag == GLOSSY])
            prob = 1.0 / (np.pi * 2.0)
            f = b * prob
            df = db * prob + 3.0 * U * np.abs(f)
            col = scene.color[lprim]

            def child(direction, ddir, f, df, seed):
                Sn = live.S * f
                o2 = lh["p"] + direction * EPSILON                      # Trace.hs:431
                eo2 = lh["dp"] + EPSILON * ddir + U * (norm(lh["p"]) + 2.0 * EPSILON * norm(direction))
                return _Rays(pix=live.pix, o=o2, d=direction, eo=eo2, ed=ddir, S=Sn,
                             dS=np.abs(f) * live.dS + np.abs(live.S) * df + 3.0 * U * np.abs(Sn), C=live.C * col, seed=seed,
                             depth=live.depth + 1, first=live.first, prev=lprim,
                             eoff=lh["off"] + EPSILON * ddir + U * (norm(lh["p"]) + 2.0 * EPSILON * norm(direction)))
            kids = child(nxt, dnext, f, df, seed2)
            if glass.any():
                refl, drefl, refr, drefr, R, dR, tir, gdec = _glass(scene, lprim, lh, live.d, live.ed)
                np.logical_and.at(decided, live.pix[glass], gdec[glass])
                mark("tir", live.pix[glass & tir])
                g = glass
                k0 = child(refl, drefl, R, dR + U, seed2).take(g)
                _, seed3 = random_float(seed2)                          # child 1: the seed advanced one more draw
                k1 = child(refr, drefr, 1.0 - R, dR + 2.0 * U, seed3).take(g)
                k1.first = np.zeros(len(k1.pix), bool)
                rays = _Rays.concat([kids.take(~g), k0, k1])
                n_plain = int((~g).sum())
                n_g = int(g.sum())
                # a split whose two children both hit something: looked up after the next step
                if n_g and step + 1 < limit:
                    h2 = check_hit(scene, rays.o[n_plain:], rays.d[n_plain:], rays.eo[n_plain:], rays.ed[n_plain:])["idx"] >= 0
                    mark("glass_both", k0.pix[h2[:n_g] & h2[n_g:]])
            else:
                rays = kids
            step += 1
        truncated += len(rays.pix)
        if mode == INLINE:
            for i in range(4):                                         # survivors of all `limit` iterations carry their seed out
                pix_seed[i][rays.pix] = rays.seed[i]
        else:
            _, pix_seed = random_float(pix_seed)                        # updateSeed (Trace.hs:151, :190-191)
            pix_seed = tuple(x.copy() for x in pix_seed)
    n_add = n_terms + (n_spp if mode == INLINE else 0)
    bound = SAFETY * (err + accumulation_bound(n_add, abs_sum))
    return {"colour": colour, "bound": bound, "seeds": pix_seed, "decided": decided, "hits": hits, "stats": stats,
            "n_terms": n_terms, "truncated": truncated}


def counter_moves_allowed(mode, limit, n_spp, before, after):
    """Whether the generator's counter moved by a count the algorithm allows (what is asserted of an undecided pixel): Inline draws three
    per live bounce, at most `limit` a sample; Streams KEEP (and the tree) one per sample; FROM_RESULT 3 k + 1 per sample"""
    moved = (np.asarray(after, np.uint32).reshape(-1) - np.asarray(before, np.uint32).reshape(-1)).astype(np.int64)
    if mode == INLINE:
        return (moved % 3 == 0) & (moved <= 3 * limit * n_spp)
    if mode == STREAMS_FROM_RESULT:
        return (moved >= n_spp) & ((moved - n_spp) % 3 == 0)
    return moved == n_spp
