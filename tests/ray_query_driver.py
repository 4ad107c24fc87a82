"""Child program of tests/test_gpu_ray_query.py (not a test module): `python tests/ray_query_driver.py WORKDIR`.

ptmi_trace_rays_device and ptmi_occluded_device through Context.trace_rays / Context.occluded, as a PyTorch caller uses them: device
tensors in, device tensors out, on the context's stream, in a process where torch brings the HIP runtime up before the library is loaded
(bench.py's order).  The scenes, their rays and the references -- ptmi_eval_check_hit and the oracle's fold with the index kept
(tests/cxx/bvh_traverse.c, mesh_traverse.c) -- are made once and shared by the cases.  One line per case, `ok <case>` or
`FAILED <case>: <why>`; a failed comparison does not end the process, a runtime error does; the last line is RAY_QUERY_DONE."""
import ctypes as C
import os
import subprocess
import sys
import traceback

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)
from t_max_families import T_MAX_OF_HITS, T_MAX_OF_MISSES, t_max_for  # noqa: E402

CASES = ["1 closest hit", "2 sizes alignment guards", "3 hit record", "4 occluded", "5 caller stream", "6 after device updates", "7 refusals",
         "8 render after queries", "9 non-finite scene data"]
KINDS = ["plain", "s16", "runs", "bvh", "mesh"]      # linear without runs, the bench scene (runs), a made run, a sphere hierarchy, a mesh scene
N_RAYS = 4096
SIZES = (0, 1, 63, 64, 65, 257, N_RAYS)
GUARD = 64                                            # words on either side of every output
SENTINEL = 0x7FC0DEAD

torch = pkg = B = W = ora = None
bvh_rays = mesh_rays = None
blib = mlib = rlib = None
SCENES = {}


def setup(workdir):
    global torch, pkg, B, W, ora, bvh_rays, mesh_rays, blib, mlib, rlib
    import torch as _torch
    torch = _torch
    torch.zeros(1, device="cuda")                      # torch brings the runtime up first
    torch.cuda.synchronize()
    import __graft_entry__ as graft
    pkg = graft.load_package()
    pkg._build.build_lib()
    ora = graft.load_oracle()
    ora.build()
    B, W = pkg.binding, pkg.world
    import bvh_rays as _b
    import mesh_rays as _m
    bvh_rays, mesh_rays = _b, _m
    blib, mlib = bvh_rays.traverse_lib(workdir), mesh_rays.traverse_lib(workdir)
    out = os.path.join(workdir, "libray_query_reference.so")
    cmd = ["gcc", "-O2", "-std=c11", "-fPIC", "-shared", "-ffp-contract=off", "-fno-fast-math", "-fno-math-errno", "-Wall", "-Werror",
           os.path.join(HERE, "cxx", "ray_query_reference.c"), "-o", out, ora.LIB, "-Wl,-rpath," + os.path.dirname(ora.LIB), "-lm"]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    rlib = C.CDLL(out)
    rlib.ray_query_sphere_records.restype = None


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda")


def host(t):
    return t.cpu().numpy()


def bits(a):
    return np.asarray(a).view(np.uint32)


def trace(c, rays, **kw):
    """Context.trace_rays on the context's OWN stream from torch's: the header's ordering rule, with host waits -- torch's writes to the
    inputs are complete before the call, and the outputs are read behind the context's stream"""
    torch.cuda.synchronize()
    out = c.trace_rays(rays, **kw)
    c.synchronize()
    return out


def occluded(c, rays, t_max, **kw):
    torch.cuda.synchronize()
    out = c.occluded(rays, t_max, **kw)
    c.synchronize()
    return out


def same_words(a, b):
    """bit for bit, a NaN for a NaN (IEEE 754 leaves its payload open: host and device choose differently) -> the rows that differ"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    nan = np.isnan(b)
    bad = (np.isnan(a) != nan) | ((bits(a) != bits(b)) & ~nan)
    return np.flatnonzero(bad.reshape(len(a), -1).any(1))


class Scene:
    """One scene kind: what to set, its rays, ptmi_eval_check_hit's answer and the oracle's fold"""

    def __init__(self, kind):
        self.kind, self.triangles = kind, None
        if kind == "plain":
            self.spheres, self.planes = W.main_scene()
        elif kind == "s16":
            self.spheres, self.planes = W.scene16()
        elif kind == "runs":
            from test_gpu_shared_xy import row_scene
            self.spheres, self.planes = row_scene(pkg, 9, 2, 4)
        elif kind == "bvh":
            self.spheres, self.planes = bvh_rays.adversarial_scene(3000)
        elif kind in ("nonfinite linear", "nonfinite bvh"):
            self.spheres, self.planes = bvh_rays.adversarial_scene(300, seed=5)
        else:
            self.spheres, self.triangles, self.planes = mesh_rays.adversarial_scene(0)
            assert len(self.spheres) == 8
        if kind == "mesh":                            # the triangles' families, and the spheres' for what the hierarchies do not serve
            rays = np.concatenate([mesh_rays.adversarial_rays(self.triangles, N_RAYS - 1024, seed=3), bvh_rays.adversarial_rays(self.spheres, 1024, seed=3)])
        else:
            rays = bvh_rays.adversarial_rays(self.spheres, N_RAYS, seed=3)
        self.rays = np.ascontiguousarray(rays, np.float32)
        if kind.startswith("nonfinite"):             # (after the rays, which are aimed at the finite scene)
            bad = np.concatenate([self.planes[:1]] * 3)
            bad["direction"][0] = (np.nan, 1.0, 0.0)
            bad["position"][1] = (0.0, np.inf, 0.0)
            bad["direction"][2] = (0.0, 0.0, 0.0)     # 0 / 0 for every ray through its position's plane, +-inf elsewhere
            self.planes = np.concatenate([bad, self.planes])
            if kind == "nonfinite linear":
                self.spheres = self.spheres.copy()
                self.spheres["position"][7, 0] = np.nan
                self.spheres["radius"][11] = np.inf
                self.spheres["position"][13] = (3e38, -3e38, 3e38)
        # (a seed's draw may hold no non-finite ray: four stand at the end of every set)
        self.rays[-4:] = [[np.nan, 0, 0, 0, 1, 0], [1, 0, -5, 0, np.inf, 0], [np.inf, 1, 2, 0, 0, -1], [1, 0, -5, 0, 0, 0]]
        assert self.rays.shape == (N_RAYS, 6)
        d2 = (self.rays[:, 3:].astype(np.float64) ** 2).sum(1)
        far = np.abs(self.rays[:, :3]).max(1) > 2.0 ** 40
        # the families that force the full search: non-finite rays, |d|^2 off 1 by more than 2^-12, origins beyond 2^40
        assert (~np.isfinite(self.rays).all(1)).sum() > 0 and (np.abs(d2 - 1.0) > 2.0 ** -12).sum() > 50 and far.sum() > 0, kind
        xy = np.ascontiguousarray(self.spheres["position"][:, :2]).view(np.uint32)
        shares = any(np.array_equal(xy[i], xy[i - 1]) for i in range(1, len(xy)))
        assert shares == (kind in ("s16", "runs")) or kind.startswith("nonfinite"), kind      # which linear kernel the launcher takes
        if kind == "mesh":
            self.fold = mesh_rays.linear_fold(mlib, self.spheres, self.triangles, self.planes, self.rays)
        else:
            self.fold = bvh_rays.linear_fold(blib, self.spheres, self.planes, self.rays)
        self.d_rays = dev(self.rays)
        torch.cuda.synchronize()
        self.ctx = pkg.Context(0)
        self.set(self.ctx)
        self.eval = self.ctx.eval_check_hit(self.rays)
        self.t, self.idx = self.eval[0], self.eval[1]

    def set(self, c):
        if self.kind == "mesh":
            c.set_scene_mesh(self.spheres, self.triangles, self.planes)
        elif self.kind in ("bvh", "nonfinite bvh"):
            c.set_scene_bvh(self.spheres, self.planes)
        else:
            c.set_scene(self.spheres, self.planes)


# ---- the cases ---------------------------------------------------------------------------------------------------------------------

def case_closest_hit():
    """1: t and idx are ptmi_eval_check_hit's bit for bit, idx >= 0 where just is set, and both are the oracle's fold"""
    def same_hits(got, want, what):
        # t as numbers: against the oracle two encodings differ where the value cannot -- a NaN key, and the -0 of a ray that starts on a
        # sphere where the oracle's min(t0, t1) is +0 (tests/test_gpu_bvh.py: same_hits)
        (t0, i0, j0), (t1, i1, j1) = got, want
        bad = np.flatnonzero(~((t0 == t1) | (np.isnan(t0) & np.isnan(t1))) | (i0 != i1) | (j0 != j1))
        assert bad.size == 0, "%s: %d rays differ, e.g. ray %d: device (%r, %d) oracle (%r, %d)" % (what, bad.size, bad[0], t0[bad[0]], i0[bad[0]], t1[bad[0]], i1[bad[0]])

    for kind in KINDS:
        sc = SCENES[kind]
        t, idx = (host(x) for x in trace(sc.ctx, sc.d_rays))
        e_t, e_idx, e_just = sc.eval
        assert np.array_equal(bits(t), bits(e_t)), "%s: t differs from ptmi_eval_check_hit in %d rays" % (kind, (bits(t) != bits(e_t)).sum())
        assert np.array_equal(idx, e_idx), "%s: idx differs from ptmi_eval_check_hit" % kind
        assert np.array_equal(idx >= 0, e_just == 1), "%s: idx >= 0 is not just" % kind
        same_hits((t, idx, (idx >= 0).astype(np.int32)), sc.fold, "%s against the oracle's fold" % kind)
        assert (idx >= 0).sum() >= 400 and (idx < 0).sum() >= 15, (kind, int((idx >= 0).sum()))     # (the mesh scene is a closed room: few rays miss)
    mesh = SCENES["mesh"]
    first = len(mesh.spheres) + len(mesh.planes)
    assert (mesh.idx >= first).sum() > 200 and ((mesh.idx >= 0) & (mesh.idx < len(mesh.spheres))).sum() > 20     # triangles and spheres are hit


def guarded(n, words, dtype, misalign):
    """n x words elements between two guards -> (the whole buffer, the view); misalign: the view starts 4 bytes off an 8-byte boundary"""
    buf = torch.full((2 * GUARD + n * words + 2,), SENTINEL, dtype=torch.int32, device="cuda")
    assert buf.data_ptr() % 8 == 0
    start = GUARD + (1 if misalign else 0)
    view = buf[start:start + n * words].view(dtype)
    assert n == 0 or view.data_ptr() % 8 == (4 if misalign else 0)
    return buf, (view.view(n, words) if words > 1 else view), start


def guards_intact(buf, start, length, what):
    h = host(buf).view(np.uint32)
    assert (h[:start] == SENTINEL).all() and (h[start + length:] == SENTINEL).all(), "%s: a guard word was written" % what


def case_sizes():
    """2: wave and block tails, rays and hit records on both alignments, outputs between guard words"""
    for kind in KINDS:
        sc = SCENES[kind]
        t_max, want_occ, _ = t_max_for(sc)
        full_hit = host(trace(sc.ctx, sc.d_rays, hit=True)[2])
        for n in SIZES:
            for misalign in (False, True):
                what = "%s, n = %d, %s" % (kind, n, "4 bytes off" if misalign else "8-byte aligned")
                rbuf, rays, _ = guarded(n, 6, torch.float32, misalign)
                rays.copy_(sc.d_rays[:n])
                mbuf, tm, _ = guarded(n, 1, torch.float32, misalign)
                tm.copy_(dev(t_max[:n]))
                outs = [guarded(n, 1, torch.float32, misalign), guarded(n, 1, torch.int32, not misalign), guarded(n, 6, torch.float32, misalign),
                        guarded(n, 1, torch.int32, misalign)]
                torch.cuda.synchronize()
                sc.ctx.trace_rays(rays, out=(outs[0][1], outs[1][1], outs[2][1]))
                sc.ctx.occluded(rays, tm, out=outs[3][1])
                sc.ctx.synchronize()
                for (buf, view, start), words in zip(outs, (1, 1, 6, 1)):
                    guards_intact(buf, start, n * words, what)
                assert np.array_equal(bits(host(outs[0][1])), bits(sc.t[:n])), what + ": t"
                assert np.array_equal(host(outs[1][1]), sc.idx[:n]), what + ": idx"
                assert np.array_equal(bits(host(outs[2][1])), bits(full_hit[:n])), what + ": hit record"
                assert np.array_equal(host(outs[3][1]), want_occ[:n]), what + ": occluded"


def case_hit_record():
    """3: position o + d * t, every f32 operation rounded on its own; sphere normals by ora_hit_sphere, plane normals the stored direction,
    triangle normals the unit normal of mesh_rays.records (its columns 9 to 11: v0, v1, v2, n); six zeros for a miss.  Bit for bit (same_words: a NaN for a NaN -- a non-finite
    ray that the fold calls a hit)."""
    for kind in KINDS:
        sc = SCENES[kind]
        t, idx, hit = (host(x) for x in trace(sc.ctx, sc.d_rays, hit=True))
        assert np.array_equal(bits(t), bits(sc.t)) and np.array_equal(idx, sc.idx)
        ns, np_ = len(sc.spheres), len(sc.planes)
        want = np.zeros((N_RAYS, 6), np.float32)
        o, d = sc.rays[:, :3], sc.rays[:, 3:]
        just = idx >= 0
        with np.errstate(all="ignore"):
            pos = (o + (d * t[:, None]).astype(np.float32)).astype(np.float32)
        want[just, :3] = pos[just]
        s = np.ascontiguousarray(sc.spheres, ora.SPHERE_DTYPE)
        by_oracle = np.zeros((N_RAYS, 6), np.float32)
        P = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
        rlib.ray_query_sphere_records(P(s), len(s), P(sc.rays), P(np.ascontiguousarray(t)), P(np.ascontiguousarray(idx)), N_RAYS, P(by_oracle))
        on_sphere = just & (idx < ns)
        assert same_words(by_oracle[on_sphere, :3], want[on_sphere, :3]).size == 0, "%s: the oracle's hit position is not o + d * t" % kind
        want[on_sphere, 3:] = by_oracle[on_sphere, 3:]
        on_plane = just & (idx >= ns) & (idx < ns + np_)
        want[on_plane, 3:] = sc.planes["direction"][idx[on_plane] - ns]
        if kind == "mesh":
            on_triangle = idx >= ns + np_
            rec = mesh_rays.records(mlib, sc.triangles)
            want[on_triangle, 3:] = rec[idx[on_triangle] - ns - np_][:, 9:12]
            assert on_triangle.sum() > 200
        assert on_sphere.sum() > 20 and on_plane.sum() > 20 and (~just).sum() >= 15, kind
        assert np.isnan(want).any(1).sum() < 64, (kind, int(np.isnan(want).any(1).sum()))
        bad = same_words(hit, want)
        assert bad.size == 0, "%s: %d hit records differ, e.g. ray %d (primitive %d): %r, expected %r" % (kind, bad.size, bad[0], idx[bad[0]], hit[bad[0]], want[bad[0]])


def case_occluded():
    """4: the specification, computed on the host from the closest hit, with every family of t_max present in every scene kind"""
    for kind in KINDS:
        sc = SCENES[kind]
        t_max, want, family = t_max_for(sc)
        hit = sc.idx >= 0
        for name in T_MAX_OF_HITS:
            assert (family[hit] == name).sum() >= 20, (kind, name)
        for name in T_MAX_OF_MISSES:
            assert (family[~hit] == name).sum() >= 5, (kind, name)
        assert want[hit].sum() >= 100 and (want[hit] == 0).sum() >= 100 and want[~hit].sum() == 0, kind
        got = host(occluded(sc.ctx, sc.d_rays, dev(t_max)))
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, "%s: %d rays differ, e.g. ray %d (t_max %s = %r, closest hit t %r, primitive %d): %d" % (
            kind, bad.size, bad[0], family[bad[0]], t_max[bad[0]], sc.t[bad[0]], sc.idx[bad[0]], got[bad[0]])


def case_caller_stream():
    """5: on torch's non-default stream through set_stream; the inputs are written on that stream behind a filler that outlasts the host's
    calls, the results are read after that stream alone is synchronised, and there is no ptmi_synchronize in between"""
    stream = torch.cuda.Stream()
    filler = torch.ones((2048, 2048), device="cuda")
    for kind in ("s16", "bvh", "mesh"):
        sc = SCENES[kind]
        t_max, want, _ = t_max_for(sc)
        d_t_max = dev(t_max)
        rays = torch.zeros_like(sc.d_rays)
        tm = torch.zeros_like(d_t_max)
        torch.cuda.synchronize()
        sc.ctx.set_stream(stream.cuda_stream)
        try:
            with torch.cuda.stream(stream):
                x = filler
                for _ in range(20):
                    x = x @ filler * 1e-3
                rays.copy_(sc.d_rays)
                tm.copy_(d_t_max)
                t, idx, hit = sc.ctx.trace_rays(rays, hit=True)
                occ = sc.ctx.occluded(rays, tm)
            stream.synchronize()
            assert np.array_equal(bits(host(t)), bits(sc.t)) and np.array_equal(host(idx), sc.idx), "%s: closest hit on the caller's stream" % kind
            assert np.array_equal(host(occ), want), "%s: occluded on the caller's stream" % kind
            assert float(x.sum()) == float(x.sum())
        finally:
            torch.cuda.synchronize()
            sc.ctx.set_stream(None)


def case_after_updates():
    """6: after update_spheres and after set_mesh_triangles from device tensors, a query enqueued at once answers for the new scene"""
    sc = SCENES["bvh"]
    g = W.displaced_spheres(W.sphere_geometry(sc.spheres), 0.5, "wave", seed=2)
    moved = W.with_sphere_geometry(sc.spheres, g)
    t_max, _, _ = t_max_for(sc)
    d_t_max, d_g = dev(t_max), dev(np.ascontiguousarray(g, np.float32))
    torch.cuda.synchronize()
    with pkg.Context(0) as c, pkg.Context(0) as fresh:
        c.set_scene_bvh(sc.spheres, sc.planes)
        c.update_spheres(d_g)
        got = list(c.trace_rays(sc.d_rays, hit=True)) + [c.occluded(sc.d_rays, d_t_max)]      # at once: ordered behind the update by the stream alone
        c.synchronize()
        got = [host(x) for x in got]
        fresh.set_scene_bvh(moved, sc.planes)
        want = [host(x) for x in trace(fresh, sc.d_rays, hit=True)] + [host(occluded(fresh, sc.d_rays, d_t_max))]
        for a, b, name in zip(got, want, ("t", "idx", "hit", "occluded")):
            assert np.array_equal(bits(a), bits(b)), "after update_spheres: %s" % name
        assert not np.array_equal(bits(got[0]), bits(sc.t)), "the update moved nothing"
        e = fresh.eval_check_hit(sc.rays)
        assert np.array_equal(bits(got[0]), bits(e[0])) and np.array_equal(got[1], e[1])
    sc = SCENES["mesh"]
    t2 = mesh_rays.adversarial_scene(1, seed=4)[1]
    d_t2 = dev(np.ascontiguousarray(t2).view(np.float32).reshape(-1, 15).copy())
    d_t_max = dev(t_max_for(sc)[0])
    torch.cuda.synchronize()
    with pkg.Context(0) as c, pkg.Context(0) as fresh:
        sc.set(c)
        c.set_mesh_triangles(d_t2)
        got = list(c.trace_rays(sc.d_rays, hit=True)) + [c.occluded(sc.d_rays, d_t_max)]      # at once: ordered behind the update by the stream alone
        c.synchronize()
        got = [host(x) for x in got]
        fresh.set_scene_mesh(sc.spheres, t2, sc.planes)
        want = [host(x) for x in trace(fresh, sc.d_rays, hit=True)] + [host(occluded(fresh, sc.d_rays, d_t_max))]
        for a, b, name in zip(got, want, ("t", "idx", "hit", "occluded")):
            assert np.array_equal(bits(a), bits(b)), "after set_mesh_triangles: %s" % name
        assert not np.array_equal(got[1], sc.idx), "the new triangles changed nothing"


def case_refusals():
    """7: PTMI_ESTATE before a scene, PTMI_EINVAL for NULL with n > 0 and for a negative n, through the raw library handle; nothing is written"""
    sc = SCENES["bvh"]
    n = 65
    bufs = [guarded(n, 1, torch.float32, False), guarded(n, 1, torch.int32, False), guarded(n, 6, torch.float32, False), guarded(n, 1, torch.int32, False)]
    d_t_max = dev(np.ones(n, np.float32))
    torch.cuda.synchronize()
    vp = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    rays, (t, idx, hit, occ) = vp(sc.d_rays), [vp(b[1]) for b in bufs]

    def untouched(what):
        torch.cuda.synchronize()
        for buf, _, _ in bufs:
            assert (host(buf).view(np.uint32) == SENTINEL).all(), "%s wrote to an output" % what

    with pkg.Context(0) as c:
        lib, h = c._lib, c._h
        assert lib.ptmi_trace_rays_device(h, rays, n, t, idx, hit) == B.PTMI_ESTATE
        assert lib.ptmi_occluded_device(h, rays, vp(d_t_max), n, occ) == B.PTMI_ESTATE
        untouched("a query before any scene")
        sc.set(c)
        for rc in (lib.ptmi_trace_rays_device(h, None, n, t, idx, hit), lib.ptmi_trace_rays_device(h, rays, n, None, idx, hit),
                   lib.ptmi_trace_rays_device(h, rays, n, t, None, hit), lib.ptmi_trace_rays_device(h, rays, -1, t, idx, hit),
                   lib.ptmi_occluded_device(h, None, vp(d_t_max), n, occ), lib.ptmi_occluded_device(h, rays, None, n, occ),
                   lib.ptmi_occluded_device(h, rays, vp(d_t_max), n, None), lib.ptmi_occluded_device(h, rays, vp(d_t_max), -5, occ)):
            assert rc == B.PTMI_EINVAL, rc
        assert b"ray-query" in lib.ptmi_last_error(h)
        assert lib.ptmi_trace_rays_device(h, None, 0, None, None, None) == B.PTMI_OK
        assert lib.ptmi_occluded_device(h, None, None, 0, None) == B.PTMI_OK
        c.synchronize()
        untouched("a refused query")
        assert lib.ptmi_trace_rays_device(h, rays, n, t, idx, None) == B.PTMI_OK            # hit may be NULL: t and idx alone are written
        c.synchronize()
        assert np.array_equal(bits(host(bufs[0][1])), bits(sc.t[:n])) and np.array_equal(host(bufs[1][1]), sc.idx[:n])
        assert (host(bufs[2][0]).view(np.uint32) == SENTINEL).all()


def case_render_after_queries():
    """8: a render after interleaved queries equals, on all seven planes, a render without them (64 x 48, one BVH and one mesh scene)"""
    from conftest import assert_planes_equal
    cam = W.initial_camera()
    for kind in ("bvh", "mesh"):
        sc = SCENES[kind]
        d_t_max = dev(t_max_for(sc)[0])
        torch.cuda.synchronize()
        with pkg.Context(0) as c:
            sc.set(c)
            c.resize(64, 48)
            planes, keep = [], []
            for queries in (False, True):
                c.init_output(0x5EED1234)
                for algorithm in (pkg.INLINE, pkg.STREAMS):
                    if queries:
                        keep.append(c.trace_rays(sc.d_rays, hit=True))      # (kept until the stream has passed the call)
                    c.render(cam, 4, 2, algorithm)
                    if queries:
                        keep.append(c.occluded(sc.d_rays, d_t_max))
                planes.append(c.download_state())
            assert_planes_equal(planes[1], planes[0], "%s: a render between queries" % kind)
            assert np.any(np.asarray(planes[0][0]) != 0.0)


def case_nonfinite_scene_data():
    """9: scene data that is not finite -- a linear scene's spheres (a NaN centre, an infinite radius, a centre at 3e38) and, for a linear
    and a BVH scene, planes with a NaN normal, an infinite position and a zero normal in front of the finite ones: the keys that send
    check_hit and check_hit_bvh to the literal fold, or that the literal fold forgets its accumulator over, send the any-hit walk to the full
    search, and the answers are still the specification's"""
    for kind in ("nonfinite linear", "nonfinite bvh"):
        sc = Scene(kind)
        try:
            t, idx = (host(x) for x in trace(sc.ctx, sc.d_rays))
            assert np.array_equal(bits(t), bits(sc.t)) and np.array_equal(idx, sc.idx), "%s: closest hit differs from ptmi_eval_check_hit" % kind
            # the zero normal's key is a NaN for every ray: the fold forgets what came before it, so no closest hit is a sphere although
            # spheres are in the way -- an any-hit walk that trusted its first occluder would answer 1 where the specification says 0
            assert (idx >= 0).sum() >= 400 and ((idx >= 0) & (idx < len(sc.spheres))).sum() == 0, kind
            t_max, want, family = t_max_for(sc)
            assert want.sum() >= 100 and (want == 0).sum() >= 100, kind
            got = host(occluded(sc.ctx, sc.d_rays, dev(t_max)))
            bad = np.flatnonzero(got != want)
            assert bad.size == 0, "%s: %d rays differ, e.g. ray %d (t_max %s = %r, closest hit t %r, primitive %d): %d" % (
                kind, bad.size, bad[0], family[bad[0]], t_max[bad[0]], sc.t[bad[0]], sc.idx[bad[0]], got[bad[0]])
        finally:
            sc.ctx.close()


RUN = dict(zip(CASES, (case_closest_hit, case_sizes, case_hit_record, case_occluded, case_caller_stream, case_after_updates, case_refusals,
                       case_render_after_queries, case_nonfinite_scene_data)))


def main():
    setup(sys.argv[1])
    for kind in KINDS:
        SCENES[kind] = Scene(kind)
    for name in CASES:
        try:
            RUN[name]()
            print("ok %s" % name, flush=True)
        except AssertionError as e:
            print("FAILED %s: %s" % (name, str(e).replace("\n", " ")[:1500] or traceback.format_exc()[-1500:].replace("\n", " | ")), flush=True)
        except B.PtmiError as e:                     # a runtime error: nothing more is started on the device
            print("FAILED %s: %s" % (name, e), flush=True)
            raise SystemExit(3)
    for sc in SCENES.values():
        sc.ctx.close()
    print("RAY_QUERY_DONE", flush=True)


if __name__ == "__main__":
    main()
