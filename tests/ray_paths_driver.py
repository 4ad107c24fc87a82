"""Child program of tests/test_gpu_ray_paths.py (not a test module): `python tests/ray_paths_driver.py WORKDIR`.

ptmi_path_seeds_device, ptmi_trace_paths_device and ptmi_trace_paths_indexed_device through Context.path_seeds / Context.trace_paths, as a
PyTorch caller uses them: device tensors in, colour and seeds updated in place, on the context's stream, in a process where torch brings
the HIP runtime up before the library is loaded (bench.py's order).  The scenes, their 4 096 rays and the reference -- the oracle's
traceInline in the loop of ora_render_inline_ex (tests/cxx/ray_paths_reference.c) -- are tests/ray_paths_inputs.py's; a reference is
computed once per (scene, limit, spp, start) and shared by the cases.  One line per case, `ok <case>` or `FAILED <case>: <why>`; a failed
comparison does not end the process, a runtime error does; the last line is RAY_PATHS_DONE."""
import ctypes as C
import os
import sys
import traceback

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)
import ray_query_driver as Q  # noqa: E402
from ray_query_driver import SENTINEL, bits, dev, guarded, guards_intact, host, same_words  # noqa: E402

CASES = ["1 colour and seed against the reference", "2 sizes alignment guards", "3 a camera's rays equal a render", "4 sample split and accumulation",
         "5 indexed", "6 degenerate arguments", "7 ordering and isolation", "8 refusals"]
LIMITS, SPPS = (1, 3, 8), (1, 2)
SIZES = (0, 1, 63, 64, 65, 257)
INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1

torch = pkg = B = W = inputs = ref = None
KINDS, N_RAYS, SEED0 = [], 0, 0
SCENES = {}
_REFS = {}


def setup(workdir):
    global torch, pkg, B, W, inputs, ref, KINDS, N_RAYS, SEED0
    import torch as _torch
    torch = Q.torch = _torch
    torch.zeros(1, device="cuda")                      # torch brings the runtime up first
    torch.cuda.synchronize()
    import __graft_entry__ as graft
    pkg = graft.load_package()
    pkg._build.build_lib()
    B, W = pkg.binding, pkg.world
    import ray_paths_inputs as _inputs
    inputs = _inputs
    KINDS, N_RAYS, SEED0 = inputs.KINDS, inputs.N_RAYS, inputs.SEED0
    ref = inputs.Reference(workdir)


class Scene:
    def __init__(self, kind):
        self.kind = kind
        self.data = inputs.scene(kind)
        self.spheres, self.triangles, self.planes = self.data
        self.rays = inputs.batch(kind, self.data, ref)
        self.d_rays = dev(self.rays)
        torch.cuda.synchronize()
        self.ctx = pkg.Context(0)
        self.set(self.ctx)

    def set(self, c, spheres=None, triangles=None):
        s = self.spheres if spheres is None else spheres
        if self.kind == "mesh":
            c.set_scene_mesh(s, self.triangles if triangles is None else triangles, self.planes)
        elif self.kind == "bvh":
            c.set_scene_bvh(s, self.planes)
        else:
            c.set_scene(s, self.planes)


def start_colour(tag):
    """A start colour by name: zeros, or seeded values with -0.0, a NaN and an infinity among them"""
    if tag == "zero":
        return np.zeros((N_RAYS, 3), np.float32)
    c = np.random.default_rng(17).normal(size=(N_RAYS, 3)).astype(np.float32)
    c[5], c[6, 1], c[7, 2] = -0.0, np.nan, np.inf
    return c


def reference(kind, limit, spp, start="zero", data=None):
    """(colour, seeds) of the reference after spp samples from `start` and genSeeds(SEED0), computed once"""
    key = (kind, limit, spp, start) if data is None else None
    if key is None or key not in _REFS:
        got = ref.trace(SCENES[kind].data if data is None else data, SCENES[kind].rays, start_colour(start), ref.seeds(N_RAYS), limit, spp)[:2]
        if key is None:
            return got
        _REFS[key] = got
    return _REFS[key]


def d_seeds(n=None):
    return dev(ref.seeds(N_RAYS)[:n].view(np.int32))


def run(c, rays, seeds, limit, spp, color, index=None):
    """Context.trace_paths on the context's OWN stream from torch's, with host waits on either side (the header's ordering rule)"""
    if color is None:                                  # (torch's zeros are through before the context's stream starts)
        color = torch.zeros((int(rays.shape[0]), 3), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    out = c.trace_paths(rays, seeds, limit, spp=spp, color=color, index=index)
    c.synchronize()
    assert out is color
    return out


def compare(color, seeds, want, what, rows=None):
    w_color, w_seeds = want
    g_color, g_seeds = host(color).reshape(-1, 3), host(seeds).view(np.uint32).reshape(-1, 4)
    if rows is not None:
        g_color, g_seeds, w_color, w_seeds = g_color[rows], g_seeds[rows], w_color[rows], w_seeds[rows]
    bad = np.flatnonzero((g_seeds != w_seeds).any(1))
    assert bad.size == 0, "%s: %d seeds differ, e.g. ray %d: %r, the reference has %r" % (what, bad.size, bad[0], g_seeds[bad[0]], w_seeds[bad[0]])
    bad = same_words(g_color, w_color)
    assert bad.size == 0, "%s: %d colours differ, e.g. ray %d: %r, the reference has %r" % (what, bad.size, bad[0], g_color[bad[0]], w_color[bad[0]])


# ---- the cases ---------------------------------------------------------------------------------------------------------------------

def case_reference():
    """1: colour and seed are the reference's word for word (a NaN for a NaN), every scene kind, limits 1, 3, 8, 1 and 2 spp"""
    for kind in KINDS:
        sc = SCENES[kind]
        for limit in LIMITS:
            for spp in SPPS:
                seeds = d_seeds()
                color = run(sc.ctx, sc.d_rays, seeds, limit, spp, None)
                assert tuple(color.shape) == (N_RAYS, 3) and color.dtype == torch.float32
                compare(color, seeds, reference(kind, limit, spp), "%s, limit %d, %d spp" % (kind, limit, spp))
        c8 = reference(kind, 8, 2)[0]
        assert (np.nan_to_num(c8, nan=1.0) != 0).any(1).sum() >= N_RAYS // 10, kind


def case_sizes():
    """2: wave and block tails; rays, colour and seeds 16-byte aligned and 4 bytes off; guard words around colour and seed"""
    for kind in KINDS:
        sc = SCENES[kind]
        want = reference(kind, 3, 2, "mixed")
        for n in SIZES:
            for misalign in (False, True):
                what = "%s, n = %d, %s" % (kind, n, "4 bytes off" if misalign else "aligned")
                rbuf, rays, _ = guarded(n, 6, torch.float32, misalign)
                cbuf, color, cstart = guarded(n, 3, torch.float32, misalign)
                sbuf, seeds, sstart = guarded(n, 4, torch.int32, misalign)
                assert n == 0 or seeds.data_ptr() % 16 == (4 if misalign else 0)
                if n:
                    rays.copy_(sc.d_rays[:n])
                    color.copy_(dev(start_colour("mixed")[:n]))
                    seeds.copy_(d_seeds(n))
                got = run(sc.ctx, rays, seeds, 3, 2, color)
                assert got is color
                guards_intact(cbuf, cstart, 3 * n, what + ": colour")
                guards_intact(sbuf, sstart, 4 * n, what + ": seeds")
                if n:
                    compare(color, seeds, (want[0][:n], want[1][:n]), what)


def case_camera():
    """3: the oracle's primary rays of a 67 x 45 image, path_seeds' seeds, a zero colour, limit 8, 3 spp == init_output + render(INLINE, 8, 3)
    on all seven planes, bit for bit; path_seeds with a first index == ora_gen_seeds"""
    w, h, cam = 67, 45, W.initial_camera()
    n = w * h
    rays = dev(ref.primaries(cam, w, h))
    for kind in KINDS:
        sc = SCENES[kind]
        torch.cuda.synchronize()
        with pkg.Context(0) as c:
            sc.set(c)
            seeds = c.path_seeds(SEED0, n)
            c.synchronize()
            assert tuple(seeds.shape) == (n, 4) and np.array_equal(host(seeds).view(np.uint32), ref.seeds(n)), "%s: path_seeds" % kind
            color = run(c, rays, seeds, 8, 3, None)
            c.resize(w, h)
            c.init_output(SEED0)
            c.render(cam, 8, 3, pkg.INLINE)
            planes = c.download_state()
        g_color, g_seeds = host(color), host(seeds).view(np.uint32)
        for k, name in enumerate("rgb"):
            assert np.array_equal(bits(g_color[:, k]), bits(np.asarray(planes[k], np.float32).reshape(-1))), "%s: plane %s" % (kind, name)
        for k, name in enumerate(("sa", "sb", "sc", "sctr")):
            assert np.array_equal(g_seeds[:, k], np.asarray(planes[3 + k]).view(np.uint32).reshape(-1)), "%s: plane %s" % (kind, name)
        assert np.any(g_color != 0)
    c = SCENES["main"].ctx
    for count, first, misalign in ((257, 1000, True), (64, 2 ** 40 + 3, False), (1, 7, False), (0, 5, False)):
        buf, out, start = guarded(count, 4, torch.int32, misalign)
        torch.cuda.synchronize()
        assert c.path_seeds(SEED0 + 1, count, first_index=first, out=out) is out
        c.synchronize()
        guards_intact(buf, start, 4 * count, "path_seeds, n = %d" % count)
        assert np.array_equal(host(out).view(np.uint32).reshape(-1, 4), ref.seeds(count, SEED0 + 1, first)), "path_seeds from index %d" % first


def case_split():
    """4: one call of 3 spp == three calls of 1 spp == the reference; accumulation into a colour that is not zero == the reference started from it"""
    for kind in KINDS:
        sc = SCENES[kind]
        for start in ("zero", "mixed"):
            want = reference(kind, 8, 3, start)
            seeds, color = d_seeds(), dev(start_colour(start))
            run(sc.ctx, sc.d_rays, seeds, 8, 3, color)
            compare(color, seeds, want, "%s, 3 spp in one call from a %s colour" % (kind, start))
            seeds, color = d_seeds(), dev(start_colour(start))
            for _ in range(3):
                run(sc.ctx, sc.d_rays, seeds, 8, 1, color)
            compare(color, seeds, want, "%s, three calls of 1 spp from a %s colour" % (kind, start))


def case_indexed():
    """5: through ray_order's permutation the plain call's words; through an active list (m < n, entries outside [0, n) among them) the named
    rays alone are updated, the rest and the guards are as they were"""
    rng = np.random.default_rng(21)
    for kind in KINDS:
        sc = SCENES[kind]
        want = reference(kind, 8, 2, "mixed")
        work = torch.empty(B.ray_order_bytes(N_RAYS), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        order = sc.ctx.ray_order(sc.d_rays, work=work)
        sc.ctx.synchronize()
        assert np.array_equal(np.sort(host(order)), np.arange(N_RAYS)), kind
        for what, index in (("the device order", order), ("its reverse", torch.flip(order, (0,)).contiguous())):
            seeds, color = d_seeds(), dev(start_colour("mixed"))
            run(sc.ctx, sc.d_rays, seeds, 8, 2, color, index=index)
            compare(color, seeds, want, "%s through %s" % (kind, what))
        for m in (1, 63, 65, 257, 1500):
            for misalign in (False, True):
                what = "%s, an active list of %d, %s" % (kind, m, "4 bytes off" if misalign else "aligned")
                picks = rng.permutation(N_RAYS)[:m].astype(np.int64)            # every ray at most once
                if m >= 63:
                    picks[[1, 17, 40, 62]] = [-1, N_RAYS, INT32_MIN, INT32_MAX]
                named = picks[(picks >= 0) & (picks < N_RAYS)]
                ibuf, d_index, istart = guarded(m, 1, torch.int32, misalign)
                d_index.copy_(dev(picks.astype(np.int32)))
                cbuf, color, cstart = guarded(N_RAYS, 3, torch.float32, misalign)
                sbuf, seeds, sstart = guarded(N_RAYS, 4, torch.int32, misalign)
                color.copy_(dev(start_colour("mixed")))
                seeds.copy_(d_seeds())
                run(sc.ctx, sc.d_rays, seeds, 8, 2, color, index=d_index)
                guards_intact(cbuf, cstart, 3 * N_RAYS, what + ": colour")
                guards_intact(sbuf, sstart, 4 * N_RAYS, what + ": seeds")
                guards_intact(ibuf, istart, m, what + ": the index")
                assert np.array_equal(host(d_index), picks.astype(np.int32)), what + ": the index was written"
                rest = np.setdiff1d(np.arange(N_RAYS), named)
                compare(color, seeds, want, what + ", the named rays", rows=named)
                compare(color, seeds, (start_colour("mixed"), ref.seeds(N_RAYS)), what + ", the rays no entry names", rows=rest)
        for bad in (-1, N_RAYS, INT32_MIN, INT32_MAX):                           # nothing but an entry outside [0, n)
            seeds, color = d_seeds(), dev(start_colour("mixed"))
            run(sc.ctx, sc.d_rays, seeds, 8, 2, color, index=dev(np.array([bad], np.int32)))
            compare(color, seeds, (start_colour("mixed"), ref.seeds(N_RAYS)), "%s, the index [%d]" % (kind, bad))
        seeds, color = d_seeds(), dev(start_colour("mixed"))                      # m == 0
        run(sc.ctx, sc.d_rays, seeds, 8, 2, color, index=torch.zeros(0, dtype=torch.int32, device="cuda"))
        compare(color, seeds, (start_colour("mixed"), ref.seeds(N_RAYS)), "%s, an empty index" % kind)


def case_degenerate():
    """6: bounce_limit 0 and -1 give colour = 0 + colour (a -0.0 becomes +0.0) and leave the seed; n_spp 0 and -1 touch nothing"""
    start, seeds0 = start_colour("mixed"), ref.seeds(N_RAYS)
    with np.errstate(all="ignore"):
        added = (np.float32(0.0) + start).astype(np.float32)
    assert bits(added)[5, 0] == 0 and bits(start)[5, 0] == 0x80000000
    for kind in KINDS:
        sc = SCENES[kind]
        for limit in (0, -1):
            for spp in (1, 2):
                seeds, color = d_seeds(), dev(start)
                run(sc.ctx, sc.d_rays, seeds, limit, spp, color)
                compare(color, seeds, (added, seeds0), "%s, limit %d, %d spp" % (kind, limit, spp))
                compare(color, seeds, reference(kind, limit, spp, "mixed"), "%s, limit %d, %d spp, the reference" % (kind, limit, spp))
                assert np.array_equal(bits(host(color)[5]), np.zeros(3, np.uint32))
        for spp in (0, -1):
            seeds, color = d_seeds(), dev(start)
            run(sc.ctx, sc.d_rays, seeds, 8, spp, color)
            assert np.array_equal(bits(host(color)), bits(start)) and np.array_equal(host(seeds).view(np.uint32), seeds0), "%s, %d spp" % (kind, spp)


def case_ordering():
    """7: on torch's non-default stream through set_stream, read after that stream alone is synchronised; after update_spheres /
    set_mesh_triangles from device tensors the results are a fresh context's; a render before and after the calls equals one without them"""
    from conftest import assert_planes_equal
    stream = torch.cuda.Stream()
    filler = torch.ones((2048, 2048), device="cuda")
    for kind in ("s16", "big", "bvh", "mesh"):
        sc = SCENES[kind]
        want = reference(kind, 8, 2)
        seeds0 = d_seeds()
        rays, seeds = torch.zeros_like(sc.d_rays), torch.zeros_like(seeds0)
        torch.cuda.synchronize()
        sc.ctx.set_stream(stream.cuda_stream)
        try:
            with torch.cuda.stream(stream):
                x = filler
                for _ in range(20):
                    x = x @ filler * 1e-3
                rays.copy_(sc.d_rays)
                seeds.copy_(seeds0)
                color = sc.ctx.trace_paths(rays, seeds, 8, spp=1)          # (colour allocated and zeroed by torch on this stream)
                sc.ctx.trace_paths(rays, seeds, 8, spp=1, color=color)
            stream.synchronize()
            compare(color, seeds, want, "%s on the caller's stream" % kind)
            assert float(x.sum()) == float(x.sum())
        finally:
            torch.cuda.synchronize()
            sc.ctx.set_stream(None)
    # after device updates, at once: ordered behind the update by the stream alone
    sc = SCENES["bvh"]
    g = W.displaced_spheres(W.sphere_geometry(sc.spheres), 0.5, "wave", seed=2)
    moved = W.with_sphere_geometry(sc.spheres, g)
    d_g = dev(np.ascontiguousarray(g, np.float32))
    seeds, color = d_seeds(), dev(start_colour("zero"))
    torch.cuda.synchronize()
    with pkg.Context(0) as c, pkg.Context(0) as fresh:
        sc.set(c)
        c.update_spheres(d_g)
        c.trace_paths(sc.d_rays, seeds, 8, spp=2, color=color)
        c.synchronize()
        sc.set(fresh, spheres=moved)
        f_seeds, f_color = d_seeds(), dev(start_colour("zero"))
        run(fresh, sc.d_rays, f_seeds, 8, 2, f_color)
        compare(color, seeds, (host(f_color), host(f_seeds).view(np.uint32)), "after update_spheres, against a context set afresh")
        compare(color, seeds, reference("bvh", 8, 2, data=(moved, None, sc.planes)), "after update_spheres, against the reference")
        assert not np.array_equal(bits(host(color)), bits(reference("bvh", 8, 2)[0])), "the update moved nothing"
    sc = SCENES["mesh"]
    import mesh_rays
    t2 = mesh_rays.adversarial_scene(1, seed=4)[1]
    d_t2 = dev(np.ascontiguousarray(t2).view(np.float32).reshape(-1, 15).copy())
    seeds, color = d_seeds(), dev(start_colour("zero"))
    torch.cuda.synchronize()
    with pkg.Context(0) as c, pkg.Context(0) as fresh:
        sc.set(c)
        c.set_mesh_triangles(d_t2)
        c.trace_paths(sc.d_rays, seeds, 8, spp=2, color=color)
        c.synchronize()
        sc.set(fresh, triangles=t2)
        f_seeds, f_color = d_seeds(), dev(start_colour("zero"))
        run(fresh, sc.d_rays, f_seeds, 8, 2, f_color)
        compare(color, seeds, (host(f_color), host(f_seeds).view(np.uint32)), "after set_mesh_triangles, against a context set afresh")
        assert not np.array_equal(bits(host(color)), bits(reference("mesh", 8, 2)[0])), "the new triangles changed nothing"
    # a render between the calls
    cam = W.initial_camera()
    for kind in ("s16", "bvh", "mesh"):
        sc = SCENES[kind]
        seeds, color = d_seeds(), dev(start_colour("zero"))
        torch.cuda.synchronize()
        with pkg.Context(0) as c:
            sc.set(c)
            c.resize(64, 48)
            planes = []
            for calls in (False, True):
                c.init_output(SEED0)
                if calls:
                    c.trace_paths(sc.d_rays, seeds, 8, spp=1, color=color)
                c.render(cam, 4, 2, pkg.INLINE)
                if calls:
                    before = c.stats()
                    c.trace_paths(sc.d_rays, seeds, 8, spp=1, color=color)
                    c.synchronize()
                    after = c.stats()
                    assert (after["live_bounces"], after["samples"]) == (before["live_bounces"], before["samples"]), "%s: a path call moved the statistics" % kind
                c.render(cam, 4, 1, pkg.STREAMS)
                planes.append(c.download_state())
            assert_planes_equal(planes[1], planes[0], "%s: renders around path calls" % kind)
            assert np.any(np.asarray(planes[0][0]) != 0.0)
            c.synchronize()
            compare(color, seeds, reference(kind, 8, 2), "%s: path calls around renders" % kind)


def case_refusals():
    """8: through the raw library handle -- PTMI_ESTATE before a scene (the path entries; the seeds need none), PTMI_EINVAL for a negative n
    or m, for NULL pointers with a positive count and for a scene with a GLASS sphere; nothing is written"""
    sc = SCENES["bvh"]
    n, m = 65, 40
    cbuf, color, _ = guarded(n, 3, torch.float32, False)
    sbuf, seeds, _ = guarded(n, 4, torch.int32, False)
    d_index = dev(np.arange(m, dtype=np.int32))
    torch.cuda.synchronize()
    vp = lambda x: C.c_void_p(x.data_ptr())  # noqa: E731
    rays, col, sd, index = vp(sc.d_rays), vp(color), vp(seeds), vp(d_index)

    def untouched(what):
        torch.cuda.synchronize()
        for buf in (cbuf, sbuf):
            assert (host(buf).view(np.uint32) == SENTINEL).all(), "%s wrote to an output" % what

    with pkg.Context(0) as c:
        lib, h = c._lib, c._h
        P, X, S = lib.ptmi_trace_paths_device, lib.ptmi_trace_paths_indexed_device, lib.ptmi_path_seeds_device
        assert P(h, rays, n, 8, 1, col, sd) == B.PTMI_ESTATE and X(h, rays, n, index, m, 8, 1, col, sd) == B.PTMI_ESTATE
        untouched("a path call before any scene")
        for rc in (S(h, SEED0, 0, -1, sd), S(h, SEED0, 0, n, None)):
            assert rc == B.PTMI_EINVAL, rc
        assert S(h, SEED0, 0, 0, None) == B.PTMI_OK
        c.synchronize()
        untouched("a refused path_seeds")
        sc.set(c)
        for rc in (P(h, None, n, 8, 1, col, sd), P(h, rays, n, 8, 1, None, sd), P(h, rays, n, 8, 1, col, None), P(h, rays, -1, 8, 1, col, sd),
                   X(h, None, n, index, m, 8, 1, col, sd), X(h, rays, n, index, m, 8, 1, None, sd), X(h, rays, n, index, m, 8, 1, col, None),
                   X(h, rays, -1, index, m, 8, 1, col, sd), X(h, rays, n, index, -1, 8, 1, col, sd), X(h, rays, n, None, m, 8, 1, col, sd)):
            assert rc == B.PTMI_EINVAL, rc
        assert b"ray-path" in lib.ptmi_last_error(h)
        assert P(h, None, 0, 8, 1, None, None) == B.PTMI_OK and P(h, rays, n, 8, 0, col, sd) == B.PTMI_OK
        assert X(h, rays, n, None, 0, 8, 1, col, sd) == B.PTMI_OK and X(h, None, 0, index, m, 8, 1, None, None) == B.PTMI_OK
        c.synchronize()
        untouched("a refused or empty path call")
        glass = sc.spheres[:40].copy()
        glass["brdf_tag"][3], glass["brdf_param"][3] = W.GLASS, 1.5
        c.set_scene(glass, sc.planes)
        assert P(h, rays, n, 8, 1, col, sd) == B.PTMI_EINVAL and b"GLASS" in lib.ptmi_last_error(h)
        assert X(h, rays, n, index, m, 8, 1, col, sd) == B.PTMI_EINVAL and b"GLASS" in lib.ptmi_last_error(h)
        assert S(h, SEED0, 0, n, sd) == B.PTMI_OK                                  # the seeds ask nothing of the scene
        c.synchronize()
        assert (host(cbuf).view(np.uint32) == SENTINEL).all(), "a path call on a GLASS scene wrote to the colour"
        assert np.array_equal(host(seeds).view(np.uint32), ref.seeds(n))


RUN = dict(zip(CASES, (case_reference, case_sizes, case_camera, case_split, case_indexed, case_degenerate, case_ordering, case_refusals)))


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
    print("RAY_PATHS_DONE", flush=True)


if __name__ == "__main__":
    main()
