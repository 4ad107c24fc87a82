"""Child program of tests/test_gpu_ray_bounce.py (not a test module): `python tests/ray_bounce_driver.py WORKDIR`.

ptmi_bounce_rays_device, ptmi_bounce_rays_indexed_device and ptmi_live_rays_device through Context.bounce_rays / Context.live_rays, as a
PyTorch caller uses them: device tensors in, the state changed in place, on the context's stream, in a process where torch brings the HIP
runtime up before the library is loaded (bench.py's order).  The scenes, their 4 096 rays and the seeds are tests/ray_paths_inputs.py's;
the step's reference -- one prepareRay over the oracle's functions (tests/cxx/ray_bounce_reference.c) -- and the live list's definition are
tests/ray_bounce_inputs.py's.  The reference's eight steps are computed once per scene and shared by the cases.  Every comparison is word
for word, a NaN for a NaN.  One line per case, `ok <case>` or `FAILED <case>: <why>`; a failed comparison does not end the process, a
runtime error does; the last line is RAY_BOUNCE_DONE."""
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
import ray_paths_driver as P  # noqa: E402
from ray_query_driver import SENTINEL, bits, dev, guarded, guards_intact, host, same_words  # noqa: E402

CASES = ["1 eight steps against the reference", "2 k steps equal trace_paths", "3 sizes alignment guards optional outputs", "4 the wavefront loop",
         "5 live_rays alone", "6 indexed step", "7 ordering and isolation", "8 refusals"]
SIZES = (0, 1, 63, 64, 65, 257)
LIVE_COUNTS = (1, 64, 65, 4097, 65537, 2 ** 22 - 1, 2 ** 22)
INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1
STEPS = 8

torch = pkg = B = W = inputs = ref = None
KINDS, N_RAYS = [], 0
SCENES = {}
_STEPS = {}
DEVICE_STATES = {}                                  # kind -> [(radiance, seeds) on the host after step 1 .. 8]: case 1's, for case 2


def setup(workdir):
    global torch, pkg, B, W, inputs, ref, KINDS, N_RAYS
    P.setup(workdir)
    torch, pkg, B, W = P.torch, P.pkg, P.B, P.W
    import ray_bounce_inputs as _inputs
    inputs = _inputs
    ref = P.ref = inputs.Reference(workdir)
    KINDS, N_RAYS = inputs.KINDS, inputs.N_RAYS


def reference_steps(kind, data=None):
    """the reference's states after 1 .. 8 steps from (1, 0, genSeeds), computed once per scene: [(rays, throughput, radiance, seeds, outcome, hit)]"""
    if data is not None:
        return ref.steps(data, SCENES[kind].rays)
    if kind not in _STEPS:
        _STEPS[kind] = ref.steps(SCENES[kind].data, SCENES[kind].rays)
    return _STEPS[kind]


def start_state(kind, after=0):
    """(rays, throughput, radiance, seeds) on the host: the start, or the reference's state after `after` steps"""
    if after == 0:
        return (SCENES[kind].rays, np.ones((N_RAYS, 3), np.float32), np.zeros((N_RAYS, 3), np.float32), ref.seeds(N_RAYS))
    return reference_steps(kind)[after - 1][:4]


def device_state(state, n=None):
    r, t, rad, s = state
    return [dev(np.array(r[:n], np.float32)), dev(np.array(t[:n], np.float32)), dev(np.array(rad[:n], np.float32)), dev(np.array(s[:n]).view(np.int32))]


def step(c, st, index=None, **kw):
    """Context.bounce_rays on the context's OWN stream from torch's, with host waits on either side (the header's ordering rule)"""
    torch.cuda.synchronize()
    out = c.bounce_rays(st[0], st[3], st[1], st[2], index=index, **kw)
    c.synchronize()
    return out


def compare_state(st, want, what, rows=None):
    names = ("rays", "throughput", "radiance")
    for k, name in enumerate(names):
        g, w = host(st[k]), np.asarray(want[k], np.float32)
        if rows is not None:
            g, w = g[rows], w[rows]
        bad = same_words(g, w) if len(g) else np.zeros(0, int)
        assert bad.size == 0, "%s: %d %s differ, e.g. row %d: %r, the reference has %r" % (what, bad.size, name, bad[0], g[bad[0]], w[bad[0]])
    g, w = host(st[3]).view(np.uint32).reshape(-1, 4), np.asarray(want[3]).view(np.uint32).reshape(-1, 4)
    if rows is not None:
        g, w = g[rows], w[rows]
    bad = np.flatnonzero((g != w).any(1))
    assert bad.size == 0, "%s: %d seeds differ, e.g. row %d: %r, the reference has %r" % (what, bad.size, bad[0], g[bad[0]], w[bad[0]])


def compare_outputs(outs, want_t, want_idx, want_hit, what, rows=None):
    for got, want, name in zip(outs, (want_t, want_idx, want_hit), ("t", "idx", "hit")):
        if got is None:
            continue
        g, w = host(got), np.asarray(want)
        if rows is not None:
            g, w = g[rows], w[rows]
        bad = np.flatnonzero(g != w) if name == "idx" else (same_words(g, w) if len(g) else np.zeros(0, int))
        assert bad.size == 0, "%s: %d %s differ, e.g. row %d: %r, expected %r" % (what, bad.size, name, bad[0], g[bad[0]], w[bad[0]])


def incoming_hits(kind, after):
    """(t, idx, hit) of Context.trace_rays on the reference's rays after `after` steps, the miss record where the reference did not trace"""
    sc = SCENES[kind]
    rays = dev(np.array(start_state(kind, after)[0], np.float32))
    torch.cuda.synchronize()
    traced = sc.ctx.trace_rays(rays, hit=True)
    sc.ctx.synchronize()
    t, idx, hit = (host(x).copy() for x in traced)
    frozen = reference_steps(kind)[after][4] == inputs.FROZEN
    t[frozen], idx[frozen], hit[frozen] = 0.0, -1, 0.0
    return t, idx, hit


# ---- the cases ---------------------------------------------------------------------------------------------------------------------

def case_reference():
    """1: per scene, 8 steps from (1, 0): rays, throughput, radiance and seeds are the reference's after every step; hit is the position and
    normal checkHit gave the reference, idx >= 0 exactly where the reference shaded; t, idx and hit are Context.trace_rays' on the incoming
    rays where the ray was traced and the miss record where it was frozen"""
    for kind in KINDS:
        sc = SCENES[kind]
        want = reference_steps(kind)
        st = device_state(start_state(kind))
        DEVICE_STATES[kind] = []
        for k in range(STEPS):
            what = "%s, step %d" % (kind, k + 1)
            incoming = st[0].clone()
            frozen_in = inputs.near_zero(host(st[1]))
            torch.cuda.synchronize()
            traced = sc.ctx.trace_rays(incoming, hit=True)
            sc.ctx.synchronize()
            q_t, q_idx, q_hit = (host(x).copy() for x in traced)
            outs = step(sc.ctx, st, hit=True)
            assert len(outs) == 3 and tuple(outs[2].shape) == (N_RAYS, 6)
            compare_state(st, want[k], what)
            outcome, rec = want[k][4], want[k][5]
            assert np.array_equal(frozen_in, outcome == inputs.FROZEN), what
            q_t[frozen_in], q_idx[frozen_in], q_hit[frozen_in] = 0.0, -1, 0.0
            compare_outputs(outs, q_t, q_idx, q_hit, what + ", against trace_rays on the incoming rays")
            assert np.array_equal(host(outs[1]) >= 0, outcome == inputs.HIT), what + ": idx >= 0 where the reference shaded"
            bad = same_words(host(outs[2]), rec)
            assert bad.size == 0, "%s: %d hit records differ from the reference's, e.g. ray %d" % (what, bad.size, bad[0])
            DEVICE_STATES[kind].append((host(st[2]).copy(), host(st[3]).copy()))
        assert not bits(host(st[1])).any(), "%s: a throughput is not zero after 8 steps" % kind


def case_trace_paths():
    """2: after k steps, 0 + radiance and the seeds are Context.trace_paths(limit k, 1 spp) from a zero colour and the same seeds: k = 1, 3, 8"""
    for kind in KINDS:
        sc = SCENES[kind]
        if len(DEVICE_STATES.get(kind, ())) != STEPS:  # (case 1 did not get there)
            st = device_state(start_state(kind))
            DEVICE_STATES[kind] = []
            for _ in range(STEPS):
                step(sc.ctx, st)
                DEVICE_STATES[kind].append((host(st[2]).copy(), host(st[3]).copy()))
        for k in (1, 3, 8):
            seeds = P.d_seeds()
            color = P.run(sc.ctx, sc.d_rays, seeds, k, 1, None)
            radiance, s = DEVICE_STATES[kind][k - 1]
            with np.errstate(all="ignore"):
                added = (np.float32(0.0) + radiance).astype(np.float32)
            P.compare(color, seeds, (added, s.view(np.uint32)), "%s, %d steps against trace_paths" % (kind, k))
            assert np.any(added != 0)


OUTPUT_SETS = ((True, True, True), (True, False, False), (False, True, False), (False, False, True), (False, False, False))


def case_sizes():
    """3: n = 0, 1, 63, 64, 65, 257; every array aligned and 4 bytes off; guard words around every in/out and output array; the optional
    outputs all, singly and none.  One step from the reference's state after two, reordered so that hits, misses and frozen rays are
    among the first 63"""
    for kind in KINDS:
        sc = SCENES[kind]
        w_t, w_idx, w_hit = incoming_hits(kind, 2)
        # the rays in an order that puts twenty of each outcome first, so that the short batches hold hits, misses and frozen rays
        outcome = reference_steps(kind)[2][4]
        first = np.stack([np.flatnonzero(outcome == o)[:20] for o in (inputs.HIT, inputs.MISSED, inputs.FROZEN)], 1).reshape(-1)
        rows = np.concatenate([first, np.setdiff1d(np.arange(N_RAYS), first)])
        assert len(set(outcome[rows][:63].tolist())) == 3, kind
        start, want = [x[rows] for x in start_state(kind, 2)], [x[rows] for x in reference_steps(kind)[2]]
        w_t, w_idx, w_hit = w_t[rows], w_idx[rows], w_hit[rows]
        for n in SIZES:
            for misalign in (False, True):
                for which in OUTPUT_SETS:
                    what = "%s, n = %d, %s, outputs %r" % (kind, n, "4 bytes off" if misalign else "aligned", which)
                    bufs = [guarded(n, words, dtype, misalign) for words, dtype in ((6, torch.float32), (3, torch.float32), (3, torch.float32), (4, torch.int32))]
                    st = [b[1] for b in bufs]
                    assert n == 0 or st[3].data_ptr() % 16 == (4 if misalign else 0)
                    for view, src in zip(st, device_state(start, n)):
                        if n:
                            view.copy_(src)
                    obufs = [guarded(n, words, dtype, misalign) for words, dtype in ((1, torch.float32), (1, torch.int32), (6, torch.float32))]
                    out = tuple(b[1] if use else None for b, use in zip(obufs, which))
                    got = step(sc.ctx, st, out=out if any(which) else None)
                    assert (got is None) if not any(which) else all(g is o for g, o in zip(got, out))
                    for (buf, _, at), words, name in zip(bufs, (6, 3, 3, 4), ("rays", "throughput", "radiance", "seeds")):
                        guards_intact(buf, at, words * n, what + ": " + name)
                    for (buf, _, at), words, use, name in zip(obufs, (1, 1, 6), which, ("t", "idx", "hit")):
                        guards_intact(buf, at, words * n if use else 0, what + ": " + name)
                    if n:
                        compare_state(st, [w[:n] for w in want[:4]], what)
                        compare_outputs(out, w_t[:n], w_idx[:n], w_hit[:n], what)


def wavefront_throughput(kind, lists):
    """what the loop leaves in the throughputs: a ray's is the reference's after the last step it was on the list for"""
    t = np.ones((N_RAYS, 3), np.float32)
    for k, named in enumerate(lists):
        t[named] = reference_steps(kind)[k][1][named]
    return t


def case_wavefront():
    """4: step, then live_rays in place, the list padded and never read by the host while the loop runs -- on torch's stream, which orders
    the snapshots taken for this check.  The final rays, radiance and seeds are case 1's; the list after each step is the host twin's of
    the list before it, count its length; the list is empty by step 8; the same through ray_order's permutation, whose order is kept"""
    stream = torch.cuda.Stream()
    for kind in KINDS:
        sc = SCENES[kind]
        want = reference_steps(kind)
        for ordered in (False, True):
            what = "%s, %s" % (kind, "from ray_order's permutation" if ordered else "from every ray")
            st = device_state(start_state(kind))
            live = torch.empty(N_RAYS, dtype=torch.int32, device="cuda")
            count = torch.full((STEPS,), -7, dtype=torch.int32, device="cuda")
            work = torch.empty(B.live_rays_bytes(N_RAYS), dtype=torch.uint8, device="cuda")
            owork = torch.empty(B.ray_order_bytes(N_RAYS), dtype=torch.uint8, device="cuda")
            snaps, thr_snaps = [], []
            torch.cuda.synchronize()
            sc.ctx.set_stream(stream.cuda_stream)
            try:
                with torch.cuda.stream(stream):
                    index = None
                    if ordered:
                        sc.ctx.ray_order(st[0], out=live, work=owork)
                        index = live
                        first = live.clone()
                    for k in range(STEPS):
                        assert sc.ctx.bounce_rays(st[0], st[3], st[1], st[2], index=index) is None
                        thr_snaps.append(st[1].clone())
                        assert sc.ctx.live_rays(st[1], index=index, out=live, count=count[k:k + 1], work=work) is live
                        index = live
                        snaps.append(live.clone())
                stream.synchronize()
            finally:
                torch.cuda.synchronize()
                sc.ctx.set_stream(None)
            before = host(first) if ordered else np.arange(N_RAYS, dtype=np.int32)
            if ordered:
                assert np.array_equal(np.sort(before), np.arange(N_RAYS)), what
            lists, counts = [], host(count)
            for k in range(STEPS):
                lists.append(before[before >= 0])
                w_live, w_count = B.live_rays(host(thr_snaps[k]), before)
                got = host(snaps[k])
                assert np.array_equal(got, w_live), "%s: the list after step %d is not the host twin's" % (what, k + 1)
                assert counts[k] == w_count == (got >= 0).sum() and (got[w_count:] == -1).all(), "%s: count after step %d" % (what, k + 1)
                # the order within the list is the candidates': the first list filtered, nothing moved
                alive = ~inputs.near_zero(host(thr_snaps[k]))
                order0 = host(first) if ordered else np.arange(N_RAYS, dtype=np.int32)
                assert np.array_equal(got[:w_count], order0[alive[order0]]), "%s: the order after step %d" % (what, k + 1)
                assert w_count == (want[k][4] == inputs.HIT).sum() - (inputs.near_zero(want[k][1]) & (want[k][4] == inputs.HIT)).sum(), what
                before = got
            assert counts[STEPS - 1] == 0 and (host(snaps[-1]) == -1).all(), "%s: the list is not empty by step 8" % what
            assert counts[0] > N_RAYS // 4 and counts[2] > 0
            final = list(want[STEPS - 1][:4])
            final[1] = wavefront_throughput(kind, lists)
            compare_state(st, final, what + ", the final state")
            assert inputs.near_zero(host(st[1])).all()


def case_live_rays():
    """5: live_rays alone against torch.nonzero on torch-made throughputs: candidate counts 1, 64, 65, 4 097, 65 537, 2^22 - 1 and 2^22 (every
    level of the scan), all live, none live and alternating; guard words around the list, the count and behind the workspace; an index
    with out-of-range entries, in place; one past PTMI_LIVE_RAYS_MAX refused with nothing written"""
    c = SCENES["main"].ctx
    with pkg.Context(0) as bare:                       # no scene is needed
        for n in LIVE_COUNTS:
            need = B.live_rays_bytes(n)
            ramp = torch.arange(n, device="cuda", dtype=torch.int32)
            for pattern in ("all", "none", "alternating", "thirds"):
                what = "%d candidates, %s" % (n, pattern)
                alive = {"all": ramp >= 0, "none": ramp < 0, "alternating": ramp % 2 == 1, "thirds": (ramp * 7 % 3 == 0) | (ramp // 300 % 2 == 0)}[pattern]
                thr = torch.zeros((n, 3), dtype=torch.float32, device="cuda")
                thr[:, n % 3] = alive.to(torch.float32) * 0.5
                want = torch.full((n,), -1, dtype=torch.int32, device="cuda")
                found = torch.nonzero(alive).flatten().to(torch.int32)
                want[:found.numel()] = found
                obuf, out, ostart = guarded(n, 1, torch.int32, n % 2 == 1)
                cbuf, cnt, cstart = guarded(1, 1, torch.int32, False)
                work = torch.full((need + 64,), 0xA5, dtype=torch.uint8, device="cuda")
                torch.cuda.synchronize()
                assert bare.live_rays(thr, out=out, count=cnt, work=work[:need]) is out
                bare.synchronize()
                assert torch.equal(out, want), what
                assert int(cnt.item()) == found.numel(), what
                guards_intact(obuf, ostart, n, what + ": the list")
                guards_intact(cbuf, cstart, 1, what + ": the count")
                assert bool((work[need:] == 0xA5).all()), what + ": a byte behind the workspace was written"
        # through an index with entries outside [0, n), repeated ones among them, in place and not
        n, m = 4097, 65537
        rng = np.random.default_rng(8)
        index = rng.integers(-5, n + 5, m).astype(np.int32)
        index[[0, 1, 2, 3]] = [INT32_MIN, INT32_MAX, -1, n]
        thr = (torch.rand((n, 3), device="cuda") * 0.5 + 0.5) * (torch.arange(n, device="cuda") % 3 != 0).to(torch.float32)[:, None]
        d_index = dev(index)
        valid = (d_index >= 0) & (d_index < n)
        alive = valid & ((thr * thr).sum(1) > 1e-3)[d_index.clamp(0, n - 1).long()]
        assert bool((((thr * thr).sum(1) > 1e-3) | ((thr * thr).sum(1) == 0)).all())          # (nothing near the threshold: torch's sum decides as nearZero does)
        want = torch.full((m,), -1, dtype=torch.int32, device="cuda")
        want[:int(alive.sum())] = d_index[alive]
        torch.cuda.synchronize()
        out = c.live_rays(thr, index=d_index)
        c.synchronize()
        assert torch.equal(out, want) and np.array_equal(host(d_index), index), "through an index"
        assert np.array_equal(host(out), B.live_rays(host(thr), index)[0])
        ibuf, own, istart = guarded(m, 1, torch.int32, True)
        own.copy_(d_index)
        cnt = torch.zeros(1, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        assert c.live_rays(thr, index=own, out=own, count=cnt) is own
        c.synchronize()
        assert torch.equal(own, want) and int(cnt.item()) == int(alive.sum()), "in place"
        guards_intact(ibuf, istart, m, "in place")
        # one past the limit: refused, nothing written
        over = B.LIVE_RAYS_MAX + 1
        thr = torch.ones((over, 3), dtype=torch.float32, device="cuda")
        obuf, out, ostart = guarded(over, 1, torch.int32, False)
        cbuf, cnt, cstart = guarded(1, 1, torch.int32, False)
        work = torch.full((B.live_rays_bytes(B.LIVE_RAYS_MAX) + 4096,), 0xA5, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        vp = lambda x: C.c_void_p(x.data_ptr())  # noqa: E731
        f = bare._lib.ptmi_live_rays_device
        assert f(bare._h, vp(thr), over, None, 0, vp(out), vp(cnt), vp(work), int(work.numel())) == B.PTMI_ELIMIT
        assert f(bare._h, vp(thr), 5, vp(out), over, vp(out), vp(cnt), vp(work), int(work.numel())) == B.PTMI_ELIMIT
        bare.synchronize()
        assert bool((obuf == SENTINEL).all()) and bool((cbuf == SENTINEL).all()) and bool((work == 0xA5).all()), "a refused live_rays wrote"


def case_indexed():
    """6: through an index only the named rays change -- state and outputs -- and entries outside [0, n) touch nothing; outputs allocated by
    the wrapper hold the miss record at the other positions"""
    rng = np.random.default_rng(21)
    for kind in KINDS:
        sc = SCENES[kind]
        start, want = start_state(kind, 2), reference_steps(kind)[2]
        w_t, w_idx, w_hit = incoming_hits(kind, 2)
        for m in (1, 63, 65, 257, 1500):
            for misalign in (False, True):
                what = "%s, an index of %d, %s" % (kind, m, "4 bytes off" if misalign else "aligned")
                picks = rng.permutation(N_RAYS)[:m].astype(np.int64)            # every ray at most once
                if m >= 63:
                    picks[[1, 17, 40, 62]] = [-1, N_RAYS, INT32_MIN, INT32_MAX]
                named = picks[(picks >= 0) & (picks < N_RAYS)]
                rest = np.setdiff1d(np.arange(N_RAYS), named)
                ibuf, d_index, istart = guarded(m, 1, torch.int32, misalign)
                d_index.copy_(dev(picks.astype(np.int32)))
                bufs = [guarded(N_RAYS, words, dtype, misalign) for words, dtype in ((6, torch.float32), (3, torch.float32), (3, torch.float32), (4, torch.int32))]
                st = [b[1] for b in bufs]
                for view, src in zip(st, device_state(start)):
                    view.copy_(src)
                obufs = [guarded(N_RAYS, words, dtype, misalign) for words, dtype in ((1, torch.float32), (1, torch.int32), (6, torch.float32))]
                out = tuple(b[1] for b in obufs)
                step(sc.ctx, st, index=d_index, out=out)
                for (buf, _, at), words, name in zip(bufs + obufs, (6, 3, 3, 4, 1, 1, 6), ("rays", "throughput", "radiance", "seeds", "t", "idx", "hit")):
                    guards_intact(buf, at, words * N_RAYS, what + ": " + name)
                guards_intact(ibuf, istart, m, what + ": the index")
                assert np.array_equal(host(d_index), picks.astype(np.int32)), what + ": the index was written"
                compare_state(st, want[:4], what + ", the named rays", rows=named)
                compare_state(st, start, what + ", the rays no entry names", rows=rest)
                compare_outputs(out, w_t, w_idx, w_hit, what + ", the named rays", rows=named)
                for o in out:
                    assert (host(o).view(np.uint32).reshape(N_RAYS, -1)[rest] == SENTINEL).all(), what + ": an output no entry names was written"
        d_index = dev(rng.permutation(N_RAYS)[:900].astype(np.int32))
        named = host(d_index)
        rest = np.setdiff1d(np.arange(N_RAYS), named)
        st = device_state(start)
        outs = step(sc.ctx, st, index=d_index, hit=True)
        compare_outputs(outs, w_t, w_idx, w_hit, "%s, outputs allocated here, the named rays" % kind, rows=named)
        assert not host(outs[0])[rest].any() and (host(outs[1])[rest] == -1).all() and not bits(host(outs[2]))[rest].any(), kind
        for bad in ([-1], [N_RAYS], [INT32_MIN], [INT32_MAX], []):                # nothing but entries outside [0, n), or none at all
            st = device_state(start)
            step(sc.ctx, st, index=dev(np.array(bad, np.int32)))
            compare_state(st, start, "%s, the index %r" % (kind, bad))


def case_ordering():
    """7: on torch's non-default stream through set_stream, read after that stream alone is synchronised; after update_spheres /
    set_mesh_triangles from device tensors the calls answer for the new scene; renders before and after the calls equal renders without
    them, and the context's statistics do not move"""
    from conftest import assert_planes_equal
    stream = torch.cuda.Stream()
    filler = torch.ones((2048, 2048), device="cuda")
    for kind in ("s16", "big", "bvh", "mesh"):
        sc = SCENES[kind]
        want = reference_steps(kind)
        src = device_state(start_state(kind))
        st = [torch.zeros_like(x) for x in src]
        torch.cuda.synchronize()
        sc.ctx.set_stream(stream.cuda_stream)
        try:
            with torch.cuda.stream(stream):
                x = filler
                for _ in range(20):
                    x = x @ filler * 1e-3
                for a, b in zip(st, src):
                    a.copy_(b)
                sc.ctx.bounce_rays(st[0], st[3], st[1], st[2])
                live = sc.ctx.live_rays(st[1])               # (list and workspace allocated by torch on this stream)
                outs = sc.ctx.bounce_rays(st[0], st[3], st[1], st[2], index=live, hit=True)
            stream.synchronize()
            final = list(want[1][:4])
            final[1] = wavefront_throughput(kind, [np.arange(N_RAYS), host(live)[host(live) >= 0]])
            compare_state(st, final, "%s on the caller's stream" % kind)
            assert np.array_equal(host(live), inputs.live_list(want[0][1])[0]), kind
            assert np.array_equal(host(outs[1]) >= 0, want[1][4] == inputs.HIT), kind
            assert float(x.sum()) == float(x.sum())
        finally:
            torch.cuda.synchronize()
            sc.ctx.set_stream(None)
    # after device updates, at once: ordered behind the update by the stream alone
    sc = SCENES["bvh"]
    g = W.displaced_spheres(W.sphere_geometry(sc.spheres), 0.5, "wave", seed=2)
    moved = W.with_sphere_geometry(sc.spheres, g)
    d_g = dev(np.ascontiguousarray(g, np.float32))
    st = device_state(start_state("bvh"))
    torch.cuda.synchronize()
    with pkg.Context(0) as c:
        sc.set(c)
        c.update_spheres(d_g)
        c.bounce_rays(st[0], st[3], st[1], st[2])
        c.bounce_rays(st[0], st[3], st[1], st[2])
        c.synchronize()
        w = reference_steps("bvh", data=(moved, None, sc.planes))
        compare_state(st, w[1], "after update_spheres, against the reference of the moved scene")
        assert same_words(host(st[0]), reference_steps("bvh")[1][0]).size > 0, "the update moved nothing"
    sc = SCENES["mesh"]
    import mesh_rays
    t2 = mesh_rays.adversarial_scene(1, seed=4)[1]
    d_t2 = dev(np.ascontiguousarray(t2).view(np.float32).reshape(-1, 15).copy())
    st, fst = device_state(start_state("mesh")), device_state(start_state("mesh"))
    torch.cuda.synchronize()
    with pkg.Context(0) as c, pkg.Context(0) as fresh:
        sc.set(c)
        c.set_mesh_triangles(d_t2)
        c.bounce_rays(st[0], st[3], st[1], st[2])
        c.bounce_rays(st[0], st[3], st[1], st[2])
        c.synchronize()
        sc.set(fresh, triangles=t2)
        step(fresh, fst)
        step(fresh, fst)
        compare_state(st, [host(x) for x in fst], "after set_mesh_triangles, against a context set afresh")
        compare_state(st, reference_steps("mesh", data=(sc.spheres, t2, sc.planes))[1], "after set_mesh_triangles, against the reference")
        assert same_words(host(st[0]), reference_steps("mesh")[1][0]).size > 0, "the new triangles changed nothing"
    # renders around the calls
    cam = W.initial_camera()
    for kind in ("s16", "bvh", "mesh"):
        sc = SCENES[kind]
        st = device_state(start_state(kind))
        work = torch.empty(B.live_rays_bytes(N_RAYS), dtype=torch.uint8, device="cuda")
        live = torch.empty(N_RAYS, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        with pkg.Context(0) as c:
            sc.set(c)
            c.resize(64, 48)
            planes = []
            for calls in (False, True):
                c.init_output(P.SEED0)
                if calls:
                    c.bounce_rays(st[0], st[3], st[1], st[2])
                    c.live_rays(st[1], out=live, work=work)
                c.render(cam, 4, 2, pkg.INLINE)
                if calls:
                    before = c.stats()
                    c.bounce_rays(st[0], st[3], st[1], st[2], index=live)
                    c.live_rays(st[1], index=live, out=live, work=work)
                    c.synchronize()
                    after = c.stats()
                    assert (after["live_bounces"], after["samples"]) == (before["live_bounces"], before["samples"]), "%s: a step moved the statistics" % kind
                c.render(cam, 4, 1, pkg.STREAMS)
                planes.append(c.download_state())
            assert_planes_equal(planes[1], planes[0], "%s: renders around the stepped calls" % kind)
            assert np.any(np.asarray(planes[0][0]) != 0.0)
            c.synchronize()
            want = reference_steps(kind)
            compare_state([st[0], st[2], st[2], st[3]], [want[1][0], want[1][2], want[1][2], want[1][3]], "%s: steps around renders" % kind)
            assert np.array_equal(host(live), B.live_rays(host(st[1]), inputs.live_list(want[0][1])[0])[0]), kind


def case_refusals():
    """8: through the raw library handle -- PTMI_ESTATE before a scene (the step entries; the live list needs none), PTMI_EINVAL for a negative
    n or m, for NULL pointers with a positive count, for a scene with a GLASS sphere, for a short or misaligned workspace; nothing is written"""
    sc = SCENES["bvh"]
    n, m = 65, 40
    bufs = [guarded(n, words, dtype, False) for words, dtype in ((6, torch.float32), (3, torch.float32), (3, torch.float32), (4, torch.int32), (1, torch.float32),
                                                                 (1, torch.int32), (6, torch.float32), (1, torch.int32), (1, torch.int32))]
    rays_t, thr_t, rad_t, seed_t, t_t, idx_t, hit_t, live_t, cnt_t = (b[1] for b in bufs)
    d_index = dev(np.arange(m, dtype=np.int32))
    ones = torch.ones((n, 3), dtype=torch.float32, device="cuda")
    need = B.live_rays_bytes(n)
    work = torch.full((need + 16,), 0xA5, dtype=torch.uint8, device="cuda")
    assert work.data_ptr() % 8 == 0
    torch.cuda.synchronize()
    vp = lambda x: C.c_void_p(x.data_ptr())  # noqa: E731
    rays, thr, rad, sd, t, idx, hit, live, cnt, index, wk = (vp(x) for x in (rays_t, thr_t, rad_t, seed_t, t_t, idx_t, hit_t, live_t, cnt_t, d_index, work))
    one = vp(ones)

    def untouched(what):
        torch.cuda.synchronize()
        for b in bufs:
            assert (host(b[0]).view(np.uint32) == SENTINEL).all(), "%s wrote to an array" % what
        assert bool((work == 0xA5).all()), "%s wrote to the workspace" % what

    with pkg.Context(0) as c:
        lib, h = c._lib, c._h
        S, X, L = lib.ptmi_bounce_rays_device, lib.ptmi_bounce_rays_indexed_device, lib.ptmi_live_rays_device
        assert S(h, rays, n, thr, rad, sd, t, idx, hit) == B.PTMI_ESTATE and X(h, rays, n, index, m, thr, rad, sd, t, idx, hit) == B.PTMI_ESTATE
        untouched("a step before any scene")
        # the live list needs no scene; its refusals
        for rc in (L(h, one, -1, None, 0, live, cnt, wk, need), L(h, one, n, index, -1, live, cnt, wk, need), L(h, None, n, None, 0, live, cnt, wk, need),
                   L(h, one, n, None, 0, None, cnt, wk, need), L(h, one, n, None, 0, live, cnt, None, need), L(h, one, n, None, 0, live, cnt, wk, need - 1),
                   L(h, one, n, None, 0, live, cnt, wk, 0), L(h, one, n, None, 0, live, cnt, C.c_void_p(work.data_ptr() + 4), need),
                   L(h, one, n, None, 0, live, cnt, C.c_void_p(work.data_ptr() + 1), need), L(h, one, n, index, m, None, cnt, wk, need)):
            assert rc == B.PTMI_EINVAL, rc
        assert b"live-rays" in lib.ptmi_last_error(h)
        assert L(h, None, 0, None, 0, None, None, None, 0) == B.PTMI_OK and L(h, one, n, index, 0, live, cnt, wk, need) == B.PTMI_OK
        c.synchronize()
        untouched("a refused or empty live_rays")
        sc.set(c)
        for rc in (S(h, None, n, thr, rad, sd, t, idx, hit), S(h, rays, n, None, rad, sd, t, idx, hit), S(h, rays, n, thr, None, sd, t, idx, hit),
                   S(h, rays, n, thr, rad, None, t, idx, hit), S(h, rays, -1, thr, rad, sd, t, idx, hit),
                   X(h, None, n, index, m, thr, rad, sd, t, idx, hit), X(h, rays, n, index, m, None, rad, sd, t, idx, hit),
                   X(h, rays, n, index, m, thr, None, sd, t, idx, hit), X(h, rays, n, index, m, thr, rad, None, t, idx, hit),
                   X(h, rays, -1, index, m, thr, rad, sd, t, idx, hit), X(h, rays, n, index, -1, thr, rad, sd, t, idx, hit),
                   X(h, rays, n, None, m, thr, rad, sd, t, idx, hit)):
            assert rc == B.PTMI_EINVAL, rc
        assert b"ray-bounce" in lib.ptmi_last_error(h)
        assert S(h, None, 0, None, None, None, None, None, None) == B.PTMI_OK and X(h, rays, n, None, 0, thr, rad, sd, t, idx, hit) == B.PTMI_OK
        assert X(h, None, 0, index, m, None, None, None, None, None, None) == B.PTMI_OK
        c.synchronize()
        untouched("a refused or empty step")
        glass = sc.spheres[:40].copy()
        glass["brdf_tag"][3], glass["brdf_param"][3] = W.GLASS, 1.5
        c.set_scene(glass, sc.planes)
        assert S(h, rays, n, thr, rad, sd, t, idx, hit) == B.PTMI_EINVAL and b"GLASS" in lib.ptmi_last_error(h)
        assert X(h, rays, n, index, m, thr, rad, sd, t, idx, hit) == B.PTMI_EINVAL and b"GLASS" in lib.ptmi_last_error(h)
        c.synchronize()
        untouched("a step on a GLASS scene")
        assert L(h, one, n, None, 0, live, cnt, wk, need) == B.PTMI_OK                # the list asks nothing of the scene
        c.synchronize()
        assert np.array_equal(host(live_t), np.arange(n)) and int(cnt_t[0].item()) == n


RUN = dict(zip(CASES, (case_reference, case_trace_paths, case_sizes, case_wavefront, case_live_rays, case_indexed, case_ordering, case_refusals)))


def main():
    setup(sys.argv[1])
    for kind in KINDS:
        SCENES[kind] = P.SCENES[kind] = P.Scene(kind)
    for name in CASES:
        try:
            RUN[name]()
            print("ok %s" % name, flush=True)
        except AssertionError as e:
            print("FAILED %s: %s" % (name, str(e).replace("\n", " ")[:1500] or traceback.format_exc()[-1500:].replace("\n", " | ")), flush=True)
        except B.PtmiError as e:                     # a runtime error: nothing more is started on the device
            print("FAILED %s: %s" % (name, e), flush=True)
            raise SystemExit(3)
        except (IndexError, KeyError, TypeError, ValueError):      # a mistake of the case's own: the others still run
            print("FAILED %s: %s" % (name, traceback.format_exc()[-1500:].replace("\n", " | ")), flush=True)
    for sc in SCENES.values():
        sc.ctx.close()
    print("RAY_BOUNCE_DONE", flush=True)


if __name__ == "__main__":
    main()
