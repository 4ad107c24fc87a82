// ptmi_inline_body.inc -- the body of render_inline_kernel, shared by the kernel of linear scenes and render_inline_bvh_kernel (BVH scenes) and
// render_inline_mesh_kernel (mesh scenes).
// Included INSIDE the kernels (ptmi_inline.hip), which define PTMI_HIT(STAGED, S, ns, np, o, d[, diag]) -- the hit search --, PTMI_HIT_RECORD and PTMI_NORMAL_AT (hit_record and
// normal_at, or a mesh scene's) and, for the BVH and mesh
// kernel, LDS_SCENE = false.  (A __device__ function for the body changes the code the compiler makes of the linear kernels; the
// text shared this way leaves them instruction for instruction as they were: tools/isa_diff.py.)
    __shared__ float pixel_const[10][kRenderBlock];         // per-lane restart record (see below)
    extern __shared__ float4 lds_scene[];
    const int ns = a.scene.n_spheres, np = a.scene.n_planes;
    if (LDS_SCENE) {
        const int total = a.scene.total_f4();
        for (int i = threadIdx.x; i < total; i += kRenderBlock) lds_scene[i] = a.scene.packed[i];
        __syncthreads();
    }
    const float4 *S = LDS_SCENE ? lds_scene : a.scene.packed;
    const float4 *M = S + a.scene.geom_f4();

    // SAMPLE CHUNKS (a.spp_chunks > 1; tiled kernels only).  A pixel's samples are one serial chain, so a launch has as
    // many waves as the image has tiles, each as long as n_spp; with few tiles and many samples -- one of 8 parts of a
    // 4K image at 1024 spp: 16 200 waves for 6 144 slots -- the last round of waves runs on a partly empty chip and
    // costs 15 %.  The grid is therefore spp_chunks copies of the tile grid: copy c of a tile renders samples
    // [c S, (c+1) S) of its pixels, after copy c-1 has stored the planes and published done[tile] = c.  A workgroup's place
    // in that chain is a ticket it draws when it starts (enter_sample_chunk), so the producer of what it waits for has
    // started before it, whatever order the hardware dispatches workgroups in (in practice the producer finished a whole
    // round earlier: the wait falls through).  The planes travel through
    // memory between copies: release / acquire at agent scope (L2 write-back, L1 invalidate); copies of one tile run on
    // the same XCD (the grid of a copy is a multiple of 32).  Results do not depend on the chunking (sample-split invariance).
    unsigned int wg; int chunk, n_spp_chunk;
    enter_sample_chunk<TILE_W>(a, wg, chunk, n_spp_chunk);
    long long pixel;
    unsigned int quad, trips = 0;
    const bool valid = lane_pixel<TILE_W>(a, pixel, quad, wg);
    unsigned int live = 0;
    if (valid) {
        const int local_row = (int)(pixel / a.width);
        const int col = (int)(pixel - (long long)local_row * a.width);
        int64_t px = col, py = global_row(local_row, a.stripe_rows, a.n_parts, a.part);
        if (a.screen_x) { px = a.screen_x[pixel]; py = a.screen_y[pixel]; }

        const V3 origin = a.cam.pos;
        const V3 primary = primary_direction(a.cam, px, py);

        V3 acc = mk(a.planes.r[pixel], a.planes.g[pixel], a.planes.b[pixel]);
        Sfc32 seed;
        seed.a = a.planes.sa[pixel]; seed.b = a.planes.sb[pixel];
        seed.c = a.planes.sc[pixel]; seed.counter = a.planes.sctr[pixel];

        const int limit = a.bounce_limit, n_spp = n_spp_chunk;

        if (limit <= 0) {
            // iterate 0: every sample returns (0, seed); new + old
            if (n_spp > 0) acc = mk(0.0f, 0.0f, 0.0f) + acc;
        } else {
            // primaryRays has no sub-pixel jitter (Trace.hs:244-262): every sample of a pixel shoots the same primary ray, so
            // its checkHit + hit are evaluated ONCE per pixel and every sample starts from that record.
            // Loop shape: [finish frozen shades][restart][shade][trace].  A lane comes round with a hit to shade (`pending`) or
            // with its sample over (`over`: the trace missed, or the last shade left a throughput that the next prepareRay
            // freezes).  The shades whose outcome is CERTAIN to be frozen (the iteration limit, or surely_frozen_after) are
            // finished first -- emittance + three draws, no sin/cos, no rotation -- and those lanes are `over` too; then ONE
            // block restarts every `over` lane on its pixel's next sample, from the cached primary hit, with the rotation axis
            // and half-angle scale that every first shade of the pixel uses; then one full shade and one trace for all.  A
            // sample whose path ends by a certain freeze -- 64 % of them on C2 -- costs k-1 full shades and k-1 traces.
            const HitSel h0 = PTMI_HIT(LDS_SCENE, S, ns, np, origin, primary);
            if (!h0.just) {
                if (n_spp > 0) acc = mk(0.0f, 0.0f, 0.0f) + acc;     // every sample: result 0, seed untouched
            } else {
                // What a sample restarts from lives in a lane-private LDS column (10 words), not in VGPRs: the position of the
                // primary hit, the axis and half-angle scale of its bounce, and the pixel's accumulator (touched once per sample).
                float *mine = &pixel_const[0][threadIdx.x];
                auto put = [&](int k, float v) { mine[k * kRenderBlock] = v; };
                auto get = [&](int k) { return mine[k * kRenderBlock]; };
                V3 pos, normal;                                       // pos: the hit to shade, then the next ray's origin
                PTMI_HIT_RECORD(S, ns, h0.idx, origin, primary, h0.t, pos, normal);
                const int idx0 = h0.idx;
                {
                    const float4 mb0 = M[2 * idx0 + 1];
                    V3 axis0; float hk0;
                    bounce_axis(mb0, normal, primary, axis0, hk0);
                    put(0, pos.x); put(1, pos.y); put(2, pos.z);
                    put(3, axis0.x); put(4, axis0.y); put(5, axis0.z); put(6, hk0);
                    put(7, acc.x); put(8, acc.y); put(9, acc.z);
                }
                int s = -1, it = 0, idx = idx0;                       // s: the sample being rendered (the first restart makes it 0)
                V3 d = primary;
                V3 throughput = mk(1.0f, 1.0f, 1.0f), result = mk(0.0f, 0.0f, 0.0f);
                bool pending = false, has_ray = false, over = n_spp > 0;
                diag::PhaseProbe phase;                               // (diagnostic builds: ptmi_diag.h)
                while (pending || over) {
                    ++trips;
                    phase.trip(); phase.round_a(pending || over);
                    float4 mb = M[2 * idx + 1];
                    V3 axis = mk(0.0f, 0.0f, 0.0f); float hk = 0.0f;
                    phase.check(pending);
                    if (pending) {
                        bounce_axis(mb, normal, d, axis, hk);
                        const float4 ma = M[2 * idx];
                        if (it + 1 >= limit || surely_frozen_after(ma, mb, axis, throughput)) {
                            finish_frozen(ma, throughput, result, seed);
                            ++live;
                            phase.frozen();
                            pending = false; over = true;
                        }
                    }
                    phase.restart(over);
                    if (over) {                                        // next sample of this pixel
                        // \(new, seed') (old, _) -> (new + old, seed') -- once a sample has been rendered (the first time round
                        // the lane only starts sample 0)
                        if (s >= 0) { put(7, result.x + get(7)); put(8, result.y + get(8)); put(9, result.z + get(9)); }
                        ++s; it = 0;
                        throughput = mk(1.0f, 1.0f, 1.0f); result = mk(0.0f, 0.0f, 0.0f);
                        pos = mk(get(0), get(1), get(2)); idx = idx0;
                        mb = M[2 * idx0 + 1];
                        axis = mk(get(3), get(4), get(5)); hk = get(6);
                        over = false; pending = s < n_spp;
                    }
                    phase.shade(pending);
                    if (pending) {
                        V3 next; float brdf;
                        sincos3_probe(a.work_counter, hk, seed);
                        next_about_axis(mb, axis, hk, seed, next, brdf);
                        apply_bounce(M, idx, pos, next, brdf, pos, d, throughput, result);
                        ++it; ++live;
                        pending = false;
                        // the next prepareRay would freeze the path (Trace.hs:364-365)
                        if (it >= limit || near_zero(throughput)) over = true;
                        else has_ray = true;
                    }
                    phase.end_a(); phase.round_c(has_ray);
                    if (has_ray) {
                        const HitSel h = PTMI_HIT(LDS_SCENE, S, ns, np, pos, d, diag::sphere_counters(a.work_counter));
                        has_ray = false;
                        if (h.just) {
                            PTMI_HIT_RECORD(S, ns, h.idx, pos, d, h.t, pos, normal);
                            idx = h.idx;
                            pending = true;
                        } else {
                            over = true;
                        }
                    }
                    phase.end_c();
                }
                acc = mk(get(7), get(8), get(9));
                phase.flush(a.work_counter);
            }
        }

        a.planes.r[pixel] = acc.x; a.planes.g[pixel] = acc.y; a.planes.b[pixel] = acc.z;
        a.planes.sa[pixel] = seed.a; a.planes.sb[pixel] = seed.b;
        a.planes.sc[pixel] = seed.c; a.planes.sctr[pixel] = seed.counter;
    }
    leave_sample_chunk<TILE_W>(a, wg, chunk);

    if (TILE_W > 0) record_cost(a, quad, trips);
    if (a.live_counter) {
        const unsigned long long total = wave_sum(live);
        if ((threadIdx.x & 63) == 0 && total) atomicAdd(a.live_counter + (size_t)(blockIdx.x & (kStatShards - 1)) * kStatStride, total);
    }
