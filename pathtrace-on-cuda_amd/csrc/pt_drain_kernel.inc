// pt_drain_kernel.inc — the body of wf_drain / wf_drain_views (pt_wavefront.hip), included once into each.  In scope: sc, cam (a DevCamera,
// or the ViewTable of a batch of views), prm, b, slotIn, listIn, spreadShift and the template parameter QUAD.
    __shared__ int lds_stack[kWavesPerBlock][(QUAD ? kDrainQuadStack : kStackDepth) * 64];
    const uint32_t nIn = b.cnt[slotIn].nActive;
    // spreadShift: only every 2^s-th lane carries a stream.  The kernel is bound by latency (a wave steps at the pace of its slowest
    // lane, every bounce), and the chip is far from full at this point: thinner waves wait for the maximum of fewer paths
    const uint32_t t = blockIdx.x * (uint32_t)kBlockThreads + threadIdx.x;
    if (t & ((1u << spreadShift) - 1u)) return;
    const uint32_t idx = t >> spreadShift;
    if (idx >= nIn) return;
    int* stack = &lds_stack[threadIdx.x >> 6][threadIdx.x & 63];
    const uint32_t sid = b.active[listIn][idx];
    SState st;
    load_state(b, sid, st);
    for (;;) {
        float2 hitP = make_float2(0.f, __int_as_float(-1)), hitS = hitP, hitA = hitP;
        TraceStats ts{0, 0, 0};
        if (QUAD) {
            // The rays of this bounce (second-to-last shadow ray, shadow ray, path ray: any subset) in ONE flat loop: a lane that has finished a ray
            // sets up its next one inside the loop, so the wave waits for the lane with the most steps in all — not, as with one
            // loop per ray kind, for the slowest lane of each kind in turn.
            int todo = ((st.flags & F_SHADOWA) ? 1 : 0) | ((st.flags & F_SHADOW) ? 2 : 0) | ((st.flags & F_PATH) ? 4 : 0);
            f3 org(0.f, 0.f, 0.f), dir(0.f, 0.f, 1.f), inv(0.f, 0.f, 0.f);
            float cscale = 0.f, bestT = 0.f, stopBelow = 0.f;
            bool degenerate = false;
            int bestPrim = -1, cur = 0, sp = 0, kind = -1;
            for (;;) {
                if (kind < 0) {
                    if (todo == 0) break;
                    kind = __builtin_ctz((unsigned)todo); todo &= todo - 1;
                    if (kind == 0) {
                        const float4 ao = b.ray_o[2][sid], ad = b.ray_d[2][sid];
                        org = f3(ao.x, ao.y, ao.z); dir = f3(ad.x, ad.y, ad.z); bestT = ao.w; stopBelow = ad.w;
                    } else if (kind == 1) { org = st.shO; dir = st.shD; bestT = st.shTmax; stopBelow = shadow_stop_t(st.shO, st.shTmax); }
                    else { org = st.pathO; dir = st.pathD; bestT = 999999.f; stopBelow = -__builtin_inff(); }
                    ray_setup(dir, inv, cscale, degenerate);
                    bestPrim = -1; cur = 0; sp = 0;
                }
                if (quad_step(sc, org, dir, inv, cscale, degenerate, stopBelow, stack, cur, sp, bestT, bestPrim)) {
                    for (int s = 0; s < sc.n_spheres; s++) {      // spheres, in order, against the triangles' closest t (CudaUtil.cuh:137-145)
                        const float4 c = sc.spheres[4 * s];
                        float root;
                        if (sphere_root(f3(c.x, c.y, c.z), c.w, org, dir, bestT, root)) { bestT = root; bestPrim = sc.n_tris + s; }
                    }
                    const float2 h = make_float2(bestT, __int_as_float(bestPrim));
                    if (kind == 0) hitA = h; else if (kind == 1) hitS = h; else hitP = h;
                    kind = -1;
                }
            }
        } else {
        if (st.flags & F_SHADOWA) {
            const float4 ao = b.ray_o[2][sid], ad = b.ray_d[2][sid];
            float t; const int prim = trace_closest<false>(sc, f3(ao.x, ao.y, ao.z), f3(ad.x, ad.y, ad.z), ao.w, stack, t, ts); hitA = make_float2(t, __int_as_float(prim));
        }
        if (st.flags & F_SHADOW) { float t; const int prim = trace_closest<false>(sc, st.shO, st.shD, st.shTmax, stack, t, ts); hitS = make_float2(t, __int_as_float(prim)); }
        if (st.flags & F_PATH) { float t; const int prim = trace_closest<false>(sc, st.pathO, st.pathD, 999999.f, stack, t, ts); hitP = make_float2(t, __int_as_float(prim)); }
        }
        if (shade_step(sc, cam, prm, b, sid, st, hitP, hitS, hitA)) break;
    }
    write_mean(b, prm, sid, st);
