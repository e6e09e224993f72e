// pt_shade_kernel.inc — the body of wf_shade / wf_shade_views (pt_wavefront.hip), included once into each: one thread per live stream, one
// step.  In scope: sc, cam (a DevCamera, or the ViewTable of a batch of views), prm, b, slotIn, slotOut, slotClear, listIn and the
// template parameters TWO, PHASE, MARK.
    static_assert(PHASE == 0 || MARK, "the two-phase step needs the not-ready marks");
    const uint32_t nIn = b.cnt[slotIn].nActive;
    if (PHASE != 1 && blockIdx.x == 0) for (int k = threadIdx.x; k < kWfSlotBytes / 4; k += blockDim.x) ((uint32_t*)&b.cnt[slotClear])[k] = 0;
    if ((uint32_t)blockIdx.x * blockDim.x >= nIn) return;
    const uint32_t idx = blockIdx.x * blockDim.x + threadIdx.x;
    const bool have = idx < nIn;
    bool alive = false, emit[kRayKinds] = {false, false, false};
    uint32_t sid = 0, resume = 0;      // resume: the queued rays are suspended traversals (wf_trace then reads their records)
    uint32_t cls = 0;                  // bit k: the ray of kind k this step emitted is short (queued from the back of its queue)
    bool step = have;
    if (have) {
        // While no stream has retired yet (more than half of a render's iterations) every stream is alive, so list position idx can
        // simply take stream idx: one dependent fetch level less for the whole step (the list itself is in stream order only inside the
        // blocks that appended to it; any one-to-one assignment of streams to lanes gives the same result).
        sid = (nIn == (uint32_t)prm.n_units * 64u) ? idx : ld_s(&b.active[listIn][idx]);
        if (PHASE == 2) {
            const uint32_t r = b.res[idx];
            if (r & R_DONE) {      // shaded by phase 1: only the appends are left
                step = false;
                alive = (r & R_ALIVE) != 0; emit[0] = (r & R_EMIT0) != 0; emit[1] = (r & R_EMIT1) != 0; emit[2] = (r & R_EMIT2) != 0;
                cls = (r / R_SHORT0) & 7u;
            }
        }
    }
    if (step) {
        SState st;
        float2 hitP, hitS, hitA;
        if (PHASE == 1) { hitP = load_hit_coherent(&b.hit[0][sid]); hitS = load_hit_coherent(&b.hit[1][sid]); hitA = load_hit_coherent(&b.hit[2][sid]); }
        else { hitP = ld_s(&b.hit[0][sid]); hitS = ld_s(&b.hit[1][sid]); hitA = ld_s(&b.hit[2][sid]); }      // same fetch level as the state
        load_state(b, sid, st);
        // a ray of this stream is still being traversed (time-sliced): wait one iteration
        const int pendP = (st.flags & F_PATH) ? __float_as_int(hitP.y) : -1, pendS = (st.flags & F_SHADOW) ? __float_as_int(hitS.y) : -1;
        const int pendA = (st.flags & F_SHADOWA) ? __float_as_int(hitA.y) : -1;
        if (PHASE == 1 && (pendP <= -2 || pendS <= -2 || pendA <= -2)) {
            // phase 1: a ray is not back yet (kNotReady), or a traversal is suspended (its slot keeps the record number until wf_trace
            // resumes it, so the slot cannot tell "back" from "not yet"): phase 2 takes the stream
            step = false;
        } else if (pendP <= -2 || pendS <= -2 || pendA <= -2) {
            alive = true; emit[0] = pendP <= -2; emit[1] = pendS <= -2; emit[2] = pendA <= -2; resume = kResumeBit;
        } else {
            const bool done = shade_step_t<TWO>(sc, cam, prm, b, sid, st, hitP, hitS, hitA);
            if (done) {
                write_mean(b, prm, sid, st);
            } else {
                const uint32_t nf = st.flags;
                store_state(b, sid, st);
                alive = true;
                emit[0] = (nf & F_PATH) != 0; emit[1] = (nf & F_SHADOW) != 0; emit[2] = (nf & F_SHADOWA) != 0;
                cls = st.cls;
            }
        }
    }
    // MARK: the hit slot of every ray this step emitted says "not traced yet" until wf_trace publishes its hit (a suspended traversal
    // that is re-queued keeps its slot: it holds the record number).  Written here, at the end, where nothing else is live.
    if (MARK && step && !resume) {
#pragma unroll
        for (int k = 0; k < kRayKinds; k++) if (emit[k]) b.hit[k][sid] = make_float2(0.f, __int_as_float(kNotReady));
    }
    if (PHASE == 1) {
        if (have) b.res[idx] = (uint8_t)(step ? (R_DONE | (alive ? R_ALIVE : 0u) | (emit[0] ? R_EMIT0 : 0u) | (emit[1] ? R_EMIT1 : 0u) | (emit[2] ? R_EMIT2 : 0u) | (cls & 7u) * R_SHORT0) : 0u);
        return;
    }
    // a re-queued suspended traversal is long by definition: cls = 0 for it (it never went through the step)
    const bool s0 = (cls & 1u) != 0, s1 = (cls & 2u) != 0, s2 = (cls & 4u) != 0;
    const uint32_t topIdx = (uint32_t)(b.hit[1] - b.hit[0]) - 1u;      // n16 - 1
    const bool e[kLists] = {alive, emit[0] && !s0, emit[1] && !s1, emit[2] && !s2, emit[0] && s0, emit[1] && s1, emit[2] && s2};
    uint32_t* const c[kLists] = {&b.cnt[slotOut].nActive, &b.cnt[slotOut].nRays[0][0], &b.cnt[slotOut].nRays[1][0], &b.cnt[slotOut].nRays[2][0],
                                 &b.cnt[slotOut].nRays[0][kShortWord], &b.cnt[slotOut].nRays[1][kShortWord], &b.cnt[slotOut].nRays[2][kShortWord]};
    uint32_t* const l[kLists] = {b.active[listIn ^ 1], b.rq[0], b.rq[1], b.rq[2], b.rq[0], b.rq[1], b.rq[2]};
    const uint32_t ids[kLists] = {sid, sid | resume, sid | resume, sid | resume, sid, sid, sid};
    const uint32_t top[kLists] = {0u, 0u, 0u, 0u, topIdx, topIdx, topIdx};
    block_append<kLists>(e, ids, c, l, top);
