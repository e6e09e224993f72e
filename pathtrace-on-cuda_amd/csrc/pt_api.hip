// pt_api.hip — device half of the C-ABI (include/pt_api.h): scene upload into the HBM
// layout of pt_device.h, render launch sequence, tile gather helpers, parity hooks.
//
// Replaces the body of PathTracer::Render (srcs/pathtracer.cu:124-259): instead of five
// cudaMallocManaged regions filled element by element from the host and a device vtable
// plant, the scene is repacked once on the host into 16-byte records and copied with one
// hipMemcpy per array; instead of NUM_MULTI_SAMPLE synchronous launches there is one
// persistent launch over all (tile, pass) units on the caller's stream.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstring>
#include <cmath>
#include <map>
#include <string>
#include <vector>

#include "pt_internal.h"
#include "../host/accel_build.h"

struct PtScene {
    int device = 0;
    ptd::DevScene dev{};
    void* d_nodes = nullptr; void* d_quad = nullptr; void* d_tri = nullptr; void* d_tripair = nullptr; void* d_leafbox = nullptr;
    void* d_surf = nullptr;
    void* d_lights = nullptr; void* d_spheres = nullptr; void* d_core = nullptr;
    unsigned int* d_unit_counter = nullptr;
    void* d_counters = nullptr;
    int32_t* d_tile_list = nullptr;      // the tile numbers of the pt_render_tile_list call in flight (grown on demand)
    int64_t tile_list_cap = 0;           // entries allocated
    void* d_views = nullptr;             // the cameras of the pt_render_views call in flight (grown on demand): origins (float4) | DevCamera | first pass (int32), view_cap of each
    int64_t view_cap = 0;                // views allocated
    std::vector<char> h_views;           // host image of d_views (the source of its stream-ordered copy)
    int64_t bytes = 0;
    int n_lights = 0;
    int max_depth = 0;
    int num_cus = 256;
    bool count_next = false;
    int mode = 1;            // 1 = wavefront pipeline (default), 0 = one-kernel state machine
    uint32_t* h_poll = nullptr;   // pinned, for the pipeline's live-stream count
    int last_iters = 0;
    int shade_rounds = 1;        // wf_shade: 1 = a stream may start its next sample in the step its path ends, 0 = one bounce per step, -1 = by live-stream count (PTAMD_TRS)
    int early_below = 2500000;   // renders of at most this many streams (pixels x passes of one call) run wf_shade's early phase beside the draining wf_trace (0 = never; pt_set_early_shade)
    int drain_below = 80000;     // hand the last streams of a render to wf_drain once this few are live (0 = never; PTAMD_DRAIN, pt_set_drain_threshold):
                                 // the last ~200 of ~1,100 bounce iterations serve < 5 % of the streams at the latency of the longest ray each
                                 // (~200 us); wf_drain runs those streams to their end in one launch, spread over every SIMD.  40,000-120,000 is flat:
                                 // +5...7 % for an 8-way rank, +3 % 4-way, +1 % on one GPU (r03_b31.log, r03_b32.log, r03_b33.log)
    // optional per-launch timing of the traversal kernel (pt_enable_trace_timing)
    std::vector<hipEvent_t> trace_ev;
    int trace_ev_used[4] = {0, 0, 0, 0};     // per cohort
    int trace_ev_per = 0;                    // event pairs per cohort in the last render
    hipStream_t xstreams[3] = {nullptr, nullptr, nullptr};   // extra streams for concurrent cohorts
    hipEvent_t ev_fork = nullptr, ev_join[3] = {nullptr, nullptr, nullptr};
    // ring of HIP event pairs, one pair per render_units launch (pt_render_timings)
    static constexpr int kEvRing = 64;
    hipEvent_t ev[kEvRing][2] = {};
    int ev_count = 0;        // launches recorded since the last pt_render_timings(reset)
    // ---- dynamic geometry (pt_scene_update_vertices, csrc/pt_dynamic.hip) ----
    size_t array_bytes[9] = {};          // nodes quad tri tripair leafbox surf lights spheres core, as uploaded (pt_dbg_scene_array)
    std::vector<float> h_spheres;        // the uploaded sphere records: pt_scene_update_spheres checks the materials against them and copies from here
    struct DynHost {                     // the maps of the build, kept on the host until the first update uploads them
        std::vector<int32_t> bn, order, level_start, wide_bn, quad_bn, leaf_range, tmap, light_prim;
        std::vector<uint8_t> small;
        double area_sum = 0.0;
    } dyn_host;
    ptd::DynScene dyn{};                 // device side of the same, valid once dyn_ready
    static constexpr int kDynAllocs = 12;    // 8 maps (bn order wide_bn quad_bn leaf_range tmap light_prim small) + 4 scratch (bbox maxabs core_partial area_partial)
    void* d_dyn[kDynAllocs] = {};        // its allocations, in that order (dyn_prepare)
    bool dyn_ready = false;
    bool updated = false;
    std::vector<double> h_area;          // host image of dyn.area_partial
    // ---- ray queries (pt_trace_rays, csrc/pt_query.hip) ----
    bool query_quad = true;              // walk the 4-wide tree when it fits the kernel's stack (PTAMD_QUERY_QUAD=0: the binary tree, A/B)
};

static int upload(void** dptr, const void* h, size_t bytes, int64_t& total)
{
    size_t alloc = bytes ? bytes : 16;
    HIPCHK(hipMalloc(dptr, alloc));
    if (bytes) HIPCHK(hipMemcpy(*dptr, h, bytes, hipMemcpyHostToDevice));
    total += (int64_t)alloc;
    return PT_OK;
}

static inline float as_float(int32_t i) { float f; memcpy(&f, &i, 4); return f; }

template <class F>
static int with_buffers(int device, const void* in, size_t in_bytes, void* out, size_t out_bytes, void* out2, size_t out2_bytes, F launch)
{
    HIPCHK(hipSetDevice(device));
    void *d_in = nullptr, *d_out = nullptr, *d_out2 = nullptr;
    auto body = [&]() -> int {
        HIPCHK(hipMalloc(&d_in, in_bytes ? in_bytes : 16));
        HIPCHK(hipMalloc(&d_out, out_bytes ? out_bytes : 16));
        HIPCHK(hipMalloc(&d_out2, out2_bytes ? out2_bytes : 16));
        if (in_bytes) HIPCHK(hipMemcpy(d_in, in, in_bytes, hipMemcpyHostToDevice));
        HIPCHK(launch(d_in, d_out, d_out2));
        HIPCHK(hipDeviceSynchronize());
        if (out_bytes) HIPCHK(hipMemcpy(out, d_out, out_bytes, hipMemcpyDeviceToHost));
        if (out2_bytes) HIPCHK(hipMemcpy(out2, d_out2, out2_bytes, hipMemcpyDeviceToHost));
        return PT_OK;
    };
    const int rc = body();
    (void)hipFree(d_in); (void)hipFree(d_out); (void)hipFree(d_out2);      // on every path (hipFree(nullptr) is a no-op)
    return rc;
}


extern "C" {

int pt_scene_create(const PtBVHNode* nodes, int32_t n_nodes, const PtTriangle* tris, int32_t n_tris,
                    const PtSphere* spheres, int32_t n_spheres, int32_t device, PtScene** out)
{
    if (!out) { pt_set_error("pt_scene_create: out is NULL"); return PT_ERR_INVALID; }
    *out = nullptr;
    if (!nodes || n_nodes < 1 || !tris || n_tris < 1 || n_spheres < 0 || (n_spheres > 0 && !spheres)) {
        pt_set_error("pt_scene_create: empty or NULL scene arrays (n_nodes=%d n_tris=%d n_spheres=%d)", n_nodes, n_tris, n_spheres);
        return PT_ERR_INVALID;
    }
    // ---- validate the flattened tree and measure its depth (host check before any kernel sees it) ----
    std::vector<int> depth((size_t)n_nodes, -1);
    std::vector<int> widx((size_t)n_nodes, -1);
    int n_wide = 0, max_depth = 0;
    {
        std::vector<int> st; st.push_back(0); depth[0] = 0;
        std::vector<char> seen((size_t)n_nodes, 0);
        while (!st.empty()) {
            int i = st.back(); st.pop_back();
            if (seen[(size_t)i]) { pt_set_error("pt_scene_create: node %d reachable twice", i); return PT_ERR_INVALID; }
            seen[(size_t)i] = 1;
            const PtBVHNode& n = nodes[i];
            if (depth[i] > max_depth) max_depth = depth[i];
            const bool leaf = (n.primStart != -1 && n.primEnd != -1);
            if (leaf) {
                if (n.primStart < 0 || n.primEnd < n.primStart || n.primEnd >= n_tris || n.primEnd - n.primStart + 1 > 7) {
                    pt_set_error("pt_scene_create: leaf %d has bad primitive range [%d,%d]", i, n.primStart, n.primEnd);
                    return PT_ERR_INVALID;
                }
                if (n.childL > 0 || n.childR > 0) { pt_set_error("pt_scene_create: leaf %d has children", i); return PT_ERR_INVALID; }
            } else {
                if (n.childL <= 0 || n.childR <= 0 || n.childL >= n_nodes || n.childR >= n_nodes) {
                    pt_set_error("pt_scene_create: interior node %d has bad children (%d,%d)", i, n.childL, n.childR);
                    return PT_ERR_INVALID;
                }
                widx[(size_t)i] = 0;    // numbered below, in index order (= the reference's pre-order)
                depth[n.childL] = depth[i] + 1; depth[n.childR] = depth[i] + 1;
                st.push_back(n.childR); st.push_back(n.childL);
            }
        }
    }
    // every triangle must belong to exactly one reference leaf (its box decides acceptance)
    {
        std::vector<char> covered((size_t)n_tris, 0);
        for (int i = 0; i < n_nodes; i++) {
            const PtBVHNode& n = nodes[i];
            if (widx[(size_t)i] == -1 && depth[(size_t)i] >= 0 && n.primStart != -1 && n.primEnd != -1)
                for (int k = n.primStart; k <= n.primEnd; k++) covered[(size_t)k]++;
        }
        for (int k = 0; k < n_tris; k++)
            if (covered[(size_t)k] != 1) { pt_set_error("pt_scene_create: triangle %d is in %d reference leaves", k, (int)covered[(size_t)k]); return PT_ERR_INVALID; }
    }
    // ---- traversal tree over the triangles (host/accel_build.cpp) ----
    PtAccel accel;
    pt_build_accel(nodes, n_nodes, tris, n_tris, accel);
    if (accel.depth > ptd::kStackDepth) {
        pt_set_error("pt_scene_create: traversal tree depth %d exceeds the traversal stack (%d)", accel.depth, ptd::kStackDepth);
        return PT_ERR_UNSUPPORTED;
    }
    if (3 * accel.quad_depth + 2 > ptk_wf_stack_capacity()) {
        pt_set_error("pt_scene_create: 4-wide traversal tree depth %d needs more than the %d stack entries of the traversal kernel",
                     accel.quad_depth, ptk_wf_stack_capacity());
        return PT_ERR_UNSUPPORTED;
    }
    max_depth = accel.depth;
    n_wide = accel.n_wide;

    // ---- triangles: surface records (reference order), lights ----
    std::vector<float> surf((size_t)n_tris * 48), lights;
    std::vector<int32_t> light_prim;          // reference-order triangle of every light (for a vertex update)
    int n_lights = 0;
    for (int i = 0; i < n_tris; i++) {
        const PtTriangle& t = tris[i];
        float* a = &surf[(size_t)i * 48];
        const float* src[12] = {t.V0, t.E1, t.E2, t.N0, t.N1, t.N2, t.T0, t.T1, t.T2, t.B0, t.B1, t.B2};
        for (int k = 0; k < 12; k++) { a[3 * k] = src[k][0]; a[3 * k + 1] = src[k][1]; a[3 * k + 2] = src[k][2]; }
        const PtMaterial& m = t.mat0;           // Triangle::hit copies mat0 only (CudaPrimitive.cuh:149-154)
        const float rec[12] = {m.emittance[0], m.emittance[1], m.emittance[2], m.albedo[0], m.albedo[1], m.albedo[2],
                               m.specular[0], m.specular[1], m.specular[2], m.opacity, m.roughness, m.metallic};
        memcpy(a + 36, rec, sizeof(rec));
        auto len = [](const float* e) { return std::sqrt(e[0] * e[0] + e[1] * e[1] + e[2] * e[2]); };
        if (len(t.mat0.emittance) > 0.0001f || len(t.mat1.emittance) > 0.0001f || len(t.mat2.emittance) > 0.0001f) {
            const float rec[16] = {t.V0[0], t.V0[1], t.V0[2], t.V1[0], t.V1[1], t.V1[2], t.V2[0], t.V2[1], t.V2[2],
                                   t.normal[0], t.normal[1], t.normal[2], t.area, 0.f, 0.f, 0.f};
            lights.insert(lights.end(), rec, rec + 16);
            light_prim.push_back(i);
            n_lights++;
        }
    }
    // dead-NEE-term pruning (pt_stream.h: bounce) needs every emittance a shadow ray can return to be finite, non-negative and small
    // enough that (weight * brdfcos) * Le cannot overflow where the pruned case assumes it is finite: |wb| < 1e30 and Le <= 1e8 give
    // |wb * Le| < 1e38 < FLT_MAX.  (With a brighter light wb * Le can be inf, inf * 0 is NaN, and the reference adds that NaN to the
    // radiance, include/CudaUtil.cuh:271-272; such scenes keep all their shadow rays.)
    bool emitOk = true;
    auto okE = [](const float* e) { return std::isfinite(e[0]) && std::isfinite(e[1]) && std::isfinite(e[2]) && e[0] >= 0.f && e[1] >= 0.f && e[2] >= 0.f &&
                                           e[0] <= 1e8f && e[1] <= 1e8f && e[2] <= 1e8f; };
    for (int i = 0; i < n_tris; i++) emitOk = emitOk && okE(tris[i].mat0.emittance);
    for (int i = 0; i < n_spheres; i++) emitOk = emitOk && okE(spheres[i].mat.emittance);
    // ---- core box: the AABB of the scene's SMALL triangles (bounding-box diagonal under an eighth of the scene's).  A ray whose
    // segment misses it can only meet the few big triangles, i.e. is short, and wf_shade queues such rays last (pt_stream.h:
    // ray_is_short) so that the traversal kernel's launch tail consists of short rays.  Scheduling only — any box gives the same frame.
    std::vector<float> core;
    std::vector<uint8_t> small;               // per triangle: inside the core box's set (for a vertex update)
    {
        float smn[3] = {1e30f, 1e30f, 1e30f}, smx[3] = {-1e30f, -1e30f, -1e30f};
        auto tribox = [&](const PtTriangle& t, float* mn, float* mx) {
            for (int k = 0; k < 3; k++) { mn[k] = std::fmin(t.V0[k], std::fmin(t.V1[k], t.V2[k])); mx[k] = std::fmax(t.V0[k], std::fmax(t.V1[k], t.V2[k])); }
        };
        for (int i = 0; i < n_tris; i++) { float mn[3], mx[3]; tribox(tris[i], mn, mx); for (int k = 0; k < 3; k++) { smn[k] = std::fmin(smn[k], mn[k]); smx[k] = std::fmax(smx[k], mx[k]); } }
        const float sd = std::sqrt((smx[0] - smn[0]) * (smx[0] - smn[0]) + (smx[1] - smn[1]) * (smx[1] - smn[1]) + (smx[2] - smn[2]) * (smx[2] - smn[2]));
        float cmn[3] = {1e30f, 1e30f, 1e30f}, cmx[3] = {-1e30f, -1e30f, -1e30f};
        int nSmall = 0;
        for (int i = 0; i < n_tris; i++) {
            float mn[3], mx[3]; tribox(tris[i], mn, mx);
            const float dd = std::sqrt((mx[0] - mn[0]) * (mx[0] - mn[0]) + (mx[1] - mn[1]) * (mx[1] - mn[1]) + (mx[2] - mn[2]) * (mx[2] - mn[2]));
            if (dd * 8.f < sd) { if (small.empty()) small.assign((size_t)n_tris, 0); small[(size_t)i] = 1; nSmall++; for (int k = 0; k < 3; k++) { cmn[k] = std::fmin(cmn[k], mn[k]); cmx[k] = std::fmax(cmx[k], mx[k]); } }
        }
        const double sv = (double)(smx[0] - smn[0]) * (smx[1] - smn[1]) * (smx[2] - smn[2]);
        const double cv = nSmall ? (double)(cmx[0] - cmn[0]) * (cmx[1] - cmn[1]) * (cmx[2] - cmn[2]) : 0.0;
        // worth it only if the small triangles are many (they are what makes rays long) and leave a good part of the scene free;
        // PTAMD_CLASS=0 switches the queue order off (A/B)
        if (nSmall >= 64 && std::isfinite(sv) && sv > 0.0 && cv <= 0.6 * sv && !(getenv("PTAMD_CLASS") && atoi(getenv("PTAMD_CLASS")) == 0)) {
            for (int k = 0; k < 3; k++) { const float pad = 0.01f * (cmx[k] - cmn[k]) + 1e-4f * sd; cmn[k] -= pad; cmx[k] += pad; }
            core = {cmn[0], cmn[1], cmn[2], cmx[0], cmx[1], cmx[2]};
        }
    }
    std::vector<float> sph((size_t)n_spheres * 16);
    for (int i = 0; i < n_spheres; i++) {
        const PtSphere& s = spheres[i];
        float* a = &sph[(size_t)i * 16];
        a[0] = s.center[0]; a[1] = s.center[1]; a[2] = s.center[2]; a[3] = s.rad;
        memcpy(a + 4, &s.mat, sizeof(PtMaterial));
    }

    HIPCHK(hipSetDevice(device));
    PtScene* sc = new PtScene();
    sc->device = device;
    sc->n_lights = n_lights;
    sc->max_depth = max_depth;
    int rc;
    if ((rc = upload(&sc->d_nodes, accel.wide.data(), accel.wide.size() * 4, sc->bytes)) ||
        (rc = upload(&sc->d_quad, accel.quad.data(), accel.quad.size() * 4, sc->bytes)) ||
        (rc = upload(&sc->d_tri, accel.tri.data(), accel.tri.size() * 4, sc->bytes)) ||
        (rc = upload(&sc->d_tripair, accel.tripair.data(), accel.tripair.size() * 4, sc->bytes)) ||
        (rc = upload(&sc->d_leafbox, accel.leafbox.data(), accel.leafbox.size() * 4, sc->bytes)) ||
        (rc = upload(&sc->d_surf, surf.data(), surf.size() * 4, sc->bytes)) ||
        (rc = upload(&sc->d_lights, lights.data(), lights.size() * 4, sc->bytes)) ||
        (rc = upload(&sc->d_spheres, sph.data(), sph.size() * 4, sc->bytes)) ||
        (!core.empty() && (rc = upload(&sc->d_core, core.data(), core.size() * 4, sc->bytes)))) {
        pt_scene_destroy(sc);
        return rc;
    }
    // from here on every failure destroys the half-built scene (geometry already uploaded, events, streams)
    auto finish = [&]() -> int {
        HIPCHK(hipMalloc((void**)&sc->d_unit_counter, 64));
        HIPCHK(hipMalloc(&sc->d_counters, ptd::kStatBytes));      // 8 work counters (+ the diagnostic launch timeline of wf_trace)
        HIPCHK(hipMemset(sc->d_counters, 0, ptd::kStatBytes));
        for (int i = 0; i < PtScene::kEvRing; i++) { HIPCHK(hipEventCreate(&sc->ev[i][0])); HIPCHK(hipEventCreate(&sc->ev[i][1])); }
        HIPCHK(hipHostMalloc((void**)&sc->h_poll, 4 * 64, hipHostMallocDefault));
        for (int i = 0; i < 3; i++) { HIPCHK(hipStreamCreateWithFlags(&sc->xstreams[i], hipStreamNonBlocking)); HIPCHK(hipEventCreateWithFlags(&sc->ev_join[i], hipEventDisableTiming)); }
        HIPCHK(hipEventCreateWithFlags(&sc->ev_fork, hipEventDisableTiming));
        hipDeviceProp_t prop;
        HIPCHK(hipGetDeviceProperties(&prop, device));
        sc->num_cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
        return PT_OK;
    };
    if ((rc = finish()) != PT_OK) { pt_scene_destroy(sc); return rc; }
    // environment overrides of the per-scene defaults (the same settings have C-ABI setters: pt_set_mode, pt_set_drain_threshold)
    if (const char* m = getenv("PTAMD_MODE")) { const int v = atoi(m); if (v >= 0 && v <= 1) sc->mode = v; }
    if (const char* m = getenv("PTAMD_DRAIN")) sc->drain_below = atoi(m);
    if (const char* m = getenv("PTAMD_EARLY")) sc->early_below = atoi(m) > 0 ? atoi(m) : 0;      // 0 = off
    // shading schedule (pt_set_shade_rounds): one bounce per step pays when wf_shade is bound by its arithmetic rather than by the
    // stream state it moves — measured: scenes whose surface table stays in L2 (+10 % on the Cornell room, 34 triangles) while
    // millions of streams are alive; with the 69,564-triangle bunny it is neutral, and with few streams in flight it loses
    sc->shade_rounds = ((size_t)n_tris * 192 <= ((size_t)2 << 20)) ? -1 : 1;
    if (const char* m = getenv("PTAMD_TR")) { const int v = atoi(m); if (v >= -1 && v <= 1) sc->shade_rounds = v; }
    if (const char* m = getenv("PTAMD_QUERY_QUAD")) sc->query_quad = atoi(m) != 0;
    sc->dev.nodes = (const float4*)sc->d_nodes; sc->dev.quad = (const uint4*)sc->d_quad; sc->dev.tri = (const float4*)sc->d_tri;
    sc->dev.tripair = (const float4*)sc->d_tripair;
    sc->dev.leafbox = (const float4*)sc->d_leafbox; sc->dev.surf = (const float4*)sc->d_surf;
    sc->dev.lights = (const float4*)sc->d_lights; sc->dev.spheres = (const float4*)sc->d_spheres;
    sc->dev.n_quad = accel.n_quad; sc->dev.quad_depth = accel.quad_depth;
    sc->dev.core = (const float*)sc->d_core;      // nullptr: no queue order by ray class
    sc->dev.nee_prune = (emitOk && !(getenv("PTAMD_PRUNE") && atoi(getenv("PTAMD_PRUNE")) == 0)) ? 1 : 0;      // PTAMD_PRUNE=0: A/B only
    sc->dev.n_nodes = n_wide; sc->dev.n_tris = n_tris; sc->dev.n_lights = n_lights; sc->dev.n_spheres = n_spheres;
    // what a vertex update needs later: the sizes, the sphere records and the maps of the build (uploaded by the first update)
    const size_t ab[9] = {accel.wide.size() * 4, accel.quad.size() * 4, accel.tri.size() * 4, accel.tripair.size() * 4, accel.leafbox.size() * 4,
                          surf.size() * 4, lights.size() * 4, sph.size() * 4, core.size() * 4};
    memcpy(sc->array_bytes, ab, sizeof(ab));
    sc->h_spheres.swap(sph);
    PtScene::DynHost& dh = sc->dyn_host;
    dh.bn.swap(accel.bn); dh.order.swap(accel.order); dh.level_start.swap(accel.level_start); dh.wide_bn.swap(accel.wide_bn);
    dh.quad_bn.swap(accel.quad_bn); dh.leaf_range.swap(accel.leaf_range); dh.tmap.swap(accel.tmap); dh.light_prim.swap(light_prim);
    if (!core.empty()) dh.small.swap(small);
    dh.area_sum = accel.area_sum;
    sc->dyn.n_bn = (int32_t)(dh.bn.size() / 4); sc->dyn.n_wide = n_wide; sc->dyn.n_quad = accel.n_quad; sc->dyn.n_tris = n_tris;
    sc->dyn.n_leaves = accel.n_leaves; sc->dyn.n_lights = n_lights;
    *out = sc;
    return PT_OK;
}

void pt_scene_destroy(PtScene* s)
{
    if (!s) return;
    (void)hipSetDevice(s->device);
    void* p[] = {s->d_nodes, s->d_quad, s->d_tri, s->d_tripair, s->d_leafbox, s->d_surf, s->d_lights, s->d_spheres, s->d_core, s->d_unit_counter, s->d_counters, s->d_tile_list, s->d_views};
    for (void* q : p) if (q) (void)hipFree(q);
    for (void* q : s->d_dyn) if (q) (void)hipFree(q);
    for (int i = 0; i < PtScene::kEvRing; i++) for (int j = 0; j < 2; j++) if (s->ev[i][j]) (void)hipEventDestroy(s->ev[i][j]);
    if (s->h_poll) (void)hipHostFree(s->h_poll);
    for (int i = 0; i < 3; i++) { if (s->xstreams[i]) (void)hipStreamDestroy(s->xstreams[i]); if (s->ev_join[i]) (void)hipEventDestroy(s->ev_join[i]); }
    if (s->ev_fork) (void)hipEventDestroy(s->ev_fork);
    for (hipEvent_t e : s->trace_ev) (void)hipEventDestroy(e);
    delete s;
}

int32_t pt_scene_num_lights(const PtScene* s) { return s ? s->n_lights : 0; }
__attribute__((visibility("hidden"))) int ptk_scene_device(const PtScene* s) { return s ? s->device : -1; }      // for pt_comm.hip
int64_t pt_scene_device_bytes(const PtScene* s) { return s ? s->bytes : 0; }

// persistent grid of the traversal kernel: 256 CUs x 7 blocks of 4 waves = 7 waves/SIMD, what its 72 VGPRs allow
// (PTAMD_TB overrides, tuning only; measured: 1536 blocks -3 %, 1024 blocks -22 %)
static const int kTraceBlocks = (getenv("PTAMD_TB") && atoi(getenv("PTAMD_TB")) >= 1) ? (atoi(getenv("PTAMD_TB")) > 16384 ? 16384 : atoi(getenv("PTAMD_TB"))) : 1792;

// ---- geometry of the tile split --------------------------------------------------------
static int fill_params(const PtCamera* cam, const PtParams* prm, ptd::DevParams& d)
{
    if (!cam || !prm) { pt_set_error("NULL camera/params"); return PT_ERR_INVALID; }
    if (cam->W < 2 || cam->H < 2) { pt_set_error("frame %dx%d too small (W-1, H-1 divide, srcs/pathtracer.cu:35-36)", cam->W, cam->H); return PT_ERR_INVALID; }
    if (prm->spp_per_pass > 65535 || prm->max_bounce > 255 || prm->max_refract < 0 || prm->max_refract > 250) {
        pt_set_error("params out of range: spp_per_pass <= 65535, max_bounce <= 255, 0 <= max_refract <= 250");
        return PT_ERR_INVALID;
    }
    if (prm->passes < 1 || prm->spp_per_pass < 1 || prm->max_bounce < 1 || prm->world < 1 || prm->rank < 0 || prm->rank >= prm->world) {
        pt_set_error("bad params: passes=%d spp=%d max_bounce=%d rank=%d world=%d", prm->passes, prm->spp_per_pass, prm->max_bounce, prm->rank, prm->world);
        return PT_ERR_INVALID;
    }
    const long long maxseed = (long long)cam->W * cam->H * (long long)(prm->first_pass + prm->passes);
    if (maxseed > 0x7fffffffLL) { pt_set_error("offset + SampleIDX*W*H overflows int (srcs/pathtracer.cu:71)"); return PT_ERR_INVALID; }
    d.passes = prm->passes; d.spp_per_pass = prm->spp_per_pass; d.max_bounce = prm->max_bounce; d.rr_bounce = prm->rr_bounce;
    d.rr_floor = prm->rr_floor; d.max_refract = prm->max_refract; d.first_pass = prm->first_pass;
    d.rank = prm->rank; d.world = prm->world;
    d.tiles_x = (cam->W + ptd::kTile - 1) / ptd::kTile;
    d.tiles_y = (cam->H + ptd::kTile - 1) / ptd::kTile;
    d.n_tiles_total = d.tiles_x * d.tiles_y;
    d.n_tiles_local = (d.n_tiles_total + prm->world - 1) / prm->world;
    const long long units = (long long)d.n_tiles_local * prm->passes;
    if (units > 0x7fffffffLL) { pt_set_error("too many work units"); return PT_ERR_INVALID; }
    d.n_units = (int)units;
    d.unit_base = 0;
    return PT_OK;
}

// srcs/pathtracer.cu:193-198 and :35-36 — the per-launch camera constants, tan/atan2 as correctly rounded float functions
static void fill_camera(const PtCamera* cam, ptd::DevCamera& c)
{
    memcpy(c.pos, cam->pos, 12); memcpy(c.forward, cam->forward, 12); memcpy(c.up, cam->up, 12); memcpy(c.right, cam->right, 12);
    c.W = cam->W; c.H = cam->H;
    const float fovy = cam->fovy_deg * 0.01745329251994329576923690768489f;                 // glm::radians
    const float fovx = 2.f * (float)std::atan2((double)((float)std::tan((double)(fovy * 0.5f)) * cam->aspect), 1.0);
    c.tan_half_fovx = (float)std::tan((double)(fovx * 0.5f));
    c.tan_half_fovy = (float)std::tan((double)(fovy * 0.5f));
}

int64_t pt_tiles_floats(const PtCamera* cam, const PtParams* prm)
{
    ptd::DevParams d;
    if (fill_params(cam, prm, d)) return -1;
    return (int64_t)d.n_tiles_local * ptd::kTilePixels * 3;
}
// d_work of a render of d: the per-pass means of the one-kernel mode or the pipeline's buffers, whichever is larger
static int64_t work_bytes(const ptd::DevParams& d)
{
    const int64_t means = (int64_t)d.n_tiles_local * ptd::kTilePixels * 3 * 4 * d.passes;
    const int64_t wave = (int64_t)ptk_wf_work_bytes((size_t)d.n_units, kTraceBlocks);
    return means > wave ? means : wave;
}
int64_t pt_work_bytes(const PtCamera* cam, const PtParams* prm)
{
    ptd::DevParams d;
    if (fill_params(cam, prm, d)) return -1;
    return work_bytes(d);
}

static bool has_light(const PtScene* s)      // false: PT_ERR_NO_LIGHT, with the error text set
{
    if (s->n_lights < 1) pt_set_error("scene has no emissive triangle: the reference's `curand(s) %% Nl` is undefined (include/CudaUtil.cuh:235)");
    return s->n_lights >= 1;
}

// The one way into the queue-driven pipeline (pt_wavefront.hip), for an entry point that has checked its arguments, set the device and filled in
// what to render and from which pixels and cameras.  Lends the job the scene's resources and runs it — the pipeline polls the live-stream count,
// so this returns once the render has drained — then sums the passes into d_tiles.  traceEvents: record the per-launch events of
// pt_enable_trace_timing.  traceStat: the PTAMD_TSTAT diagnostics apply (wf_trace counts its trips and the lanes they serve; pt_last_counters).
static int run_job(PtScene* s, ptd::WfJob& job, bool traceEvents, bool traceStat, float* d_tiles)
{
    const int slot = s->ev_count % PtScene::kEvRing;
    job.device = s->device; job.scene = &s->dev; job.traceBlocks = kTraceBlocks;
    job.h_poll = s->h_poll; job.xstreams = s->xstreams; job.ev_fork = s->ev_fork; job.ev_join = s->ev_join;
    job.ev_begin = s->ev[slot][0]; job.ev_end = s->ev[slot][1];
    job.drainBelow = s->drain_below; job.shadeRounds = s->shade_rounds; job.earlyBelow = s->early_below;
    if (traceEvents && !s->trace_ev.empty()) { job.trace_ev = s->trace_ev.data(); job.trace_ev_triples = (int)s->trace_ev.size() / 3; }
    s->trace_ev_per = job.trace_ev_triples / ptk_wf_cohorts((size_t)job.prm.n_units);
    for (int k = 0; k < 4; k++) s->trace_ev_used[k] = 0;
    job.trace_ev_used = s->trace_ev_used;
    if (traceStat && ptk_wf_trace_stat() != 0) {
        HIPCHK(hipMemsetAsync(s->d_counters, 0, ptd::kStatBytes, job.stream));
        job.traceStat = (unsigned long long*)s->d_counters;
    }
    job.iters = &s->last_iters;
    HIPCHK(ptk_wf_render(job));
    s->ev_count++;
    HIPCHK(ptk_sum_passes(ptk_wf_staging(job.work), job.prm.passes, (long long)job.prm.n_tiles_local * ptd::kTilePixels * 3, d_tiles, job.stream));
    return PT_OK;
}

int pt_render_tiles(PtScene* s, const PtCamera* cam, const PtParams* prm, float* d_tiles, void* d_work, void* hip_stream)
{
    if (!s || !d_tiles || !d_work) { pt_set_error("pt_render_tiles: NULL argument"); return PT_ERR_INVALID; }
    if (!has_light(s)) return PT_ERR_NO_LIGHT;
    ptd::WfJob job{};
    ptd::DevParams& d = job.prm;
    int rc = fill_params(cam, prm, d);
    if (rc) return rc;
    ptd::DevCamera c;
    fill_camera(cam, c);

    hipStream_t stream = (hipStream_t)hip_stream;
    HIPCHK(hipSetDevice(s->device));
    if (s->mode == 1 && !s->count_next) {
        // the only entry point that honours pt_set_mode(0), the counting build and the PTAMD_TSTAT diagnostics
        job.work = d_work; job.stream = stream; job.cam = &c;
        return run_job(s, job, /*traceEvents=*/true, /*traceStat=*/true, d_tiles);
    }
    const int slot = s->ev_count % PtScene::kEvRing;
    HIPCHK(hipMemsetAsync(s->d_unit_counter, 0, 4, stream));
    if (s->count_next) HIPCHK(hipMemsetAsync(s->d_counters, 0, 64, stream));
    // persistent grid: 4 blocks of 4 waves per CU (16 waves/CU; register- and LDS-feasible), never more blocks than units need
    int blocks = s->num_cus * 4;
    const int need = (d.n_units + ptd::kWavesPerBlock - 1) / ptd::kWavesPerBlock;
    if (blocks > need) blocks = need;
    if (blocks < 1) blocks = 1;
    // events bracket exactly the render_units launch (the dominant kernel), on the launch stream
    HIPCHK(hipEventRecord(s->ev[slot][0], stream));
    HIPCHK(ptk_render_units(&s->dev, &c, &d, (float*)d_work, s->d_unit_counter, s->d_counters, blocks, s->count_next ? 1 : 0, stream));
    HIPCHK(hipEventRecord(s->ev[slot][1], stream));
    s->ev_count++;
    HIPCHK(ptk_sum_passes((const float*)d_work, d.passes, (long long)d.n_tiles_local * ptd::kTilePixels * 3, d_tiles, stream));
    return PT_OK;
}

// ---- a list of tiles instead of a rank's fixed share (csrc/pt_region.hip has the window helpers and the scatter) ----------------
// DevParams of a list render: a world of one whose "frame" has n_tiles tiles — the pipeline only counts units; the pixels come from the list
static int fill_list_params(const PtCamera* cam, const PtParams* prm, int32_t n_tiles, ptd::DevParams& d)
{
    const int rc = fill_params(cam, prm, d);
    if (rc) return rc;
    if (prm->rank != 0 || prm->world != 1) { pt_set_error("a tile list is rendered with rank 0 of world 1 (split a frame by making lists): rank=%d world=%d", prm->rank, prm->world); return PT_ERR_INVALID; }
    if (n_tiles < 1 || n_tiles > d.n_tiles_total) { pt_set_error("n_tiles=%d: a list holds 1 .. %d tiles of a %dx%d frame", n_tiles, d.n_tiles_total, cam->W, cam->H); return PT_ERR_INVALID; }
    d.n_tiles_local = n_tiles;
    d.n_units = n_tiles * prm->passes;      // <= the full frame's, which fill_params has bounded
    return PT_OK;
}

int64_t pt_tile_list_floats(int32_t n_tiles)
{
    if (n_tiles < 1) { pt_set_error("pt_tile_list_floats: n_tiles=%d", n_tiles); return -1; }
    return (int64_t)n_tiles * ptd::kTilePixels * 3;
}

int64_t pt_tile_list_work_bytes(const PtCamera* cam, const PtParams* prm, int32_t n_tiles)
{
    ptd::DevParams d;
    if (fill_list_params(cam, prm, n_tiles, d)) return -1;
    return work_bytes(d);
}

int pt_render_tile_list(PtScene* s, const PtCamera* cam, const PtParams* prm, const int32_t* h_tiles, int32_t n_tiles,
                        float* d_tiles, void* d_work, void* hip_stream)
{
    if (!s || !h_tiles || !d_tiles || !d_work) { pt_set_error("pt_render_tile_list: NULL argument"); return PT_ERR_INVALID; }
    ptd::WfJob job{};
    ptd::DevParams& d = job.prm;
    int rc = fill_list_params(cam, prm, n_tiles, d);
    if (rc) return rc;
    {
        std::vector<bool> seen((size_t)d.n_tiles_total, false);
        for (int32_t i = 0; i < n_tiles; i++) {
            const int32_t t = h_tiles[i];
            if (t < 0 || t >= d.n_tiles_total) { pt_set_error("pt_render_tile_list: entry %d is tile %d, the frame has tiles 0 .. %d", i, t, d.n_tiles_total - 1); return PT_ERR_INVALID; }
            if (seen[(size_t)t]) { pt_set_error("pt_render_tile_list: tile %d is listed twice (entry %d)", t, i); return PT_ERR_INVALID; }
            seen[(size_t)t] = true;
        }
    }
    if (!has_light(s)) return PT_ERR_NO_LIGHT;
    ptd::DevCamera c;
    fill_camera(cam, c);

    job.stream = (hipStream_t)hip_stream;
    HIPCHK(hipSetDevice(s->device));
    if (s->tile_list_cap < n_tiles) {
        // the previous list render on this scene has drained (one render at a time per scene), so nothing reads the old buffer
        if (s->d_tile_list) { HIPCHK(hipFree(s->d_tile_list)); s->d_tile_list = nullptr; s->tile_list_cap = 0; }
        const int64_t cap = n_tiles < 1024 ? 1024 : n_tiles;
        HIPCHK(hipMalloc((void**)&s->d_tile_list, (size_t)cap * 4));
        s->tile_list_cap = cap;
    }
    // stream-ordered before wf_init_list; the render below returns only once it has drained, so h_tiles is not read after the call
    HIPCHK(hipMemcpyAsync(s->d_tile_list, h_tiles, (size_t)n_tiles * 4, hipMemcpyHostToDevice, job.stream));
    // always the queue-driven pipeline (pt_set_mode, the counting build and the PTAMD_TSTAT diagnostics do not apply); no per-launch trace events
    job.work = d_work; job.cam = &c; job.tileList = s->d_tile_list;
    return run_job(s, job, /*traceEvents=*/false, /*traceStat=*/false, d_tiles);
}

// ---- a batch of cameras in one pipeline run -----------------------------------------------------------------------------------------
// DevParams of a batch: a world of one whose "frame" has n_views x tiles tiles (tiles_x / tiles_y / n_tiles_total stay those of one view:
// wf_init_views turns a local tile into (view, tile of the view) with them) — the pipeline only counts units.  first_pass: the
// largest of the batch, so that fill_params' seed limit covers every view (W and H are shared).
static int fill_views_params(const PtCamera* cam0, const PtParams* prm, int32_t n_views, int32_t max_first_pass, ptd::DevParams& d)
{
    if (!cam0 || !prm) { pt_set_error("NULL camera/params"); return PT_ERR_INVALID; }
    if (n_views < 1) { pt_set_error("n_views=%d: a batch holds at least one view", n_views); return PT_ERR_INVALID; }
    PtParams p = *prm; p.first_pass = max_first_pass;
    const int rc = fill_params(cam0, &p, d);
    if (rc) return rc;
    if (prm->rank != 0 || prm->world != 1) { pt_set_error("a batch of views is rendered with rank 0 of world 1: rank=%d world=%d", prm->rank, prm->world); return PT_ERR_INVALID; }
    // what a single frame of that many tiles may have: fill_params' own limit on the units, and 64 streams per unit below 2^31
    // (bit 31 of a ray-queue entry is the resume flag)
    const long long units = (long long)n_views * d.n_tiles_total * prm->passes;
    if (units > 0x7fffffffLL || units * 64 >= (1LL << 31)) {
        pt_set_error("%d views x %d tiles x %d passes: too many work units for one pipeline run (64 x units must stay below 2^31)", n_views, d.n_tiles_total, prm->passes);
        return PT_ERR_INVALID;
    }
    d.n_tiles_local = n_views * d.n_tiles_total;
    d.n_units = (int)units;
    return PT_OK;
}

int64_t pt_views_floats(const PtCamera* cam0, int32_t n_views)
{
    PtParams p; pt_params_default(&p); p.passes = 1; p.first_pass = 0;
    ptd::DevParams d;
    if (n_views < 1) { pt_set_error("pt_views_floats: n_views=%d", n_views); return -1; }
    if (fill_params(cam0, &p, d)) return -1;
    return (int64_t)n_views * d.n_tiles_total * ptd::kTilePixels * 3;
}

int64_t pt_views_work_bytes(const PtCamera* cam0, const PtParams* prm, int32_t n_views)
{
    ptd::DevParams d;
    if (fill_views_params(cam0, prm, n_views, prm ? prm->first_pass : 0, d)) return -1;
    return work_bytes(d);
}

// every host-side check of a batch (include/pt_api.h), before any HIP call
static int views_args(const PtCamera* h_cams, int32_t n_views, const PtParams* prm, const int32_t* h_first_pass, ptd::DevParams& d)
{
    if (!h_cams || !prm) { pt_set_error("pt_render_views: NULL argument"); return PT_ERR_INVALID; }
    if (n_views < 1) { pt_set_error("pt_render_views: n_views=%d", n_views); return PT_ERR_INVALID; }
    int32_t maxFirst = prm->first_pass;
    for (int32_t v = 0; v < n_views; v++) {
        if (h_cams[v].W != h_cams[0].W || h_cams[v].H != h_cams[0].H) {
            pt_set_error("pt_render_views: view %d is %dx%d, view 0 is %dx%d (all views of a batch share W and H)", v, h_cams[v].W, h_cams[v].H, h_cams[0].W, h_cams[0].H);
            return PT_ERR_INVALID;
        }
        if (h_first_pass) {
            if (h_first_pass[v] < 0) { pt_set_error("pt_render_views: first_pass of view %d is %d", v, h_first_pass[v]); return PT_ERR_INVALID; }
            if (v == 0 || h_first_pass[v] > maxFirst) maxFirst = h_first_pass[v];
        }
    }
    return fill_views_params(&h_cams[0], prm, n_views, maxFirst, d);
}

int pt_render_views(PtScene* s, const PtCamera* h_cams, int32_t n_views, const PtParams* prm, const int32_t* h_first_pass,
                    float* d_tiles, void* d_work, void* hip_stream)
{
    if (!s || !d_tiles || !d_work) { pt_set_error("pt_render_views: NULL argument"); return PT_ERR_INVALID; }
    ptd::WfJob job{};
    const int rc = views_args(h_cams, n_views, prm, h_first_pass, job.prm);
    if (rc) return rc;
    if (!has_light(s)) return PT_ERR_NO_LIGHT;
    job.stream = (hipStream_t)hip_stream;
    HIPCHK(hipSetDevice(s->device));
    if (s->view_cap < n_views) {
        // the previous batch on this scene has drained (one render at a time per scene), so nothing reads the old buffer
        if (s->d_views) { HIPCHK(hipFree(s->d_views)); s->d_views = nullptr; s->view_cap = 0; }
        const int64_t cap = n_views < 64 ? 64 : n_views;
        HIPCHK(hipMalloc(&s->d_views, (size_t)cap * (16 + sizeof(ptd::DevCamera) + 4)));
        s->view_cap = cap;
    }
    // origins | cameras | first passes, each n_views long, packed for one copy (16-byte entries first: every part stays aligned)
    const size_t offCam = (size_t)n_views * 16, offFirst = offCam + (size_t)n_views * sizeof(ptd::DevCamera), total = offFirst + (size_t)n_views * 4;
    s->h_views.resize(total);
    for (int32_t v = 0; v < n_views; v++) {
        ptd::DevCamera c;
        fill_camera(&h_cams[v], c);
        const float org[4] = {c.pos[0], c.pos[1], c.pos[2], 0.f};
        const int32_t first = h_first_pass ? h_first_pass[v] : prm->first_pass;
        memcpy(s->h_views.data() + (size_t)v * 16, org, 16);
        memcpy(s->h_views.data() + offCam + (size_t)v * sizeof(ptd::DevCamera), &c, sizeof(c));
        memcpy(s->h_views.data() + offFirst + (size_t)v * 4, &first, 4);
    }
    // stream-ordered before wf_init_views; the render below returns only once it has drained, so the callers' arrays are not read after the call
    HIPCHK(hipMemcpyAsync(s->d_views, s->h_views.data(), total, hipMemcpyHostToDevice, job.stream));
    const char* dv = (const char*)s->d_views;
    // always the queue-driven pipeline (pt_set_mode, the counting build and the PTAMD_TSTAT diagnostics do not apply); a batch passes no single camera
    job.work = d_work;
    job.viewOrg = (const float4*)dv; job.viewCams = (const ptd::DevCamera*)(dv + offCam); job.viewFirstPass = (const int32_t*)(dv + offFirst);
    return run_job(s, job, /*traceEvents=*/true, /*traceStat=*/false, d_tiles);
}

int pt_render_views_host(PtScene* s, const PtCamera* h_cams, int32_t n_views, const PtParams* prm, const int32_t* h_first_pass, float* h_rgb)
{
    if (!s || !h_rgb) { pt_set_error("pt_render_views_host: NULL argument"); return PT_ERR_INVALID; }
    ptd::DevParams d;
    int rc = views_args(h_cams, n_views, prm, h_first_pass, d);
    if (rc) return rc;
    const int64_t nt = pt_views_floats(&h_cams[0], n_views), wb = pt_views_work_bytes(&h_cams[0], prm, n_views);
    if (nt < 0 || wb < 0) return PT_ERR_INVALID;
    const size_t perView = (size_t)nt / (size_t)n_views, frame = (size_t)h_cams[0].W * h_cams[0].H * 3;
    HIPCHK(hipSetDevice(s->device));
    float *d_tiles = nullptr, *d_frames = nullptr; void* d_work = nullptr;
    auto body = [&]() -> int {
        HIPCHK(hipMalloc((void**)&d_tiles, (size_t)nt * 4));
        HIPCHK(hipMalloc(&d_work, (size_t)wb));
        HIPCHK(hipMalloc((void**)&d_frames, frame * 4 * (size_t)n_views));
        int r = pt_render_views(s, h_cams, n_views, prm, h_first_pass, d_tiles, d_work, nullptr);
        for (int32_t v = 0; v < n_views && !r; v++) r = pt_untile(d_tiles + (size_t)v * perView, &h_cams[v], 1, d_frames + (size_t)v * frame, nullptr);
        if (!r) HIPCHK(hipMemcpy(h_rgb, d_frames, frame * 4 * (size_t)n_views, hipMemcpyDeviceToHost));
        return r;
    };
    rc = body();
    (void)hipFree(d_tiles); (void)hipFree(d_work); (void)hipFree(d_frames);
    return rc;
}

int pt_untile(const float* d_gathered, const PtCamera* cam, int32_t world, float* d_frame_rgb, void* hip_stream)
{
    if (!d_gathered || !cam || !d_frame_rgb || world < 1) { pt_set_error("pt_untile: bad argument"); return PT_ERR_INVALID; }
    const int tiles_x = (cam->W + ptd::kTile - 1) / ptd::kTile, tiles_y = (cam->H + ptd::kTile - 1) / ptd::kTile;
    const int n_total = tiles_x * tiles_y;
    const long long per_rank = (long long)((n_total + world - 1) / world) * ptd::kTilePixels * 3;
    HIPCHK(ptk_untile(d_gathered, cam->W, cam->H, tiles_x, n_total, world, per_rank, d_frame_rgb, (hipStream_t)hip_stream));
    return PT_OK;
}

int pt_render(PtScene* s, const PtCamera* cam, const PtParams* prm, float* h_accum_rgb)
{
    if (!s || !h_accum_rgb || !prm) { pt_set_error("pt_render: NULL argument"); return PT_ERR_INVALID; }
    PtParams p = *prm; p.rank = 0; p.world = 1;
    const int64_t nt = pt_tiles_floats(cam, &p), wb = pt_work_bytes(cam, &p);
    if (nt < 0 || wb < 0) return PT_ERR_INVALID;
    HIPCHK(hipSetDevice(s->device));
    float *d_tiles = nullptr, *d_frame = nullptr; void* d_work = nullptr;
    auto body = [&]() -> int {
        HIPCHK(hipMalloc((void**)&d_tiles, (size_t)nt * 4));
        HIPCHK(hipMalloc(&d_work, (size_t)wb));
        HIPCHK(hipMalloc((void**)&d_frame, (size_t)cam->W * cam->H * 12));
        int r = pt_render_tiles(s, cam, &p, d_tiles, d_work, nullptr);
        if (!r) r = pt_untile(d_tiles, cam, 1, d_frame, nullptr);
        if (!r) HIPCHK(hipMemcpy(h_accum_rgb, d_frame, (size_t)cam->W * cam->H * 12, hipMemcpyDeviceToHost));
        return r;
    };
    const int rc = body();
    (void)hipFree(d_tiles); (void)hipFree(d_work); (void)hipFree(d_frame);
    return rc;
}

int pt_last_render_ms(PtScene* s, float* ms)
{
    if (!s || !ms || s->ev_count < 1) { pt_set_error("pt_last_render_ms: nothing rendered yet"); return PT_ERR_INVALID; }
    const int slot = (s->ev_count - 1) % PtScene::kEvRing;
    HIPCHK(hipSetDevice(s->device));
    HIPCHK(hipEventSynchronize(s->ev[slot][1]));
    HIPCHK(hipEventElapsedTime(ms, s->ev[slot][0], s->ev[slot][1]));
    return PT_OK;
}

int pt_render_timings(PtScene* s, float* ms_out, int32_t cap, int32_t reset)
{
    if (!s) { pt_set_error("pt_render_timings: NULL scene"); return PT_ERR_INVALID; }
    int n = s->ev_count < PtScene::kEvRing ? s->ev_count : PtScene::kEvRing;
    if (n > cap) n = cap;
    HIPCHK(hipSetDevice(s->device));
    for (int i = 0; i < n; i++) {
        const int slot = (s->ev_count - n + i) % PtScene::kEvRing;
        HIPCHK(hipEventSynchronize(s->ev[slot][1]));
        HIPCHK(hipEventElapsedTime(&ms_out[i], s->ev[slot][0], s->ev[slot][1]));
    }
    if (reset) s->ev_count = 0;
    return n;
}

int pt_last_counters(PtScene* s, int64_t* out8)
{
    if (!s || !out8) { pt_set_error("pt_last_counters: NULL"); return PT_ERR_INVALID; }
    HIPCHK(hipSetDevice(s->device));
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(out8, s->d_counters, 64, hipMemcpyDeviceToHost));
    return PT_OK;
}
// Record a HIP event pair around each of the first `max_launches` wf_trace launches of every
// following render (0 turns it off); pt_trace_timing then reports their summed duration.
PT_API int pt_enable_trace_timing(PtScene* s, int32_t max_launches)
{
    if (!s || max_launches < 0 || max_launches > (1 << 20)) { pt_set_error("pt_enable_trace_timing: bad argument"); return PT_ERR_INVALID; }
    HIPCHK(hipSetDevice(s->device));
    for (hipEvent_t e : s->trace_ev) (void)hipEventDestroy(e);
    s->trace_ev.assign((size_t)max_launches * 3, nullptr);
    for (auto& e : s->trace_ev) HIPCHK(hipEventCreate(&e));
    for (int k = 0; k < 4; k++) s->trace_ev_used[k] = 0;
    return PT_OK;
}
static int kernel_timing(PtScene* s, int first, double* sum_ms, int32_t* launches, double* max_ms)
{
    if (!s || !sum_ms || !launches) { pt_set_error("pt_trace_timing / pt_shade_timing: NULL"); return PT_ERR_INVALID; }
    HIPCHK(hipSetDevice(s->device));
    double sum = 0, mx = 0;
    int total = 0;
    for (int c = 0; c < 4; c++)
        for (int i = 0; i < s->trace_ev_used[c]; i++) {
            const size_t k = ((size_t)c * s->trace_ev_per + i) * 3 + (size_t)first;
            float ms = 0.f;
            HIPCHK(hipEventSynchronize(s->trace_ev[k + 1]));
            HIPCHK(hipEventElapsedTime(&ms, s->trace_ev[k], s->trace_ev[k + 1]));
            sum += ms; if (ms > mx) mx = ms;
            total++;
        }
    *sum_ms = sum; *launches = total; if (max_ms) *max_ms = mx;
    return PT_OK;
}
PT_API int pt_trace_timing(PtScene* s, double* sum_ms, int32_t* launches, double* max_ms) { return kernel_timing(s, 0, sum_ms, launches, max_ms); }
PT_API int pt_shade_timing(PtScene* s, double* sum_ms, int32_t* launches, double* max_ms) { return kernel_timing(s, 1, sum_ms, launches, max_ms); }
PT_API int pt_set_mode(PtScene* s, int32_t mode) { if (!s || mode < 0 || mode > 1) { pt_set_error("pt_set_mode: mode must be 0 or 1"); return PT_ERR_INVALID; } s->mode = mode; return PT_OK; }
PT_API int pt_last_iterations(PtScene* s) { return s ? s->last_iters : -1; }
PT_API int pt_set_drain_threshold(PtScene* s, int32_t live_streams)
{
    if (!s || live_streams < 0) { pt_set_error("pt_set_drain_threshold: bad argument"); return PT_ERR_INVALID; }
    s->drain_below = live_streams;
    return PT_OK;
}
PT_API int pt_set_early_shade(PtScene* s, int32_t live_streams)
{
    if (!s || live_streams < 0) { pt_set_error("pt_set_early_shade: bad argument"); return PT_ERR_INVALID; }
    s->early_below = live_streams;
    return PT_OK;
}
PT_API int pt_set_shade_rounds(PtScene* s, int32_t mode)
{
    if (!s || mode < -1 || mode > 1) { pt_set_error("pt_set_shade_rounds: mode must be -1, 0 or 1"); return PT_ERR_INVALID; }
    s->shade_rounds = mode;
    return PT_OK;
}
// Ask the next pt_render_tiles on this scene to run the counting build of the kernel.
int pt_dbg_trace_timeline(PtScene* s, int64_t* out3n, int32_t n_launches)
{
    using namespace ptd;
    if (!s || !out3n || (n_launches < -kStatLaunches && (n_launches > -3000 || n_launches < -3005)) || n_launches > kStatLaunches) { pt_set_error("pt_dbg_trace_timeline: bad arguments"); return PT_ERR_INVALID; }
    HIPCHK(hipSetDevice(s->device));
    HIPCHK(hipDeviceSynchronize());
    auto read = [&](void* dst, size_t byteOff, size_t bytes) { return hipMemcpy(dst, (const char*)s->d_counters + byteOff, bytes, hipMemcpyDeviceToHost); };
    const size_t waveOff = (size_t)kStatWords * 8, logOff = waveOff + (size_t)kStatWaves * 64;
    const struct { int code; size_t byteOff, bytes; } section[] = {
        {-3005, kStatStripeOff, (size_t)kStatLaunches * kStatStripes * 24},      // PTAMD_TSTAT=2: the raw timeline stripes, kStatLaunches launches x kStatStripes x 3 int64 (maxima of ~start, ~dry, end per stripe of workgroups)
        {-3004, logOff, (size_t)kStatLogWaves * kStatLogTrips * 4},              // PTAMD_TSTAT=2 + PTAMD_TDUMP=launch: the per-trip log (kStatLogWaves x kStatLogTrips uint32)
        {-3003, waveOff, logOff - waveOff},                                      // PTAMD_TSTAT=2 + PTAMD_TDUMP=launch: 8 x int64 per wave (kStatWaves)
        {-3002, (size_t)kStatClocks * 8, 5 * 8},                                 // shader clocks per section of wf_trace's loop, summed over waves (5 x int64: refill, vote, node step, triangle step, epilogue), PTAMD_TSTAT=1
        {-3001, (size_t)kStatDepthHist * 8, 32 * 8},                             // histogram of the stack depth after each node step (32 x int64), PTAMD_TSTAT=1
        {-3000, (size_t)kStatStepHist * 8, 64 * 8},                              // the histogram of node steps per ray (64 x int64: bins of 4 steps), PTAMD_TSTAT=1
        {0, (size_t)kStatLifeHist * 8, 32 * 8},                                  // the 32-bin histogram of wave lifetimes (32 us bins)
    };
    for (const auto& q : section)
        if (q.code == n_launches) { HIPCHK(read(out3n, q.byteOff, q.bytes)); return PT_OK; }
    if (n_launches < 0) { HIPCHK(read(out3n, (size_t)kStatLaunchRays * 8, (size_t)(-n_launches) * 8)); return PT_OK; }      // -n: the ray count of each of the first n launches (n x int64)
    if (ptk_wf_trace_stat() == 2) {
        // the timestamp-only build keeps kStatStripes copies of every launch's three words (maxima of ~start, ~dry, end)
        std::vector<unsigned long long> raw((size_t)n_launches * kStatStripes * 3);
        HIPCHK(read(raw.data(), kStatStripeOff, raw.size() * 8));
        for (int l = 0; l < n_launches; l++)
            for (int k = 0; k < 3; k++) {
                unsigned long long m = 0;
                for (int st = 0; st < kStatStripes; st++) { const unsigned long long v = raw[((size_t)l * kStatStripes + st) * 3 + k]; if (v > m) m = v; }
                out3n[(size_t)l * 3 + k] = (int64_t)m;
            }
    } else
    HIPCHK(read(out3n, (size_t)kStatTimeline * 8, (size_t)n_launches * 24));
    return PT_OK;
}

PT_API int pt_enable_counters(PtScene* s, int32_t on) { if (!s) return PT_ERR_INVALID; s->count_next = on != 0; return PT_OK; }

// ---- first-hit feature buffers and the denoiser (pt_denoise.hip) --------------------------
static const int64_t kMaxPixels = (int64_t)1 << 28;      // keeps every per-pixel float offset (x 8) inside int64 and the pixel index inside int

static int aov_args(const PtCamera* cam, const PtParams* prm)
{
    if (!cam || !prm) { pt_set_error("NULL camera/params"); return PT_ERR_INVALID; }
    if (cam->W < 2 || cam->H < 2 || (int64_t)cam->W * cam->H > kMaxPixels) { pt_set_error("frame %dx%d out of range", cam->W, cam->H); return PT_ERR_INVALID; }
    if (prm->passes < 1 || prm->first_pass < 0) { pt_set_error("bad params: passes=%d first_pass=%d", prm->passes, prm->first_pass); return PT_ERR_INVALID; }
    if ((long long)cam->W * cam->H * (long long)(prm->first_pass + prm->passes) > 0x7fffffffLL) {
        pt_set_error("offset + SampleIDX*W*H overflows int (srcs/pathtracer.cu:71)");
        return PT_ERR_INVALID;
    }
    return PT_OK;
}

int64_t pt_aov_floats(const PtCamera* cam)
{
    if (!cam || cam->W < 2 || cam->H < 2 || (int64_t)cam->W * cam->H > kMaxPixels) { pt_set_error("pt_aov_floats: bad camera"); return -1; }
    return (int64_t)cam->W * cam->H * 8;
}

int pt_render_aov(PtScene* s, const PtCamera* cam, const PtParams* prm, float* d_aov, int32_t* d_prim, void* hip_stream)
{
    if (!s || !d_aov) { pt_set_error("pt_render_aov: NULL argument"); return PT_ERR_INVALID; }
    if ((uintptr_t)d_aov % 16) { pt_set_error("pt_render_aov: d_aov is not 16-byte aligned"); return PT_ERR_INVALID; }
    int rc = aov_args(cam, prm);
    if (rc) return rc;
    ptd::DevCamera c;
    fill_camera(cam, c);
    HIPCHK(hipSetDevice(s->device));
    HIPCHK(ptk_aov(&s->dev, &c, prm->first_pass, prm->passes, d_aov, d_prim, (hipStream_t)hip_stream));
    return PT_OK;
}

int pt_aov(PtScene* s, const PtCamera* cam, const PtParams* prm, float* h_aov, int32_t* h_prim)
{
    if (!s || !h_aov) { pt_set_error("pt_aov: NULL argument"); return PT_ERR_INVALID; }
    int rc = aov_args(cam, prm);
    if (rc) return rc;
    const size_t n = (size_t)cam->W * cam->H;
    HIPCHK(hipSetDevice(s->device));
    float* d_aov = nullptr; int32_t* d_prim = nullptr;
    auto body = [&]() -> int {
        HIPCHK(hipMalloc((void**)&d_aov, n * 32));
        if (h_prim) HIPCHK(hipMalloc((void**)&d_prim, n * 4));
        int r = pt_render_aov(s, cam, prm, d_aov, d_prim, nullptr);
        if (r) return r;
        HIPCHK(hipMemcpy(h_aov, d_aov, n * 32, hipMemcpyDeviceToHost));
        if (h_prim) HIPCHK(hipMemcpy(h_prim, d_prim, n * 4, hipMemcpyDeviceToHost));
        return PT_OK;
    };
    rc = body();
    (void)hipFree(d_aov); (void)hipFree(d_prim);
    return rc;
}

int64_t pt_denoise_work_bytes(int32_t W, int32_t H)
{
    if (W < 2 || H < 2 || (int64_t)W * H > kMaxPixels) { pt_set_error("pt_denoise_work_bytes: frame %dx%d out of range", W, H); return -1; }
    return (int64_t)W * H * 48;
}

static bool overlaps(const void* a, size_t na, const void* b, size_t nb)
{
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + nb && y < x + na;
}

static int denoise_args(const void* rgb, const void* aov, int32_t W, int32_t H, int32_t sample_cnt, const PtDenoiseParams* p,
                        const void* out, const void* work, bool device)
{
    if (!rgb || !aov || !p || !out || (device && !work)) { pt_set_error("pt_denoise: NULL argument"); return PT_ERR_INVALID; }
    if (W < 2 || H < 2 || (int64_t)W * H > kMaxPixels) { pt_set_error("pt_denoise: frame %dx%d out of range", W, H); return PT_ERR_INVALID; }
    if (sample_cnt <= 0) { pt_set_error("pt_denoise: sample_cnt %d <= 0", sample_cnt); return PT_ERR_INVALID; }
    if (p->iterations < 0 || p->iterations > 12) { pt_set_error("pt_denoise: iterations %d outside 0..12", p->iterations); return PT_ERR_INVALID; }
    if (!(p->sigma_color > 0.f) || !(p->sigma_normal > 0.f) || !(p->sigma_depth > 0.f) ||
        !std::isfinite(p->sigma_color) || !std::isfinite(p->sigma_normal) || !std::isfinite(p->sigma_depth)) {
        pt_set_error("pt_denoise: sigmas must be finite and > 0"); return PT_ERR_INVALID;
    }
    const size_t n = (size_t)W * H;
    if (overlaps(out, n * 12, rgb, n * 12) || overlaps(out, n * 12, aov, n * 32) || (work && overlaps(out, n * 12, work, n * 48))) {
        pt_set_error("pt_denoise: the output overlaps an input or the work buffer"); return PT_ERR_INVALID;
    }
    if (device && (((uintptr_t)aov % 16) || ((uintptr_t)work % 16) || overlaps(work, n * 48, rgb, n * 12) || overlaps(work, n * 48, aov, n * 32))) {
        pt_set_error("pt_denoise: d_aov / d_work not 16-byte aligned, or d_work overlaps an input"); return PT_ERR_INVALID;
    }
    return PT_OK;
}

int pt_denoise(const float* d_rgb, const float* d_aov, int32_t W, int32_t H, int32_t sample_cnt, const PtDenoiseParams* p,
               float* d_out, void* d_work, void* hip_stream)
{
    const int rc = denoise_args(d_rgb, d_aov, W, H, sample_cnt, p, d_out, d_work, true);
    if (rc) return rc;
    const hipStream_t stream = (hipStream_t)hip_stream;
    if (p->iterations == 0) { HIPCHK(hipMemcpyAsync(d_out, d_rgb, (size_t)W * H * 12, hipMemcpyDeviceToDevice, stream)); return PT_OK; }
    HIPCHK(ptk_denoise(d_rgb, d_aov, W, H, sample_cnt, p->iterations, p->sigma_color, p->sigma_normal, p->sigma_depth,
                       p->demodulate ? 1 : 0, d_out, d_work, stream));
    return PT_OK;
}

int pt_denoise_host(int32_t device, const float* h_rgb, const float* h_aov, int32_t W, int32_t H, int32_t sample_cnt,
                    const PtDenoiseParams* p, float* h_out)
{
    int rc = denoise_args(h_rgb, h_aov, W, H, sample_cnt, p, h_out, nullptr, false);
    if (rc) return rc;
    const size_t n = (size_t)W * H;
    HIPCHK(hipSetDevice(device));
    char* d = nullptr;      // one allocation: rgb | aov | out | work
    auto body = [&]() -> int {
        HIPCHK(hipMalloc((void**)&d, n * (12 + 32 + 12 + 48) + 64));
        float* d_rgb = (float*)d;
        float* d_aov = (float*)(d + ((n * 12 + 15) & ~(size_t)15));
        float* d_out = (float*)((char*)d_aov + n * 32);
        void* d_work = (char*)d_aov + ((n * 44 + 15) & ~(size_t)15);
        HIPCHK(hipMemcpy(d_rgb, h_rgb, n * 12, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(d_aov, h_aov, n * 32, hipMemcpyHostToDevice));
        int r = pt_denoise(d_rgb, d_aov, W, H, sample_cnt, p, d_out, d_work, nullptr);
        if (r) return r;
        HIPCHK(hipMemcpy(h_out, d_out, n * 12, hipMemcpyDeviceToHost));
        return PT_OK;
    };
    rc = body();
    (void)hipFree(d);
    return rc;
}

// ---- moments over passes, error estimate, render-to-target (pt_stats.hip) -----------------
int pt_accumulate_passes(const void* d_work, const PtCamera* cam, const PtParams* prm, int32_t n_before, float* d_sum, float* d_m2,
                         void* hip_stream)
{
    if (!d_work || !d_sum || !d_m2) { pt_set_error("pt_accumulate_passes: NULL argument"); return PT_ERR_INVALID; }
    if (n_before < 0 || (prm && (long long)n_before + prm->passes > 0x7fffffffLL)) { pt_set_error("pt_accumulate_passes: bad n_before %d", n_before); return PT_ERR_INVALID; }
    ptd::DevParams d;
    const int rc = fill_params(cam, prm, d);
    if (rc) return rc;
    const long long perPass = (long long)d.n_tiles_local * ptd::kTilePixels * 3;
    // both render modes leave the per-pass means at the start of the work buffer (pt_render_tiles: what sum_passes reads)
    HIPCHK(ptk_stats_fold(ptk_wf_staging(const_cast<void*>(d_work)), d.passes, perPass, n_before, d_sum, d_m2, (hipStream_t)hip_stream));
    return PT_OK;
}

int pt_variance(const float* d_m2, int64_t n_floats, int32_t n_passes, float* d_var, void* hip_stream)
{
    if (!d_m2 || !d_var || n_floats < 1 || n_passes < 2) { pt_set_error("pt_variance: NULL buffer, n_floats < 1 or n_passes < 2"); return PT_ERR_INVALID; }
    HIPCHK(ptk_stats_variance(d_m2, n_floats, n_passes, d_var, (hipStream_t)hip_stream));
    return PT_OK;
}

int64_t pt_error_scratch_bytes(int64_t n_floats)
{
    if (n_floats < 1) { pt_set_error("pt_error_scratch_bytes: n_floats < 1"); return -1; }
    const int64_t nb = (n_floats + 3071) / 3072;
    return (nb > 1024 ? 1024 : nb) * ptk_stats_partial_bytes();
}

int pt_error_estimate(const float* d_sum, const float* d_m2, const PtCamera* cam, const PtParams* prm, int32_t n_passes,
                      void* d_scratch, PtErrorEstimate* h_out, void* hip_stream)
{
    if (!d_sum || !d_m2 || !d_scratch || !h_out) { pt_set_error("pt_error_estimate: NULL argument"); return PT_ERR_INVALID; }
    if (n_passes < 2) { pt_set_error("pt_error_estimate: n_passes %d < 2", n_passes); return PT_ERR_INVALID; }
    if (!cam || !prm) { pt_set_error("NULL camera/params"); return PT_ERR_INVALID; }
    PtParams p = *prm; p.passes = 1; p.first_pass = 0;      // only the geometry of the split is read
    ptd::DevParams d;
    const int rc = fill_params(cam, &p, d);
    if (rc) return rc;
    const long long n = (long long)d.n_tiles_local * ptd::kTilePixels * 3;
    const hipStream_t stream = (hipStream_t)hip_stream;
    HIPCHK(ptk_stats_estimate(d_sum, d_m2, n, n_passes, cam->W, cam->H, d.tiles_x, d.n_tiles_total, d.rank, d.world, d_scratch, stream));
    struct Partial { double var, s2, se; long long pixels, skipped; };
    std::vector<Partial> part((size_t)ptk_stats_blocks(n));
    if ((int)sizeof(Partial) != ptk_stats_partial_bytes()) { pt_set_error("pt_error_estimate: partial layout mismatch"); return PT_ERR_INVALID; }
    HIPCHK(hipMemcpyAsync(part.data(), d_scratch, part.size() * sizeof(Partial), hipMemcpyDeviceToHost, stream));
    HIPCHK(hipStreamSynchronize(stream));
    double var = 0.0, s2 = 0.0, se = 0.0; long long pixels = 0, skipped = 0;
    for (const Partial& q : part) { var += q.var; s2 += q.s2; se += q.se; pixels += q.pixels; skipped += q.skipped; }      // block order
    h_out->rel_rms = std::sqrt(var / s2);
    h_out->mean_rel_se = se / (double)pixels;
    h_out->pixels = pixels; h_out->skipped = skipped;
    return PT_OK;
}

int pt_render_converge(PtScene* s, const PtCamera* cam, const PtParams* prm, double target_rel_rms, int32_t max_passes,
                       float* h_accum_rgb, float* h_var_rgb, int32_t* passes_done, PtErrorEstimate* est)
{
    if (!s || !prm || !h_accum_rgb || !passes_done || !est) { pt_set_error("pt_render_converge: NULL argument"); return PT_ERR_INVALID; }
    if (max_passes < 2 || !(target_rel_rms >= 0.0)) { pt_set_error("pt_render_converge: max_passes %d < 2 or target not >= 0", max_passes); return PT_ERR_INVALID; }
    PtParams p = *prm; p.rank = 0; p.world = 1;
    if (p.passes < 1) { pt_set_error("pt_render_converge: batch of %d passes", p.passes); return PT_ERR_INVALID; }
    if (p.passes > max_passes) p.passes = max_passes;
    const int batch = p.passes;
    const int64_t nt = pt_tiles_floats(cam, &p);
    int64_t wb = pt_work_bytes(cam, &p);
    PtParams all = p; all.passes = max_passes;              // the seed limit for the last pass that may be rendered
    if (nt < 0 || wb < 0 || pt_tiles_floats(cam, &all) < 0) return PT_ERR_INVALID;
    if (max_passes % batch) {                               // the shortened last batch
        PtParams q = p; q.passes = max_passes % batch;
        const int64_t w2 = pt_work_bytes(cam, &q);
        if (w2 < 0) return PT_ERR_INVALID;
        if (w2 > wb) wb = w2;
    }
    HIPCHK(hipSetDevice(s->device));
    float *d_tiles = nullptr, *d_sum = nullptr, *d_m2 = nullptr, *d_frame = nullptr; void *d_work = nullptr, *d_scratch = nullptr;
    const size_t frameBytes = (size_t)cam->W * cam->H * 12;
    auto body = [&]() -> int {
        HIPCHK(hipMalloc((void**)&d_tiles, (size_t)nt * 4));
        HIPCHK(hipMalloc((void**)&d_sum, (size_t)nt * 4));
        HIPCHK(hipMalloc((void**)&d_m2, (size_t)nt * 4));
        HIPCHK(hipMalloc(&d_work, (size_t)wb));
        HIPCHK(hipMalloc(&d_scratch, (size_t)pt_error_scratch_bytes(nt)));
        HIPCHK(hipMalloc((void**)&d_frame, frameBytes));
        int done = 0;
        while (done < max_passes) {
            p.first_pass = prm->first_pass + done;
            p.passes = max_passes - done < batch ? max_passes - done : batch;
            int r = pt_render_tiles(s, cam, &p, d_tiles, d_work, nullptr);
            if (!r) r = pt_accumulate_passes(d_work, cam, &p, done, d_sum, d_m2, nullptr);
            if (r) return r;
            done += p.passes;
            if (done < 2) continue;
            r = pt_error_estimate(d_sum, d_m2, cam, &p, done, d_scratch, est, nullptr);
            if (r) return r;
            if (est->rel_rms <= target_rel_rms) break;
        }
        *passes_done = done;
        int r = pt_untile(d_sum, cam, 1, d_frame, nullptr);
        if (r) return r;
        HIPCHK(hipMemcpy(h_accum_rgb, d_frame, frameBytes, hipMemcpyDeviceToHost));
        if (h_var_rgb) {
            r = pt_variance(d_m2, nt, done, d_tiles, nullptr);      // d_tiles is free by now
            if (!r) r = pt_untile(d_tiles, cam, 1, d_frame, nullptr);
            if (r) return r;
            HIPCHK(hipMemcpy(h_var_rgb, d_frame, frameBytes, hipMemcpyDeviceToHost));
        }
        return PT_OK;
    };
    const int rc = body();
    (void)hipFree(d_tiles); (void)hipFree(d_sum); (void)hipFree(d_m2); (void)hipFree(d_work); (void)hipFree(d_scratch); (void)hipFree(d_frame);
    return rc;
}

// ---- dynamic geometry (csrc/pt_dynamic.hip) ----------------------------------------------------------------------------------
// First update of a scene: the maps of the build go to the device and the scratch is allocated; the host copies are dropped.
static int dyn_prepare(PtScene* s)
{
    if (s->dyn_ready) return PT_OK;
    PtScene::DynHost& h = s->dyn_host;
    ptd::DynScene& d = s->dyn;
    int k = 0, rc;
    const int64_t bytes_before = s->bytes;
    auto up = [&](const void* src, size_t bytes, const void** dst) -> int {
        if ((rc = upload(&s->d_dyn[k], src, bytes, s->bytes)) != PT_OK) return rc;
        *dst = s->d_dyn[k++];
        return PT_OK;
    };
    auto scratch = [&](size_t bytes, void** dst) -> int {
        HIPCHK(hipMalloc(&s->d_dyn[k], bytes));
        s->bytes += (int64_t)bytes;
        *dst = s->d_dyn[k++];
        return PT_OK;
    };
    const size_t area_blocks = ((size_t)d.n_bn + kAreaBlock - 1) / kAreaBlock;
    if ((rc = up(h.bn.data(), h.bn.size() * 4, (const void**)&d.bn)) || (rc = up(h.order.data(), h.order.size() * 4, (const void**)&d.order)) ||
        (rc = up(h.wide_bn.data(), h.wide_bn.size() * 4, (const void**)&d.wide_bn)) || (rc = up(h.quad_bn.data(), h.quad_bn.size() * 4, (const void**)&d.quad_bn)) ||
        (rc = up(h.leaf_range.data(), h.leaf_range.size() * 4, (const void**)&d.leaf_range)) || (rc = up(h.tmap.data(), h.tmap.size() * 4, (const void**)&d.tmap)) ||
        (rc = up(h.light_prim.data(), h.light_prim.size() * 4, (const void**)&d.light_prim)) ||
        (!h.small.empty() && (rc = up(h.small.data(), h.small.size(), (const void**)&d.small))) ||
        (rc = scratch((size_t)d.n_bn * 32, (void**)&d.bbox)) || (rc = scratch(16, (void**)&d.maxabs)) ||
        (rc = scratch((size_t)ptd::kCoreBlocks * 32, (void**)&d.core_partial)) || (rc = scratch(area_blocks * 8, (void**)&d.area_partial)))
    {
        // leave the scene as it was before the call: a later update may try again
        for (void*& q : s->d_dyn) if (q) { (void)hipFree(q); q = nullptr; }
        s->bytes = bytes_before;
        return rc;
    }
    d.nodes = (float4*)s->d_nodes; d.quad = (uint4*)s->d_quad; d.tri = (float4*)s->d_tri; d.tripair = (float4*)s->d_tripair;
    d.leafbox = (float4*)s->d_leafbox; d.surf = (float4*)s->d_surf; d.lights = (float4*)s->d_lights; d.core = (float*)s->d_core;
    s->h_area.assign(area_blocks, 0.0);
    for (std::vector<int32_t>* v : {&h.bn, &h.order, &h.wide_bn, &h.quad_bn, &h.leaf_range, &h.tmap, &h.light_prim}) std::vector<int32_t>().swap(*v);
    std::vector<uint8_t>().swap(h.small);      // level_start stays: the launch sequence reads it
    s->dyn_ready = true;
    return PT_OK;
}

int pt_scene_update_vertices(PtScene* s, const float* d_pos, const float* d_frames, void* hip_stream)
{
    if (!s || !d_pos) { pt_set_error("pt_scene_update_vertices: NULL %s", !s ? "scene" : "d_pos"); return PT_ERR_INVALID; }
    HIPCHK(hipSetDevice(s->device));
    int rc;
    if ((rc = dyn_prepare(s)) != PT_OK) return rc;
    hipStream_t st = (hipStream_t)hip_stream;
    HIPCHK(ptk_dyn_update(&s->dyn, d_pos, d_frames, s->dyn_host.level_start.data(), (int)s->dyn_host.level_start.size() - 1, st));
    s->updated = true;
    return PT_OK;
}

int pt_scene_update_vertices_host(PtScene* s, const float* h_pos, const float* h_frames)
{
    if (!s || !h_pos) { pt_set_error("pt_scene_update_vertices_host: NULL %s", !s ? "scene" : "h_pos"); return PT_ERR_INVALID; }
    HIPCHK(hipSetDevice(s->device));
    const size_t n = (size_t)s->dev.n_tris;
    float *d_pos = nullptr, *d_frames = nullptr;
    auto body = [&]() -> int {
        HIPCHK(hipMalloc((void**)&d_pos, n * 36));
        HIPCHK(hipMemcpy(d_pos, h_pos, n * 36, hipMemcpyHostToDevice));
        if (h_frames) {
            HIPCHK(hipMalloc((void**)&d_frames, n * 108));
            HIPCHK(hipMemcpy(d_frames, h_frames, n * 108, hipMemcpyHostToDevice));
        }
        const int rc = pt_scene_update_vertices(s, d_pos, d_frames, nullptr);
        if (rc != PT_OK) return rc;
        HIPCHK(hipStreamSynchronize(nullptr));
        return PT_OK;
    };
    const int rc = body();
    (void)hipFree(d_pos); (void)hipFree(d_frames);
    return rc;
}

int pt_scene_update_spheres(PtScene* s, const PtSphere* h_spheres, int32_t n_spheres)
{
    if (!s || !h_spheres) { pt_set_error("pt_scene_update_spheres: NULL %s", !s ? "scene" : "h_spheres"); return PT_ERR_INVALID; }
    if (n_spheres != s->dev.n_spheres || n_spheres < 1) {
        pt_set_error("pt_scene_update_spheres: %d spheres given, the scene has %d", n_spheres, s->dev.n_spheres);
        return PT_ERR_INVALID;
    }
    for (int i = 0; i < n_spheres; i++)
        if (memcmp(&h_spheres[i].mat, &s->h_spheres[(size_t)i * 16 + 4], sizeof(PtMaterial)) != 0) {
            pt_set_error("pt_scene_update_spheres: the material of sphere %d differs from the uploaded one (only centre and radius may change)", i);
            return PT_ERR_INVALID;
        }
    HIPCHK(hipSetDevice(s->device));
    for (int i = 0; i < n_spheres; i++) {
        float* a = &s->h_spheres[(size_t)i * 16];
        a[0] = h_spheres[i].center[0]; a[1] = h_spheres[i].center[1]; a[2] = h_spheres[i].center[2]; a[3] = h_spheres[i].rad;
    }
    HIPCHK(hipMemcpy(s->d_spheres, s->h_spheres.data(), (size_t)n_spheres * 64, hipMemcpyHostToDevice));      // ordered on the NULL stream
    return PT_OK;
}

int pt_scene_tree_inflation(PtScene* s, double* ratio)
{
    if (!s || !ratio) { pt_set_error("pt_scene_tree_inflation: NULL %s", !s ? "scene" : "ratio"); return PT_ERR_INVALID; }
    *ratio = 1.0;
    if (!s->updated) return PT_OK;
    HIPCHK(hipSetDevice(s->device));
    HIPCHK(hipDeviceSynchronize());      // the stream of the last update may be gone by now: wait for the device, reduce on the NULL stream
    HIPCHK(ptk_dyn_area(&s->dyn, nullptr));
    HIPCHK(hipMemcpy(s->h_area.data(), s->dyn.area_partial, s->h_area.size() * 8, hipMemcpyDeviceToHost));
    double sum = 0.0;
    for (double v : s->h_area) sum += v;      // block sums in index order (host/accel_build.cpp: pt_accel_area_sum)
    *ratio = sum / s->dyn_host.area_sum;
    return PT_OK;
}

int64_t pt_dbg_scene_array(PtScene* s, int32_t which, void* h_out, int64_t cap_bytes)
{
    if (!s || which < 0 || which > 8 || cap_bytes < 0 || (cap_bytes > 0 && !h_out)) {
        pt_set_error("pt_dbg_scene_array: %s", !s ? "NULL scene" : (which < 0 || which > 8) ? "which must be 0..8" : "bad output buffer");
        return PT_ERR_INVALID;
    }
    void* const src[9] = {s->d_nodes, s->d_quad, s->d_tri, s->d_tripair, s->d_leafbox, s->d_surf, s->d_lights, s->d_spheres, s->d_core};
    const int64_t size = (int64_t)s->array_bytes[which];
    const int64_t n = size < cap_bytes ? size : cap_bytes;
    if (n > 0) {
        HIPCHK(hipSetDevice(s->device));
        HIPCHK(hipDeviceSynchronize());
        HIPCHK(hipMemcpy(h_out, src[which], (size_t)n, hipMemcpyDeviceToHost));
    }
    return size;
}

// ---- ray queries (csrc/pt_query.hip) -------------------------------------------------------------------------------------------
static int query_args_ok(const char* who, const PtScene* s, const float* rays, int64_t n, int32_t mode, const PtRayHit* hits, const float* surface,
                         bool device)
{
    const char* bad = !s ? "NULL scene" : !rays ? "NULL rays" : !hits ? "NULL hits" : n < 0 ? "n < 0" :
                      (mode != PT_QUERY_CLOSEST && mode != PT_QUERY_ANY) ? "mode must be PT_QUERY_CLOSEST or PT_QUERY_ANY" :
                      (mode == PT_QUERY_ANY && surface) ? "an any-hit query has no surface record (d_surface29 must be NULL)" :
                      (device && ((uintptr_t)rays & 15)) ? "rays must be 16-byte aligned" :
                      (device && ((uintptr_t)hits & 7)) ? "hits must be 8-byte aligned" :
                      (device && ((uintptr_t)surface & 3)) ? "surface must be 4-byte aligned" : nullptr;
    if (bad) { pt_set_error("%s: %s", who, bad); return PT_ERR_INVALID; }
    return PT_OK;
}

int pt_trace_rays(PtScene* s, const float* d_rays8, int64_t n, int32_t mode, PtRayHit* d_hits, float* d_surface29, void* hip_stream)
{
    int rc;
    if ((rc = query_args_ok("pt_trace_rays", s, d_rays8, n, mode, d_hits, d_surface29, true)) != PT_OK) return rc;
    if (n == 0) return PT_OK;
    HIPCHK(hipSetDevice(s->device));
    const bool quad = s->query_quad && ptk_query_quad_fits(s->dev.quad_depth);
    const int64_t kBatch = (int64_t)1 << 30;      // rays per launch: ray numbers are 32-bit
    for (int64_t off = 0; off < n; off += kBatch) {
        const uint32_t m = (uint32_t)(n - off < kBatch ? n - off : kBatch);
        HIPCHK(ptk_trace_rays(&s->dev, d_rays8 + off * 8, m, mode == PT_QUERY_ANY, quad, d_hits + off,
                              d_surface29 ? d_surface29 + off * 29 : nullptr, (hipStream_t)hip_stream));
    }
    return PT_OK;
}

int pt_trace_rays_host(PtScene* s, const float* h_rays8, int64_t n, int32_t mode, PtRayHit* h_hits, float* h_surface29)
{
    int rc;
    if ((rc = query_args_ok("pt_trace_rays_host", s, h_rays8, n, mode, h_hits, h_surface29, false)) != PT_OK) return rc;
    if (n == 0) return PT_OK;
    HIPCHK(hipSetDevice(s->device));
    float *d_rays = nullptr, *d_surf = nullptr;
    PtRayHit* d_hits = nullptr;
    auto body = [&]() -> int {
        HIPCHK(hipMalloc((void**)&d_rays, (size_t)n * 32));
        HIPCHK(hipMalloc((void**)&d_hits, (size_t)n * 8));
        if (h_surface29) HIPCHK(hipMalloc((void**)&d_surf, (size_t)n * 116));
        HIPCHK(hipMemcpy(d_rays, h_rays8, (size_t)n * 32, hipMemcpyHostToDevice));
        const int r = pt_trace_rays(s, d_rays, n, mode, d_hits, d_surf, nullptr);
        if (r != PT_OK) return r;
        HIPCHK(hipStreamSynchronize(nullptr));
        HIPCHK(hipMemcpy(h_hits, d_hits, (size_t)n * 8, hipMemcpyDeviceToHost));
        if (h_surface29) HIPCHK(hipMemcpy(h_surface29, d_surf, (size_t)n * 116, hipMemcpyDeviceToHost));
        return PT_OK;
    };
    rc = body();
    (void)hipFree(d_rays); (void)hipFree(d_hits); (void)hipFree(d_surf);
    return rc;
}

// ---- parity hooks ------------------------------------------------------------------------
int pt_dbg_raycast(PtScene* s, const float* rays8, int32_t n, float* out_hits29, int32_t* out_prim)
{
    if (!s || !rays8 || n < 0 || !out_hits29 || !out_prim) { pt_set_error("pt_dbg_raycast: bad argument"); return PT_ERR_INVALID; }
    return with_buffers(s->device, rays8, (size_t)n * 32, out_hits29, (size_t)n * 29 * 4, out_prim, (size_t)n * 4,
                        [&](void* i, void* o, void* o2) { return ptk_dbg_raycast(&s->dev, (const float*)i, n, (float*)o, (int*)o2, nullptr); });
}
int pt_dbg_bxdf(int32_t device, int32_t lobe, const float* in28, int32_t n, float* out12)
{
    if (!in28 || !out12 || n < 0 || lobe < 0 || lobe > 3) { pt_set_error("pt_dbg_bxdf: bad argument"); return PT_ERR_INVALID; }
    return with_buffers(device, in28, (size_t)n * 28 * 4, out12, (size_t)n * 12 * 4, nullptr, 0,
                        [&](void* i, void* o, void*) { return ptk_dbg_bxdf(lobe, (const float*)i, n, (float*)o, nullptr); });
}
int pt_dbg_rng(int32_t device, uint64_t seed, int32_t n, uint32_t* raw_out, float* uniform_out)
{
    if (!raw_out || !uniform_out || n < 0) { pt_set_error("pt_dbg_rng: bad argument"); return PT_ERR_INVALID; }
    return with_buffers(device, nullptr, 0, raw_out, (size_t)n * 4, uniform_out, (size_t)n * 4,
                        [&](void*, void* o, void* o2) { return ptk_dbg_rng(seed, n, (uint32_t*)o, (float*)o2, nullptr); });
}
__global__ __launch_bounds__(256) void triad_kernel(float4* __restrict__ a, const float4* __restrict__ b, const float4* __restrict__ c, float s, size_t n)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) {
        const float4 x = b[i], y = c[i];
        a[i] = make_float4(x.x + s * y.x, x.y + s * y.y, x.z + s * y.z, x.w + s * y.w);
    }
}

int pt_dbg_triad(int32_t device, int64_t bytes_per_array, int32_t iters, double* gb_per_s)
{
    if (!gb_per_s || bytes_per_array < 4096 || iters < 1) { pt_set_error("pt_dbg_triad: bad argument"); return PT_ERR_INVALID; }
    HIPCHK(hipSetDevice(device));
    const size_t n = (size_t)bytes_per_array / 16;
    float4 *a = nullptr, *b = nullptr, *c = nullptr;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    int rc = PT_OK;
    do {
        if (hipMalloc((void**)&a, n * 16) != hipSuccess || hipMalloc((void**)&b, n * 16) != hipSuccess || hipMalloc((void**)&c, n * 16) != hipSuccess) { pt_set_error("pt_dbg_triad: out of device memory"); rc = PT_ERR_DEVICE; break; }
        (void)hipMemset(b, 0, n * 16); (void)hipMemset(c, 0, n * 16);
        (void)hipEventCreate(&e0); (void)hipEventCreate(&e1);
        const unsigned blocks = (unsigned)((n + 255) / 256);
        hipLaunchKernelGGL(triad_kernel, dim3(blocks), dim3(256), 0, 0, a, b, c, 0.5f, n);       // warm-up
        (void)hipEventRecord(e0, 0);
        for (int k = 0; k < iters; k++) hipLaunchKernelGGL(triad_kernel, dim3(blocks), dim3(256), 0, 0, a, b, c, 0.5f, n);
        (void)hipEventRecord(e1, 0);
        if (hipEventSynchronize(e1) != hipSuccess) { pt_set_error("pt_dbg_triad: kernel failed"); rc = PT_ERR_DEVICE; break; }
        float ms = 0.f;
        (void)hipEventElapsedTime(&ms, e0, e1);
        *gb_per_s = 3.0 * (double)n * 16.0 * iters / ((double)ms * 1e-3) / 1e9;
    } while (0);
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    if (a) (void)hipFree(a);
    if (b) (void)hipFree(b);
    if (c) (void)hipFree(c);
    return rc;
}

int pt_dbg_pixel_dir(int32_t device, const PtCamera* cam, const int32_t* pxpypass, int32_t n, float* out8)
{
    if (!cam || !pxpypass || !out8 || n < 0 || cam->W < 2 || cam->H < 2) { pt_set_error("pt_dbg_pixel_dir: bad argument"); return PT_ERR_INVALID; }
    ptd::DevCamera c;
    fill_camera(cam, c);
    return with_buffers(device, pxpypass, (size_t)n * 12, out8, (size_t)n * 32, nullptr, 0,
                        [&](void* i, void* o, void*) { return ptk_dbg_pixel_dir(&c, (const int*)i, n, (float*)o, nullptr); });
}
int pt_dbg_nee(PtScene* s, const float* in5, int32_t n, float* out12)
{
    if (!s || !in5 || !out12 || n < 0) { pt_set_error("pt_dbg_nee: bad argument"); return PT_ERR_INVALID; }
    if (s->n_lights < 1) { pt_set_error("pt_dbg_nee: scene has no light"); return PT_ERR_NO_LIGHT; }
    return with_buffers(s->device, in5, (size_t)n * 20, out12, (size_t)n * 48, nullptr, 0,
                        [&](void* i, void* o, void*) { return ptk_dbg_nee(&s->dev, (const float*)i, n, (float*)o, nullptr); });
}

int pt_dbg_ray_setup(int32_t device, const float* dir3, int32_t n, float* out5)
{
    if (!dir3 || !out5 || n < 0) { pt_set_error("pt_dbg_ray_setup: bad argument"); return PT_ERR_INVALID; }
    return with_buffers(device, dir3, (size_t)n * 12, out5, (size_t)n * 20, nullptr, 0,
                        [&](void* i, void* o, void*) { return ptk_dbg_ray_setup((const float*)i, n, (float*)o, nullptr); });
}
int pt_dbg_math(int32_t device, const float* in, int32_t n, float* out8)
{
    if (!in || !out8 || n < 0) { pt_set_error("pt_dbg_math: bad argument"); return PT_ERR_INVALID; }
    return with_buffers(device, in, (size_t)n * 4, out8, (size_t)n * 8 * 4, nullptr, 0,
                        [&](void* i, void* o, void*) { return ptk_dbg_math((const float*)i, n, (float*)o, nullptr); });
}
int pt_dbg_sincos(int32_t device, const float* in, int32_t n, float* out2)
{
    if (!in || !out2 || n < 0) { pt_set_error("pt_dbg_sincos: bad argument"); return PT_ERR_INVALID; }
    return with_buffers(device, in, (size_t)n * 4, out2, (size_t)n * 2 * 4, nullptr, 0,
                        [&](void* i, void* o, void*) { return ptk_dbg_sincos((const float*)i, n, (float*)o, nullptr); });
}

}  // extern "C"
