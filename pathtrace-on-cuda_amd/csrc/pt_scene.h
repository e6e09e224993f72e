// pt_scene.h — the uploaded scene behind the C-ABI's opaque PtScene*: its device arrays, the resources it lends a render, its settings and
// the state of the dynamic-geometry path.  Built by pt_scene.hip (pt_scene_create); included by every file whose entry points take a scene.
// Everything the scene owns is released by its destructor, whichever path deletes it.
#pragma once
#include <cstdlib>
#include <type_traits>
#include <vector>

#include "pt_internal.h"

// The device arrays a render reads (layouts: pt_device.h), in the order of pt_dbg_scene_array's `which` and of ptamd.SCENE_ARRAYS.
enum SceneArray { kArrNodes, kArrQuad, kArrTri, kArrTripair, kArrLeafbox, kArrSurf, kArrLights, kArrSpheres, kArrCore, kSceneArrays };
// The allocations of the first update (pt_dynamic.hip: pt_dyn_prepare): the 8 maps of the build and the position mirror, which come
// from the host, then 5 scratch arrays.  kDynLightPrim grows with the set of lights (pt_material.hip).
constexpr int kMatBlock = 256;      // triangles per block of the material update: kDynMatPartial holds one int2 per block and one more
enum DynAlloc { kDynBn, kDynOrder, kDynWideBn, kDynQuadBn, kDynLeafRange, kDynTmap, kDynLightPrim, kDynSmall, kDynPos,
                kDynBbox, kDynMaxabs, kDynCorePartial, kDynAreaPartial, kDynMatPartial, kDynAllocs };

struct PtScene {
    int device = 0;
    ptd::DevScene dev{};
    DevBuf arr[kSceneArrays];            // as uploaded; an empty array holds 16 bytes, kArrCore is null when the scene has no core box; nodes and quad have
                                         // room for n_tris - 1 records once a tree rebuild has run (dev.n_nodes / dev.n_quad are the counts)
    DevBuf uv;                           // u0 v0 u1 v1 u2 v2 per triangle (reference order): HitResult::u / v of the HIT record (parity hook, surface pass of the queries)
    DevBuf unit_counter;
    DevBuf counters;
    DevBuf tile_list;                    // the tile numbers (int32) of the pt_render_tile_list call in flight (grown on demand)
    DevBuf views;                        // the cameras of the pt_render_views call in flight (grown on demand): origins (float4) | DevCamera | first pass (int32), one capacity each
    std::vector<char> h_views;           // host image of `views` (the source of its stream-ordered copy)
    int64_t bytes = 0;
    int n_lights = 0;
    int max_depth = 0;       // deepest node of the binary traversal tree, from upload or from the last rebuild
    int num_cus = 256;
    bool count_next = false;
    int mode = 1;            // 1 = wavefront pipeline (default), 0 = one-kernel state machine
    ptd::WfLent wf;          // what every run of the wavefront pipeline borrows: early shade's stream and events, the pinned poll word (frees itself)
    int last_iters = 0;
    int shade_rounds = 1;        // wf_shade: 1 = a stream may start its next sample in the step its path ends, 0 = one bounce per step, -1 = by live-stream count (pt_wavefront.hip: kTwoRoundsBelow)
    int early_below = 2500000;   // renders of at most this many streams (pixels x passes of one call) run wf_shade's early phase beside the draining wf_trace (0 = never; pt_set_early_shade)
    int drain_below = 80000;     // hand the last streams of a render to wf_drain once this few are live (0 = never; PTAMD_DRAIN, pt_set_drain_threshold):
                                 // the last ~200 of ~1,100 bounce iterations serve < 5 % of the streams at the latency of the longest ray each
                                 // (~200 us); wf_drain runs those streams to their end in one launch, spread over every SIMD.  40,000-120,000 is flat:
                                 // +5...7 % for an 8-way rank, +3 % 4-way, +1 % on one GPU (r03_b31.log, r03_b32.log, r03_b33.log)
    // optional per-launch timing of the traversal kernel (pt_enable_trace_timing)
    std::vector<hipEvent_t> trace_ev;
    int trace_ev_used = 0;                   // triples of trace_ev the last render recorded (one per iteration)
    // ring of HIP event pairs, one pair per render_units launch (pt_render_timings)
    static constexpr int kEvRing = 64;
    hipEvent_t ev[kEvRing][2] = {};
    int ev_count = 0;        // launches recorded since the last pt_render_timings(reset)
    // ---- dynamic geometry (pt_scene_update_vertices, csrc/pt_dynamic.hip) ----
    std::vector<float> h_spheres;        // the uploaded sphere records: pt_scene_update_spheres checks the materials against them and copies from here
    struct DynHost {                     // the maps of the build and the positions, kept on the host until the first update uploads them
        std::vector<int32_t> bn, order, level_start, wide_bn, quad_bn, leaf_range, tmap, light_prim;
        std::vector<uint8_t> small;
        std::vector<float> pos;          // V0 V1 V2 per triangle (reference order): becomes the device mirror kDynPos, which every vertex update refreshes
        double area_sum = 0.0;
    } dyn_host;
    ptd::DynScene dyn{};                 // device side of the same: the rewritten arrays from upload on, the maps and scratch once dyn_ready
    DevBuf dyn_buf[kDynAllocs];          // its allocations (dyn_prepare); kDynSmall stays null when the scene has no core box
    bool dyn_ready = false;
    bool updated = false;
    std::vector<double> h_area;          // host image of dyn.area_partial
    // ---- tree rebuild (pt_scene_rebuild_tree, csrc/pt_rebuild.hip) ----
    std::vector<DevBuf> rb_buf;          // the build's workspace, one slot per line of pt_rebuild.hip's table, worst case: a rebuild allocates what its
                                         // parameters need and no earlier call did (rb_prepare)
    size_t rb_temp_bytes = 0, rb_temp64_bytes = 0;      // rocPRIM's temporary storage (queried once); the second is 0 where the first serves the 64-bit sort too
    bool rb_ready = false;
    int rebuilds = 0;
    // ---- materials and lights (pt_scene_update_materials, csrc/pt_material.hip) ----
    bool tri_emit_ok = true;             // emittance_ok's test over the triangles alone, from pt_scene_create or the last material update (the spheres' part: h_spheres)
    int32_t* h_mat = nullptr;            // pinned, 2 words: the light count and the flag a material update reads back (pt_dyn_prepare)
    // ---- ray queries (pt_trace_rays, csrc/pt_query.hip) ----
    bool query_quad = true;              // walk the 4-wide tree when it fits the kernel's stack (PTAMD_QUERY_QUAD=0: the binary tree, A/B)

    // The events; `wf` and the DevBuf members free themselves after it.  The caller has made `device` current.
    ~PtScene()
    {
        for (int i = 0; i < kEvRing; i++) for (int j = 0; j < 2; j++) if (ev[i][j]) (void)hipEventDestroy(ev[i][j]);
        for (hipEvent_t e : trace_ev) if (e) (void)hipEventDestroy(e);
        if (h_mat) (void)hipHostFree(h_mat);
    }
};

// Which walk pt_trace_rays and the feature-buffer kernel of pt_aov.hip take: the 4-wide tree when its walk fits their per-lane stack
// (and PTAMD_QUERY_QUAD=0 does not force the other), else the binary tree with trace_closest
inline bool pt_query_walks_quad(const PtScene* s) { return s->query_quad && 3 * s->dev.quad_depth + 2 <= ptd::kQueryStack; }

// ---- what the query entry points share (pt_query.hip, pt_nearest.hip, pt_knearest.hip, pt_rayhits.hip; pt_aov.hip: pt_aov_rays) ----
// The argument checks, in the order every query makes them: scene, input, a list's offsets, output (a list's host variant may leave it
// NULL: the sizing call), n, a list's cap, the query's own parameters (`param`: the message of the first one that fails, nullptr = none),
// then on the device the alignment of input (16), offsets (8), output (outAlign bytes, named outName) and detail (4, named detName).
// A filtered query (`filter`; NULL, the neutral one, has nothing to check) adds, after all of its twin's: unknown filter flags,
// PT_FILTER_TMIN on a point query, the alignment (4) of the filter's three arrays.  The filter is a host struct and is read; its
// arrays are not.  PT_OK, or PT_ERR_INVALID with "who: message" set.
struct QueryArgs {
    const char* in; const void* inPtr;                                   // "rays" or "points"
    const char* outNull; const void* outPtr;                             // the name "NULL ..." gives the output
    const char* outName; int outAlign;
    const char* detName; const void* detPtr;
    const char* param;
    bool list; const int64_t* offsets; int64_t cap;
    const PtQueryFilter* filter; bool filterRays;                        // the _f entry points; filterRays: a ray query (it may take PT_FILTER_TMIN)
};
inline int pt_query_args(const char* who, const PtScene* s, int64_t n, bool device, const QueryArgs& a)
{
    const auto fail = [&](const char* fmt, const char* what) { pt_set_error(fmt, who, what); return PT_ERR_INVALID; };
    if (!s) return fail("%s: NULL %s", "scene");
    if (!a.inPtr) return fail("%s: NULL %s", a.in);
    if (a.list && !a.offsets) return fail("%s: NULL %s", "offsets");
    if ((device || !a.list) && !a.outPtr) return fail("%s: NULL %s", a.outNull);
    if (n < 0) return fail("%s: %s", "n < 0");
    if (a.list && a.cap < 0) return fail("%s: %s", "cap < 0");
    if (a.param) return fail("%s: %s", a.param);
    if (!device) return PT_OK;
    if ((uintptr_t)a.inPtr & 15) return fail("%s: %s must be 16-byte aligned", a.in);
    if (a.list && ((uintptr_t)a.offsets & 7)) return fail("%s: %s must be 8-byte aligned", "offsets");
    if ((uintptr_t)a.outPtr & (uintptr_t)(a.outAlign - 1)) return fail(a.outAlign == 8 ? "%s: %s must be 8-byte aligned" : "%s: %s must be 4-byte aligned", a.outName);
    if ((uintptr_t)a.detPtr & 3) return fail("%s: %s must be 4-byte aligned", a.detName);
    if (a.filter) {
        const PtQueryFilter& f = *a.filter;
        if (f.flags & ~PT_FILTER_TMIN) return fail("%s: %s", "unknown filter flags");
        if ((f.flags & PT_FILTER_TMIN) && !a.filterRays) return fail("%s: %s", "PT_FILTER_TMIN applies to ray queries only");
        if ((uintptr_t)f.d_prim_bits & 3) return fail("%s: %s must be 4-byte aligned", "filter d_prim_bits");
        if ((uintptr_t)f.d_query_bits & 3) return fail("%s: %s must be 4-byte aligned", "filter d_query_bits");
        if ((uintptr_t)f.d_skip_prim & 3) return fail("%s: %s must be 4-byte aligned", "filter d_skip_prim");
    }
    return PT_OK;
}

constexpr int64_t kQueryBatch = (int64_t)1 << 30;      // queries per launch: query numbers are 32-bit

// launch(off, m) for each batch of m <= kQueryBatch queries from off, in order; the first error ends the loop
template <class LAUNCH>
inline hipError_t pt_query_batches(int64_t n, LAUNCH launch)
{
    for (int64_t off = 0; off < n; off += kQueryBatch) {
        const hipError_t e = launch(off, (uint32_t)(n - off < kQueryBatch ? n - off : kQueryBatch));
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

// f(std::integral_constant<int, KC>()) with KC the capacity class of a K query's list: the smallest of 4, 8, 16, 32 that holds k, so that
// k = 2 does not pay the LDS of k = 32
template <class F>
inline void pt_kc_dispatch(int k, F f)
{
    if (k <= 4) f(std::integral_constant<int, 4>());
    else if (k <= 8) f(std::integral_constant<int, 8>());
    else if (k <= 16) f(std::integral_constant<int, 16>());
    else f(std::integral_constant<int, 32>());
}

// The detail kernels of the K queries, one 256-thread workgroup per 256 slots: 2^30 queries are up to 2^35 slots, so launch(first,
// blocks) enqueues the slots from `first` on, at most kDetailSlots of them (a multiple of 256), so that no grid exceeds 2^31 threads
constexpr uint64_t kDetailSlots = (uint64_t)1 << 31;
template <class LAUNCH>
inline void pt_detail_chunks(uint64_t slots, LAUNCH launch)
{
    for (uint64_t first = 0; first < slots; first += kDetailSlots) {
        const uint64_t m = slots - first < kDetailSlots ? slots - first : kDetailSlots;
        launch(first, dim3((uint32_t)((m + 255u) / 256u)));
    }
}

// The body of a query's _host variant, after its checks and hipSetDevice: the inBytes of h_in and room for the outBytes of h_out and, if
// h_det is given, the detBytes of h_det on the device; run(d_in, d_out, d_det) — the device entry point on the null stream, d_det null
// when h_det is —, a synchronisation, the results copied back.
template <class RUN>
inline int pt_host_query(const void* h_in, size_t inBytes, void* h_out, size_t outBytes, void* h_det, size_t detBytes, RUN run)
{
    DevBuf d_in, d_out, d_det;
    HIPCHK(d_in.alloc(inBytes));
    HIPCHK(d_out.alloc(outBytes));
    if (h_det) HIPCHK(d_det.alloc(detBytes));
    HIPCHK(hipMemcpy(d_in.as<>(), h_in, inBytes, hipMemcpyHostToDevice));
    int rc;
    if ((rc = run(d_in.as<float>(), d_out.as<>(), d_det.as<float>())) != PT_OK) return rc;
    HIPCHK(hipStreamSynchronize(nullptr));
    HIPCHK(hipMemcpy(h_out, d_out.as<>(), outBytes, hipMemcpyDeviceToHost));
    if (h_det) HIPCHK(hipMemcpy(h_det, d_det.as<>(), detBytes, hipMemcpyDeviceToHost));
    return PT_OK;
}

// The body of a list's _host variant (pt_trace_rays_list_host, pt_within_radius_list_host), after its checks and hipSetDevice: n > 0
// queries of inRec bytes each; count(d_in, d_count) and offsets into h_offsets; without h_out the sizing call ends there; else cap must
// hold the total, and fill(d_in, d_offsets, total, d_out, d_det) writes records of 8 bytes and, if h_det is given, detRec bytes.
template <class COUNT, class FILL>
inline int pt_host_list(const char* who, const void* h_in, int64_t n, size_t inRec, int64_t* h_offsets, int64_t cap, void* h_out, void* h_det,
                        size_t detRec, COUNT count, FILL fill)
{
    DevBuf d_in, d_count, d_off, d_scratch, d_out, d_det;      // d_det stays null when the caller asked for no detail records
    HIPCHK(d_in.alloc((size_t)n * inRec));
    HIPCHK(d_count.alloc((size_t)n * 4));
    HIPCHK(d_off.alloc((size_t)(n + 1) * 8));
    HIPCHK(d_scratch.alloc((size_t)pt_list_offsets_scratch_bytes(n)));
    HIPCHK(hipMemcpy(d_in.as<>(), h_in, (size_t)n * inRec, hipMemcpyHostToDevice));
    int rc;
    if ((rc = count(d_in.as<float>(), d_count.as<int32_t>())) != PT_OK) return rc;
    if ((rc = pt_list_offsets(d_count.as<int32_t>(), n, d_off.as<int64_t>(), d_scratch.as<>(), nullptr)) != PT_OK) return rc;
    HIPCHK(hipStreamSynchronize(nullptr));
    HIPCHK(hipMemcpy(h_offsets, d_off.as<>(), (size_t)(n + 1) * 8, hipMemcpyDeviceToHost));
    if (!h_out) return PT_OK;      // the sizing call
    const int64_t total = h_offsets[n];
    if (cap < total) { pt_set_error("%s: cap %lld < %lld records", who, (long long)cap, (long long)total); return PT_ERR_INVALID; }
    HIPCHK(d_out.alloc((size_t)total * 8));
    if (h_det) HIPCHK(d_det.alloc((size_t)total * detRec));
    if ((rc = fill(d_in.as<float>(), d_off.as<int64_t>(), total, d_out.as<>(), d_det.as<float>())) != PT_OK) return rc;
    HIPCHK(hipStreamSynchronize(nullptr));
    HIPCHK(hipMemcpy(h_out, d_out.as<>(), (size_t)total * 8, hipMemcpyDeviceToHost));
    if (h_det) HIPCHK(hipMemcpy(h_det, d_det.as<>(), (size_t)total * detRec, hipMemcpyDeviceToHost));
    return PT_OK;
}

// pt_api.hip: the table of a batch of views in the scene's buffer `views` (grown on demand; the caller knows that nothing on the device
// still reads the old one): origins | cameras | first passes, packed by way of the host image h_views and copied in stream order.
// first = h_first_pass[v], or default_first for every view when h_first_pass is NULL.  PT_OK, or PT_ERR_DEVICE with the error text set.
struct PtViewTable { const ptd::DevCamera* cams; const int32_t* firstPass; const float4* org; };
int pt_upload_views(PtScene* s, const PtCamera* h_cams, int32_t n_views, int32_t default_first, const int32_t* h_first_pass, hipStream_t stream,
                    PtViewTable& t);

// DevScene::nee_prune may be 1 unless PTAMD_PRUNE=0 (A/B only); read whenever the flag is formed
inline bool pt_prune_allowed() { const char* m = getenv("PTAMD_PRUNE"); return !(m && atoi(m) == 0); }
// pt_dynamic.hip: the first update of either kind brings the maps and the position mirror to the device (no-op afterwards)
int pt_dyn_prepare(PtScene* s);
// pt_dynamic.hip: enqueues a vertex update on `stream`.  level_start: host array of n_levels + 1 offsets into `order`.  trees_only: the
// records and boxes of the two traversal trees alone (tri, tripair, nodes, quad) — leafbox, surf, lights, the core box and the
// position mirror d_keep are not touched (a tree rebuild: the positions are the scene's own)
hipError_t pt_dyn_launch_update(const ptd::DynScene& s, const float* d_pos, const float* d_frames, float* d_keep, const int32_t* level_start, int n_levels,
                                bool trees_only, hipStream_t stream);
// pt_dynamic.hip: enqueues dyn_area, the block sums of the box areas of all n_bn builder nodes into s.area_partial
hipError_t pt_dyn_launch_area(const ptd::DynScene& s, hipStream_t stream);
// pt_scene.hip: the stack limits of the traversal kernels (host only): PT_OK, or PT_ERR_UNSUPPORTED with the error text set
int pt_tree_limits(const char* who, int depth, int quad_depth);
