// pt_scene.h — the uploaded scene behind the C-ABI's opaque PtScene*: its device arrays, the resources it lends a render, its settings and
// the state of the dynamic-geometry path.  Built by pt_scene.hip (pt_scene_create); included by every file whose entry points take a scene.
// Everything the scene owns is released by its destructor, whichever path deletes it.
#pragma once
#include <cstdlib>
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
