// pt_scene.hip — scene upload into the HBM layout of pt_device.h (include/pt_api.h: pt_scene_create, pt_scene_destroy, the scene getters,
// pt_dbg_scene_array).
//
// Replaces the scene half of PathTracer::Render (srcs/pathtracer.cu:124-259): instead of five cudaMallocManaged regions filled element
// by element from the host and a device vtable plant, the scene is repacked once on the host into 16-byte records and copied with one
// hipMemcpy per array.  pt_scene_create is a sequence of named steps, each a static function below.  The core box and the light test
// are float arithmetic that a vertex update (pt_dynamic.hip) restates on the device bit for bit: this file is built with the library's
// device flags (no contraction), not with the host files' compiler.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "pt_scene.h"
#include "../host/accel_build.h"

// ---- validate the flattened tree (host check before any kernel sees it) ----
static int validate_tree(const PtBVHNode* nodes, int32_t n_nodes, int32_t n_tris)
{
    std::vector<int> depth((size_t)n_nodes, -1);
    std::vector<int> widx((size_t)n_nodes, -1);
    {
        std::vector<int> st; st.push_back(0); depth[0] = 0;
        std::vector<char> seen((size_t)n_nodes, 0);
        while (!st.empty()) {
            int i = st.back(); st.pop_back();
            if (seen[(size_t)i]) { pt_set_error("pt_scene_create: node %d reachable twice", i); return PT_ERR_INVALID; }
            seen[(size_t)i] = 1;
            const PtBVHNode& n = nodes[i];
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
                widx[(size_t)i] = 0;    // an interior node
                depth[n.childL] = depth[i] + 1; depth[n.childR] = depth[i] + 1;
                st.push_back(n.childR); st.push_back(n.childL);
            }
        }
    }
    // every triangle must belong to exactly one reference leaf (its box decides acceptance)
    std::vector<char> covered((size_t)n_tris, 0);
    for (int i = 0; i < n_nodes; i++) {
        const PtBVHNode& n = nodes[i];
        if (widx[(size_t)i] == -1 && depth[(size_t)i] >= 0 && n.primStart != -1 && n.primEnd != -1)
            for (int k = n.primStart; k <= n.primEnd; k++) covered[(size_t)k]++;
    }
    for (int k = 0; k < n_tris; k++)
        if (covered[(size_t)k] != 1) { pt_set_error("pt_scene_create: triangle %d is in %d reference leaves", k, (int)covered[(size_t)k]); return PT_ERR_INVALID; }
    return PT_OK;
}

// ---- triangles: surface records (reference order), lights; spheres ----
static void pack_surfaces(const PtTriangle* tris, int32_t n_tris, std::vector<float>& surf, std::vector<float>& lights, std::vector<int32_t>& light_prim)
{
    surf.resize((size_t)n_tris * 48);
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
            light_prim.push_back(i);          // reference-order triangle of every light (for a vertex update)
        }
    }
}

static std::vector<float> pack_spheres(const PtSphere* spheres, int32_t n_spheres)
{
    std::vector<float> sph((size_t)n_spheres * 16);
    for (int i = 0; i < n_spheres; i++) {
        const PtSphere& s = spheres[i];
        float* a = &sph[(size_t)i * 16];
        a[0] = s.center[0]; a[1] = s.center[1]; a[2] = s.center[2]; a[3] = s.rad;
        memcpy(a + 4, &s.mat, sizeof(PtMaterial));
    }
    return sph;
}

// dead-NEE-term pruning (pt_stream.h: bounce) needs every emittance a shadow ray can return to be finite, non-negative and small
// enough that (weight * brdfcos) * Le cannot overflow where the pruned case assumes it is finite: |wb| < 1e30 and Le <= 1e8 give
// |wb * Le| < 1e38 < FLT_MAX.  (With a brighter light wb * Le can be inf, inf * 0 is NaN, and the reference adds that NaN to the
// radiance, include/CudaUtil.cuh:271-272; such scenes keep all their shadow rays.)
// triOk: the triangles' part alone, which a material update of the spheres combines with the new spheres (pt_material.hip).
static bool emittance_ok(const PtTriangle* tris, int32_t n_tris, const PtSphere* spheres, int32_t n_spheres, bool& triOk)
{
    bool emitOk = true;
    auto okE = [](const float* e) { return std::isfinite(e[0]) && std::isfinite(e[1]) && std::isfinite(e[2]) && e[0] >= 0.f && e[1] >= 0.f && e[2] >= 0.f &&
                                           e[0] <= 1e8f && e[1] <= 1e8f && e[2] <= 1e8f; };
    for (int i = 0; i < n_tris; i++) emitOk = emitOk && okE(tris[i].mat0.emittance);
    triOk = emitOk;
    for (int i = 0; i < n_spheres; i++) emitOk = emitOk && okE(spheres[i].mat.emittance);
    return emitOk;
}

// ---- core box: the AABB of the scene's SMALL triangles (bounding-box diagonal under an eighth of the scene's).  A ray whose
// segment misses it can only meet the few big triangles, i.e. is short, and wf_shade queues such rays last (pt_stream.h:
// ray_is_short) so that the traversal kernel's launch tail consists of short rays.  Scheduling only — any box gives the same frame.
// core: 6 floats, or empty when the scene gets none.  small: per triangle, inside the core box's set (for a vertex update).
static void core_box(const PtTriangle* tris, int32_t n_tris, std::vector<float>& core, std::vector<uint8_t>& small)
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

// ---- upload: one allocation and one copy per array of the table (an empty array still holds 16 bytes) ----
struct HostArray { const void* data; size_t bytes; };
static int upload_arrays(PtScene* sc, const HostArray (&src)[kSceneArrays])
{
    for (int a = 0; a < kSceneArrays; a++) {
        if (a == kArrCore && !src[a].bytes) continue;      // no core box: the pointer stays null
        HIPCHK(sc->arr[a].upload(src[a].data, src[a].bytes));
        sc->bytes += (int64_t)sc->arr[a].held();
    }
    // the one place that knows which array a kernel argument block calls what (a vertex update rewrites all but the spheres)
    ptd::DevScene& d = sc->dev;
    ptd::DynScene& y = sc->dyn;
    d.nodes = y.nodes = sc->arr[kArrNodes].as<float4>(); d.quad = y.quad = sc->arr[kArrQuad].as<uint4>(); d.tri = y.tri = sc->arr[kArrTri].as<float4>();
    d.tripair = y.tripair = sc->arr[kArrTripair].as<float4>(); d.leafbox = y.leafbox = sc->arr[kArrLeafbox].as<float4>();
    d.surf = y.surf = sc->arr[kArrSurf].as<float4>(); d.lights = y.lights = sc->arr[kArrLights].as<float4>();
    d.spheres = sc->arr[kArrSpheres].as<float4>();
    d.core = y.core = sc->arr[kArrCore].as<float>();      // nullptr: no queue order by ray class
    return PT_OK;
}

// ---- what the scene lends every render: counters, the event ring, and the pipeline's stream, events and pinned poll word (WfLent) ----
static int create_resources(PtScene* sc)
{
    HIPCHK(sc->unit_counter.alloc(64));
    HIPCHK(sc->counters.alloc(ptd::kStatBytes));      // 8 work counters (+ the diagnostic launch timeline of wf_trace)
    HIPCHK(hipMemset(sc->counters.as<>(), 0, ptd::kStatBytes));
    for (int i = 0; i < PtScene::kEvRing; i++) { HIPCHK(hipEventCreate(&sc->ev[i][0])); HIPCHK(hipEventCreate(&sc->ev[i][1])); }
    HIPCHK(sc->wf.create());
    hipDeviceProp_t prop;
    HIPCHK(hipGetDeviceProperties(&prop, sc->device));
    sc->num_cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    return PT_OK;
}

// ---- the per-scene defaults and their environment overrides (the same settings have C-ABI setters: pt_set_mode, pt_set_drain_threshold) ----
static void apply_defaults(PtScene* sc, int32_t n_tris, bool emitOk)
{
    if (const char* m = getenv("PTAMD_MODE")) { const int v = atoi(m); if (v >= 0 && v <= 1) sc->mode = v; }
    if (const char* m = getenv("PTAMD_DRAIN")) sc->drain_below = atoi(m);
    if (const char* m = getenv("PTAMD_EARLY")) sc->early_below = atoi(m) > 0 ? atoi(m) : 0;      // 0 = off
    // shading schedule (pt_set_shade_rounds): one bounce per step pays when wf_shade is bound by its arithmetic rather than by the
    // stream state it moves — measured: scenes whose surface table stays in L2 (+10 % on the Cornell room, 34 triangles) while
    // millions of streams are alive; with the 69,564-triangle bunny it is neutral, and with few streams in flight it loses
    sc->shade_rounds = ((size_t)n_tris * 192 <= ((size_t)2 << 20)) ? -1 : 1;
    if (const char* m = getenv("PTAMD_TR")) { const int v = atoi(m); if (v >= -1 && v <= 1) sc->shade_rounds = v; }
    if (const char* m = getenv("PTAMD_QUERY_QUAD")) sc->query_quad = atoi(m) != 0;
    sc->dev.nee_prune = (emitOk && pt_prune_allowed()) ? 1 : 0;
}

// The limits of the traversal kernels, for the tree of an upload and for a rebuilt one alike.  Host only.
int pt_tree_limits(const char* who, int depth, int quad_depth)
{
    if (depth > ptd::kStackDepth) {
        pt_set_error("%s: traversal tree depth %d exceeds the traversal stack (%d)", who, depth, ptd::kStackDepth);
        return PT_ERR_UNSUPPORTED;
    }
    if (3 * quad_depth + 2 > ptk_wf_stack_capacity()) {
        pt_set_error("%s: 4-wide traversal tree depth %d needs more than the %d stack entries of the traversal kernel", who, quad_depth, ptk_wf_stack_capacity());
        return PT_ERR_UNSUPPORTED;
    }
    return PT_OK;
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
    int rc;
    if ((rc = validate_tree(nodes, n_nodes, n_tris)) != PT_OK) return rc;
    // ---- traversal tree over the triangles (host/accel_build.cpp) ----
    PtAccel accel;
    pt_build_accel(nodes, n_nodes, tris, n_tris, accel);
    if ((rc = pt_tree_limits("pt_scene_create", accel.depth, accel.quad_depth)) != PT_OK) return rc;
    std::vector<float> surf, lights, core;
    std::vector<int32_t> light_prim;
    std::vector<uint8_t> small;
    pack_surfaces(tris, n_tris, surf, lights, light_prim);
    const int n_lights = (int)light_prim.size();
    bool triOk;
    const bool emitOk = emittance_ok(tris, n_tris, spheres, n_spheres, triOk);
    core_box(tris, n_tris, core, small);
    std::vector<float> sph = pack_spheres(spheres, n_spheres);

    HIPCHK(hipSetDevice(device));
    // from here on every failure deletes the half-built scene (geometry already uploaded, events, streams)
    std::unique_ptr<PtScene> sc(new PtScene());
    sc->device = device;
    sc->n_lights = n_lights;
    sc->max_depth = accel.depth;
    auto host = [](const auto& v) { return HostArray{v.data(), v.size() * sizeof(v[0])}; };
    HostArray src[kSceneArrays];
    src[kArrNodes] = host(accel.wide); src[kArrQuad] = host(accel.quad); src[kArrTri] = host(accel.tri); src[kArrTripair] = host(accel.tripair);
    src[kArrLeafbox] = host(accel.leafbox); src[kArrSurf] = host(surf); src[kArrLights] = host(lights); src[kArrSpheres] = host(sph);
    src[kArrCore] = host(core);
    if ((rc = upload_arrays(sc.get(), src)) != PT_OK) return rc;
    std::vector<float> uv((size_t)n_tris * 6);
    for (int i = 0; i < n_tris; i++) { const PtTriangle& t = tris[i]; const float c[6] = {t.u0, t.v0, t.u1, t.v1, t.u2, t.v2}; memcpy(&uv[(size_t)i * 6], c, sizeof(c)); }
    HIPCHK(sc->uv.upload(uv.data(), uv.size() * sizeof(float)));
    sc->bytes += (int64_t)sc->uv.held();
    if ((rc = create_resources(sc.get())) != PT_OK) return rc;
    apply_defaults(sc.get(), n_tris, emitOk);
    sc->tri_emit_ok = triOk;
    sc->dev.n_quad = accel.n_quad; sc->dev.quad_depth = accel.quad_depth;
    sc->dev.n_nodes = accel.n_wide; sc->dev.n_tris = n_tris; sc->dev.n_lights = n_lights; sc->dev.n_spheres = n_spheres;
    // what a vertex update needs later: the sphere records and the maps of the build (uploaded by the first update)
    sc->h_spheres.swap(sph);
    PtScene::DynHost& dh = sc->dyn_host;
    dh.bn.swap(accel.bn); dh.order.swap(accel.order); dh.level_start.swap(accel.level_start); dh.wide_bn.swap(accel.wide_bn);
    dh.quad_bn.swap(accel.quad_bn); dh.leaf_range.swap(accel.leaf_range); dh.tmap.swap(accel.tmap); dh.light_prim.swap(light_prim);
    if (!core.empty()) dh.small.swap(small);
    dh.pos.resize((size_t)n_tris * 9);      // a triangle that becomes a light needs V1 and V2 themselves: V0 + E1 is not V1
    for (int i = 0; i < n_tris; i++) memcpy(&dh.pos[(size_t)i * 9], &tris[i], 36);      // V0 V1 V2 are the first nine floats of a PtTriangle
    dh.area_sum = accel.area_sum;
    sc->dyn.n_bn = (int32_t)(dh.bn.size() / 4); sc->dyn.n_wide = accel.n_wide; sc->dyn.n_quad = accel.n_quad; sc->dyn.n_tris = n_tris;
    sc->dyn.n_leaves = accel.n_leaves; sc->dyn.n_lights = n_lights;
    *out = sc.release();
    return PT_OK;
}

void pt_scene_destroy(PtScene* s)
{
    if (!s) return;
    (void)hipSetDevice(s->device);
    delete s;
}

int32_t pt_scene_num_lights(const PtScene* s) { return s ? s->n_lights : 0; }
int64_t pt_scene_device_bytes(const PtScene* s) { return s ? s->bytes : 0; }

int pt_scene_tree_info(const PtScene* s, PtTreeInfo* out)
{
    if (!s || !out) { pt_set_error("pt_scene_tree_info: NULL %s", !s ? "scene" : "out"); return PT_ERR_INVALID; }
    out->n_wide = s->dev.n_nodes; out->n_quad = s->dev.n_quad; out->depth = s->max_depth; out->quad_depth = s->dev.quad_depth; out->rebuilds = s->rebuilds;
    return PT_OK;
}

int pt_dbg_tree_limits(int32_t depth, int32_t quad_depth, int32_t* max_depth, int32_t* max_quad_depth)
{
    if (max_depth) *max_depth = ptd::kStackDepth;
    if (max_quad_depth) *max_quad_depth = (ptk_wf_stack_capacity() - 2) / 3;
    return pt_tree_limits("pt_dbg_tree_limits", depth, quad_depth);
}

int64_t pt_dbg_scene_array(PtScene* s, int32_t which, void* h_out, int64_t cap_bytes)
{
    if (!s || which < 0 || which > 8 || cap_bytes < 0 || (cap_bytes > 0 && !h_out)) {
        pt_set_error("pt_dbg_scene_array: %s", !s ? "NULL scene" : (which < 0 || which > 8) ? "which must be 0..8" : "bad output buffer");
        return PT_ERR_INVALID;
    }
    // `lights` keeps its largest size through the material updates, `nodes` and `quad` have worst-case room once a tree rebuild has
    // run: what a render reads is the current number of records
    const int64_t size = which == kArrLights ? (int64_t)s->n_lights * 64 : which == kArrNodes ? (int64_t)s->dev.n_nodes * 64 :
                         which == kArrQuad ? (int64_t)s->dev.n_quad * 64 : (int64_t)s->arr[which].bytes();
    const int64_t n = size < cap_bytes ? size : cap_bytes;
    if (n > 0) {
        HIPCHK(hipSetDevice(s->device));
        HIPCHK(hipDeviceSynchronize());
        HIPCHK(hipMemcpy(h_out, s->arr[which].as<>(), (size_t)n, hipMemcpyDeviceToHost));
    }
    return size;
}

}  // extern "C"
static_assert(kSceneArrays == 9, "pt_dbg_scene_array documents which = 0..8 (include/pt_api.h, ptamd.SCENE_ARRAYS)");
