// pt_internal.h — what crosses translation units inside libptamd.so, on the host side: error reporting, the owner of a device allocation,
// the small facts every entry point states the same way (tile grid, seed range), the argument blocks of the wavefront pipeline and of the
// vertex update, and the prototype of every ptk_* launcher that is called from another file.  Included by the files that define these
// functions and by those that call them, so a signature that drifts is a compile error (with C linkage it would link and run).  Not part
// of the C-ABI.  The scene itself (struct PtScene) is in pt_scene.h.
#pragma once
#include <hip/hip_runtime.h>
#include <utility>

#include "../../include/pt_api.h"
#include "pt_device.h"

void pt_set_error(const char* fmt, ...);   // pt_host.cpp

#define HIPCHK(expr)                                                                        \
    do {                                                                                    \
        hipError_t e_ = (expr);                                                             \
        if (e_ != hipSuccess) {                                                             \
            pt_set_error("HIP error %d at %s:%d '%s': %s", (int)e_, __FILE__, __LINE__, #expr, hipGetErrorString(e_)); \
            return PT_ERR_DEVICE;                                                           \
        }                                                                                   \
    } while (0)

// Owner of one hipMalloc'ed block: whatever path leaves its scope, the block is freed.  Move-only (its move members delete the copies).  alloc(0) holds 16 bytes (a kernel
// argument is never a null array) and remembers 0 as the size asked for.  A DevBuf that was never allocated is a null pointer.
class DevBuf {
public:
    DevBuf() = default;
    DevBuf(DevBuf&& o) noexcept : p_(std::exchange(o.p_, nullptr)), bytes_(std::exchange(o.bytes_, 0)) {}
    DevBuf& operator=(DevBuf&& o) noexcept { std::swap(p_, o.p_); std::swap(bytes_, o.bytes_); return *this; }
    ~DevBuf() { release(); }
    void release() { if (p_) (void)hipFree(p_); p_ = nullptr; bytes_ = 0; }      // the device of the allocation is the current one
    hipError_t alloc(size_t bytes)
    {
        release();
        const hipError_t e = hipMalloc(&p_, bytes ? bytes : 16);
        if (e == hipSuccess) bytes_ = bytes; else p_ = nullptr;
        return e;
    }
    // alloc + one synchronous copy of `bytes` from the host
    hipError_t upload(const void* h, size_t bytes)
    {
        const hipError_t e = alloc(bytes);
        return (e != hipSuccess || !bytes) ? e : hipMemcpy(p_, h, bytes, hipMemcpyHostToDevice);
    }
    // grow-on-demand: room for `count` elements of `elem` bytes, at least `min` of them when it has to allocate.  The old block is
    // freed first, so the caller must know that nothing on the device still reads it.
    hipError_t reserve(int64_t count, int64_t min, size_t elem)
    {
        if (p_ && bytes_ >= (size_t)count * elem) return hipSuccess;
        return alloc((size_t)(count < min ? min : count) * elem);
    }
    template <class T = void> T* as() const { return (T*)p_; }
    explicit operator bool() const { return p_ != nullptr; }
    size_t bytes() const { return bytes_; }                               // as asked for
    size_t held() const { return p_ ? (bytes_ ? bytes_ : 16) : 0; }      // as allocated
private:
    void* p_ = nullptr;
    size_t bytes_ = 0;
};

namespace ptd {

// The 8x8 tile grid of a W x H frame, and a rank's share of it when `world` ranks split the frame.
struct TileGrid { int tiles_x, tiles_y, total, per_rank; };
inline TileGrid tile_grid(int W, int H, int world = 1)
{
    TileGrid g;
    g.tiles_x = (W + kTile - 1) / kTile;
    g.tiles_y = (H + kTile - 1) / kTile;
    g.total = g.tiles_x * g.tiles_y;
    g.per_rank = (g.total + world - 1) / world;
    return g;
}

// The frames (and stacks of frames) the feature buffers and the denoiser take: every per-pixel float offset (x 8) stays inside int64
// and the pixel index inside int
constexpr int64_t kMaxPixels = (int64_t)1 << 28;
inline bool frame_ok(int32_t W, int32_t H) { return W >= 2 && H >= 2 && (int64_t)W * H <= kMaxPixels; }

// The render seeds a pixel's stream with offset + SampleIDX * W * H as an int: false, with the error text set, when the last pass overflows it.
inline bool seed_in_range(const PtCamera* cam, int first_pass, int passes)
{
    const bool ok = (long long)cam->W * cam->H * (long long)(first_pass + passes) <= 0x7fffffffLL;
    if (!ok) pt_set_error("offset + SampleIDX*W*H overflows int (srcs/pathtracer.cu:71)");
    return ok;
}

// The seven path parameters every render copies from the caller's PtParams as they are (the geometry of the units is each entry point's own).
inline void path_params(const PtParams* prm, DevParams& d)
{
    d.passes = prm->passes; d.spp_per_pass = prm->spp_per_pass; d.max_bounce = prm->max_bounce; d.rr_bounce = prm->rr_bounce;
    d.rr_floor = prm->rr_floor; d.max_refract = prm->max_refract; d.first_pass = prm->first_pass;
}

// What a scene lends every run of the wavefront pipeline, for the scene's life: early shade's second stream with the events that order
// it and the caller's stream, and the pinned word the host polls the live-stream count through.  One render at a time per scene.
struct WfLent {
    hipStream_t aux = nullptr;                                       // non-blocking: wf_shade PHASE 1 runs here beside the draining wf_trace
    hipEvent_t toAux[2] = {nullptr, nullptr};                        // main -> aux: the previous iteration's shade is done, by iteration parity (no timing)
    hipEvent_t toMain[2] = {nullptr, nullptr};                       // aux -> main: PHASE 1 is done, by iteration parity (no timing)
    uint32_t* h_poll = nullptr;                                      // pinned
    WfLent() = default;
    WfLent(const WfLent&) = delete;
    WfLent& operator=(const WfLent&) = delete;
    hipError_t create()                                              // once; the device is the current one
    {
        hipError_t e = hipStreamCreateWithFlags(&aux, hipStreamNonBlocking);
        for (int k = 0; k < 2 && e == hipSuccess; k++) {
            e = hipEventCreateWithFlags(&toAux[k], hipEventDisableTiming);
            if (e == hipSuccess) e = hipEventCreateWithFlags(&toMain[k], hipEventDisableTiming);
        }
        return e != hipSuccess ? e : hipHostMalloc((void**)&h_poll, 64, hipHostMallocDefault);
    }
    ~WfLent()
    {
        if (h_poll) (void)hipHostFree(h_poll);
        for (int k = 0; k < 2; k++) { if (toAux[k]) (void)hipEventDestroy(toAux[k]); if (toMain[k]) (void)hipEventDestroy(toMain[k]); }
        if (aux) (void)hipStreamDestroy(aux);
    }
};

// Where a stream's pixel and camera come from: the kind, and the fields of that kind alone.  Each render entry point fills in its own.
struct WfSource {
    enum Kind {
        kFrame,      // pt_render_tiles: the fixed share of prm.rank / world (wf_init)
        kTileList,   // pt_render_tile_list: prm.n_tiles_local global tile numbers (wf_init_list); nothing else of the pipeline differs from kFrame
        kViews,      // pt_render_views: a batch, n_tiles_local = views x prm.n_tiles_total; wf_init_views, the ViewTable instantiations of wf_shade / wf_drain
        kRays,       // pt_render_rays: n_tiles_local = ceil(nRays / 64) groups of 64 rays; wf_init_rays, the RayTable instantiations
    } kind;
    union {
        struct { DevCamera cam; } frame;
        struct { DevCamera cam; const int32_t* tiles; } list;                                        // tiles: on the device
        struct { const DevCamera* cams; const int32_t* firstPass; const float4* org; } views;        // one device entry per view
        struct { const float4* rays8; const int32_t* seed; int32_t seedStride; uint32_t nRays; } rays;      // rays8: the caller's device buffer (also the origin table); seed may be nullptr (seed of ray i = i)
    };
};

// One run of the wavefront pipeline (ptk_wf_render, pt_wavefront.hip).  An entry point fills in what is its own (prm, work, stream, src)
// and pt_run_job (pt_api.hip) the rest; the pipeline reads it and writes through the two output pointers only.
struct WfJob {
    // ---- what to render
    const DevScene* scene;
    DevParams prm;                       // n_units (tile, pass) units; a list, a batch or a ray set: a world of one whose frame has n_tiles_local tiles
    void* work;                          // ptk_wf_work_bytes(prm.n_units, traceBlocks) bytes; the per-pass means end up at its start (ptk_wf_staging)
    int traceBlocks;                     // persistent grid of wf_trace
    hipStream_t stream;                  // the caller's
    WfSource src;
    // ---- what the scene lends
    const WfLent* lent;
    hipEvent_t ev_begin, ev_end;         // bracket the whole render on `stream`
    // ---- schedule (PtScene: drain_below, shade_rounds, early_below)
    int drainBelow, shadeRounds, earlyBelow;
    // ---- diagnostics, optional
    hipEvent_t* trace_ev;                // triples (before wf_trace, after it, after wf_shade), one per iteration; nullptr = none
    int trace_ev_triples;
    unsigned long long* traceStat;       // the counter buffer (PTAMD_TSTAT), cleared by the caller; nullptr = the production wf_trace
    // ---- out
    int* trace_ev_used;                  // triples recorded
    int* iters;                          // bounce iterations
};

// ---- argument block of the vertex update (pt_dynamic.hip) ----
constexpr int kCoreBlocks = 256;         // partial boxes of the core-box reduction (one per workgroup)

// Device pointers of one scene: the arrays a render reads (rewritten by an update), the maps of the build (host/accel_build.h,
// read only) and the update's scratch.  "Builder node" = node of the binary traversal tree in the builder's numbering, 0 = root.
struct DynScene {
    // rewritten
    float4* nodes; uint4* quad; float4* tri; float4* tripair; float4* leafbox; float4* surf; float4* lights; float* core;
    // maps
    const int4* bn;              // per builder node: l, r, first, count (count > 0: leaf over tree-order triangles first .. first + count)
    const int32_t* order;        // builder nodes sorted by height
    const int2* wide_bn;         // per `nodes` record: builder node of its L / R box
    const int4* quad_bn;         // per `quad` record: builder node of each child, -1 = none
    const int2* leaf_range;      // per reference leaf: first triangle (reference order), count
    const int2* tmap;            // per tree-order triangle: prim (reference order), reference leaf
    const int32_t* light_prim;   // per light: prim
    const uint8_t* small;        // per prim: 1 = classified small at upload (core box), nullptr when the scene has no core box
    // scratch
    float4* bbox;                // per builder node: unpadded box, mn.xyz 0 | mx.xyz 0
    float* maxabs;               // largest |coordinate| of the root box
    float* core_partial;         // kCoreBlocks x 8 floats
    double* area_partial;        // one block sum per kAreaBlock builder nodes
    int32_t n_bn, n_wide, n_quad, n_tris, n_leaves, n_lights;
};

}  // namespace ptd

// pt_api.hip: the checks and the geometry of a render call; the per-launch camera constants
int pt_check_params(const PtParams* prm);                        // the parameter ranges alone (prm not NULL), the error text set
int pt_fill_params(const PtCamera* cam, const PtParams* prm, ptd::DevParams& d);
void pt_fill_camera(const PtCamera* cam, ptd::DevCamera& c);
// pt_denoise.hip: what every feature-buffer call asks of its camera and params (the frame, passes >= 1, first_pass >= 0, the seed limit)
int pt_aov_args(const PtCamera* cam, const PtParams* prm);
// pt_region.hip: a half-open window inside the frame of cam (not NULL, W and H >= 2), the error text set
int pt_window_args(const char* who, const PtCamera* cam, int32_t x0, int32_t y0, int32_t x1, int32_t y1);

extern "C" {
// pt_api.hip
int64_t pt_job_work_bytes(const ptd::DevParams& d);      // d_work of a render of d
bool pt_has_light(const PtScene* s);                     // false: PT_ERR_NO_LIGHT is due, the error text set
int pt_run_job(PtScene* s, ptd::WfJob& job, bool traceEvents, bool traceStat, float* d_tiles);      // the one way into the queue-driven pipeline
// pt_kernels.hip
hipError_t ptk_render_units(const ptd::DevScene*, const ptd::DevCamera*, const ptd::DevParams*, float*, unsigned int*, void*, int, int, hipStream_t);
hipError_t ptk_sum_passes(const float*, int, long long, float*, hipStream_t);
hipError_t ptk_untile(const float*, int, int, int, int, int, long long, float*, hipStream_t);
hipError_t ptk_untile_views(const float* tiles, int W, int H, int tiles_x, int n_tiles_total, int n_views, float* frames, hipStream_t);
hipError_t ptk_dbg_raycast(const ptd::DevScene*, const float* uv, const float*, int, float*, int*, hipStream_t);
hipError_t ptk_dbg_bxdf(int, const float*, int, float*, hipStream_t);
hipError_t ptk_dbg_rng(unsigned long long, int, uint32_t*, float*, hipStream_t);
hipError_t ptk_dbg_math(const float*, int, float*, hipStream_t);
hipError_t ptk_dbg_sincos(const float*, int, float*, hipStream_t);
// pt_wavefront.hip
hipError_t ptk_dbg_ray_setup(const float*, int, float*, hipStream_t);
hipError_t ptk_dbg_pixel_dir(const ptd::DevCamera*, const int*, int, float*, hipStream_t);
hipError_t ptk_dbg_nee(const ptd::DevScene*, const float*, int, float*, hipStream_t);
size_t ptk_wf_work_bytes(size_t nUnits, int traceBlocks);
const float* ptk_wf_staging(void* work);
int ptk_wf_stack_capacity(void);
int ptk_wf_trace_stat(void);      // PTAMD_TSTAT as the pipeline read it (0 = off)
hipError_t ptk_wf_render(const ptd::WfJob& job);
}
