// pt_api.hip — the render half of the C-ABI (include/pt_api.h): the checks and the geometry of a render call, the launch sequence of the
// tile, tile-list and view-batch renders (the ray render's is in pt_rays.hip), tile gather helpers, timing and diagnostics, parity hooks.  The scene is built in pt_scene.hip;
// every other feature's entry points sit beside its kernels (pt_denoise.hip, pt_stats.hip, pt_region.hip, pt_dynamic.hip, pt_query.hip, pt_rays.hip).
//
// Replaces the render half of PathTracer::Render (srcs/pathtracer.cu:124-259): instead of NUM_MULTI_SAMPLE synchronous launches there is
// one persistent launch over all (tile, pass) units on the caller's stream.  This file holds no device code.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "pt_scene.h"

template <class F>
static int with_buffers(int device, const void* in, size_t in_bytes, void* out, size_t out_bytes, void* out2, size_t out2_bytes, F launch)
{
    HIPCHK(hipSetDevice(device));
    DevBuf d_in, d_out, d_out2;
    HIPCHK(d_in.upload(in, in_bytes));
    HIPCHK(d_out.alloc(out_bytes));
    HIPCHK(d_out2.alloc(out2_bytes));
    HIPCHK(launch(d_in.as<>(), d_out.as<>(), d_out2.as<>()));
    HIPCHK(hipDeviceSynchronize());
    if (out_bytes) HIPCHK(hipMemcpy(out, d_out.as<>(), out_bytes, hipMemcpyDeviceToHost));
    if (out2_bytes) HIPCHK(hipMemcpy(out2, d_out2.as<>(), out2_bytes, hipMemcpyDeviceToHost));
    return PT_OK;
}

// persistent grid of the traversal kernel: 256 CUs x 7 blocks of 4 waves = 7 waves/SIMD, what its 72 VGPRs allow
// (PTAMD_TB overrides, tuning only; measured: 1536 blocks -3 %, 1024 blocks -22 %)
static const int kTraceBlocks = (getenv("PTAMD_TB") && atoi(getenv("PTAMD_TB")) >= 1) ? (atoi(getenv("PTAMD_TB")) > 16384 ? 16384 : atoi(getenv("PTAMD_TB"))) : 1792;

// ---- geometry of the tile split --------------------------------------------------------
int pt_check_params(const PtParams* prm)
{
    // the limits of the packed stream state (pt_stream.h: store_state)
    if (prm->spp_per_pass > 65535) { pt_set_error("params out of range: spp_per_pass=%d, at most 65535", prm->spp_per_pass); return PT_ERR_INVALID; }
    if (prm->max_bounce > 255) { pt_set_error("params out of range: max_bounce=%d, at most 255", prm->max_bounce); return PT_ERR_INVALID; }
    if (prm->max_refract < 0 || prm->max_refract > 250) { pt_set_error("params out of range: max_refract=%d, 0 .. 250", prm->max_refract); return PT_ERR_INVALID; }
    if (prm->passes < 1 || prm->spp_per_pass < 1 || prm->max_bounce < 1 || prm->world < 1 || prm->rank < 0 || prm->rank >= prm->world) {
        pt_set_error("bad params: passes=%d spp_per_pass=%d max_bounce=%d rank=%d world=%d", prm->passes, prm->spp_per_pass, prm->max_bounce, prm->rank, prm->world);
        return PT_ERR_INVALID;
    }
    return PT_OK;
}

int pt_fill_params(const PtCamera* cam, const PtParams* prm, ptd::DevParams& d)
{
    if (!cam || !prm) { pt_set_error("NULL camera/params"); return PT_ERR_INVALID; }
    if (cam->W < 2 || cam->H < 2) { pt_set_error("frame %dx%d too small (W-1, H-1 divide, srcs/pathtracer.cu:35-36)", cam->W, cam->H); return PT_ERR_INVALID; }
    if (pt_check_params(prm)) return PT_ERR_INVALID;
    if (!ptd::seed_in_range(cam, prm->first_pass, prm->passes)) return PT_ERR_INVALID;
    ptd::path_params(prm, d);
    d.rank = prm->rank; d.world = prm->world;
    const ptd::TileGrid g = ptd::tile_grid(cam->W, cam->H, prm->world);
    d.tiles_x = g.tiles_x; d.tiles_y = g.tiles_y; d.n_tiles_total = g.total; d.n_tiles_local = g.per_rank;
    const long long units = (long long)d.n_tiles_local * prm->passes;
    if (units > 0x7fffffffLL) { pt_set_error("too many work units"); return PT_ERR_INVALID; }
    d.n_units = (int)units;
    d.unit_base = 0;
    return PT_OK;
}

// srcs/pathtracer.cu:193-198 and :35-36 — the per-launch camera constants, tan/atan2 as correctly rounded float functions
void pt_fill_camera(const PtCamera* cam, ptd::DevCamera& c)
{
    memcpy(c.pos, cam->pos, 12); memcpy(c.forward, cam->forward, 12); memcpy(c.up, cam->up, 12); memcpy(c.right, cam->right, 12);
    c.W = cam->W; c.H = cam->H;
    const float fovy = cam->fovy_deg * 0.01745329251994329576923690768489f;                 // glm::radians
    const float fovx = 2.f * (float)std::atan2((double)((float)std::tan((double)(fovy * 0.5f)) * cam->aspect), 1.0);
    c.tan_half_fovx = (float)std::tan((double)(fovx * 0.5f));
    c.tan_half_fovy = (float)std::tan((double)(fovy * 0.5f));
}

int pt_upload_views(PtScene* s, const PtCamera* h_cams, int32_t n_views, int32_t default_first, const int32_t* h_first_pass, hipStream_t stream,
                    PtViewTable& t)
{
    HIPCHK(s->views.reserve(n_views, 64, 16 + sizeof(ptd::DevCamera) + 4));
    // origins | cameras | first passes, each n_views long, packed for one copy (16-byte entries first: every part stays aligned)
    const size_t offCam = (size_t)n_views * 16, offFirst = offCam + (size_t)n_views * sizeof(ptd::DevCamera), total = offFirst + (size_t)n_views * 4;
    s->h_views.resize(total);
    for (int32_t v = 0; v < n_views; v++) {
        ptd::DevCamera c;
        pt_fill_camera(&h_cams[v], c);
        const float org[4] = {c.pos[0], c.pos[1], c.pos[2], 0.f};
        const int32_t first = h_first_pass ? h_first_pass[v] : default_first;
        memcpy(s->h_views.data() + (size_t)v * 16, org, 16);
        memcpy(s->h_views.data() + offCam + (size_t)v * sizeof(ptd::DevCamera), &c, sizeof(c));
        memcpy(s->h_views.data() + offFirst + (size_t)v * 4, &first, 4);
    }
    HIPCHK(hipMemcpyAsync(s->views.as<>(), s->h_views.data(), total, hipMemcpyHostToDevice, stream));
    const char* dv = s->views.as<const char>();
    t = {(const ptd::DevCamera*)(dv + offCam), (const int32_t*)(dv + offFirst), (const float4*)dv};
    return PT_OK;
}

extern "C" {

int64_t pt_tiles_floats(const PtCamera* cam, const PtParams* prm)
{
    ptd::DevParams d;
    if (pt_fill_params(cam, prm, d)) return -1;
    return (int64_t)d.n_tiles_local * ptd::kTilePixels * 3;
}
// d_work of a render of d: the per-pass means of the one-kernel mode or the pipeline's buffers, whichever is larger
int64_t pt_job_work_bytes(const ptd::DevParams& d)
{
    const int64_t means = (int64_t)d.n_tiles_local * ptd::kTilePixels * 3 * 4 * d.passes;
    const int64_t wave = (int64_t)ptk_wf_work_bytes((size_t)d.n_units, kTraceBlocks);
    return means > wave ? means : wave;
}
int64_t pt_work_bytes(const PtCamera* cam, const PtParams* prm)
{
    ptd::DevParams d;
    if (pt_fill_params(cam, prm, d)) return -1;
    return pt_job_work_bytes(d);
}

bool pt_has_light(const PtScene* s)      // false: PT_ERR_NO_LIGHT, with the error text set
{
    if (s->n_lights < 1) pt_set_error("scene has no emissive triangle: the reference's `curand(s) %% Nl` is undefined (include/CudaUtil.cuh:235)");
    return s->n_lights >= 1;
}

// The one way into the queue-driven pipeline (pt_wavefront.hip), for an entry point that has checked its arguments, made the scene's device current
// and filled in what to render (prm, work, stream) and from which pixels and cameras (src).  Lends the job the scene's resources and runs it — the pipeline polls the live-stream count,
// so this returns once the render has drained — then sums the passes into d_tiles.  traceEvents: record the per-launch events of
// pt_enable_trace_timing.  traceStat: the PTAMD_TSTAT diagnostics apply (wf_trace counts its trips and the lanes they serve; pt_last_counters).
int pt_run_job(PtScene* s, ptd::WfJob& job, bool traceEvents, bool traceStat, float* d_tiles)
{
    const int slot = s->ev_count % PtScene::kEvRing;
    job.scene = &s->dev; job.traceBlocks = kTraceBlocks; job.lent = &s->wf;
    job.ev_begin = s->ev[slot][0]; job.ev_end = s->ev[slot][1];
    job.drainBelow = s->drain_below; job.shadeRounds = s->shade_rounds; job.earlyBelow = s->early_below;
    if (traceEvents && !s->trace_ev.empty()) { job.trace_ev = s->trace_ev.data(); job.trace_ev_triples = (int)s->trace_ev.size() / 3; }
    s->trace_ev_used = 0;
    job.trace_ev_used = &s->trace_ev_used;
    if (traceStat && ptk_wf_trace_stat() != 0) {
        HIPCHK(hipMemsetAsync(s->counters.as<>(), 0, ptd::kStatBytes, job.stream));
        job.traceStat = s->counters.as<unsigned long long>();
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
    if (!pt_has_light(s)) return PT_ERR_NO_LIGHT;
    ptd::WfJob job{};
    ptd::DevParams& d = job.prm;
    int rc = pt_fill_params(cam, prm, d);
    if (rc) return rc;
    job.src.kind = ptd::WfSource::kFrame;
    ptd::DevCamera& c = job.src.frame.cam;
    pt_fill_camera(cam, c);

    hipStream_t stream = (hipStream_t)hip_stream;
    HIPCHK(hipSetDevice(s->device));
    if (s->mode == 1 && !s->count_next) {
        // the only entry point that honours pt_set_mode(0), the counting build and the PTAMD_TSTAT diagnostics
        job.work = d_work; job.stream = stream;
        return pt_run_job(s, job, /*traceEvents=*/true, /*traceStat=*/true, d_tiles);
    }
    const int slot = s->ev_count % PtScene::kEvRing;
    HIPCHK(hipMemsetAsync(s->unit_counter.as<>(), 0, 4, stream));
    if (s->count_next) HIPCHK(hipMemsetAsync(s->counters.as<>(), 0, 64, stream));
    // persistent grid: 4 blocks of 4 waves per CU (16 waves/CU; register- and LDS-feasible), never more blocks than units need
    int blocks = s->num_cus * 4;
    const int need = (d.n_units + ptd::kWavesPerBlock - 1) / ptd::kWavesPerBlock;
    if (blocks > need) blocks = need;
    if (blocks < 1) blocks = 1;
    // events bracket exactly the render_units launch (the dominant kernel), on the launch stream
    HIPCHK(hipEventRecord(s->ev[slot][0], stream));
    HIPCHK(ptk_render_units(&s->dev, &c, &d, (float*)d_work, s->unit_counter.as<unsigned int>(), s->counters.as<>(), blocks, s->count_next ? 1 : 0, stream));
    HIPCHK(hipEventRecord(s->ev[slot][1], stream));
    s->ev_count++;
    HIPCHK(ptk_sum_passes((const float*)d_work, d.passes, (long long)d.n_tiles_local * ptd::kTilePixels * 3, d_tiles, stream));
    return PT_OK;
}

// ---- a list of tiles instead of a rank's fixed share (csrc/pt_region.hip has the window helpers and the scatter) ----------------
// DevParams of a list render: a world of one whose "frame" has n_tiles tiles — the pipeline only counts units; the pixels come from the list
static int fill_list_params(const PtCamera* cam, const PtParams* prm, int32_t n_tiles, ptd::DevParams& d)
{
    const int rc = pt_fill_params(cam, prm, d);
    if (rc) return rc;
    if (prm->rank != 0 || prm->world != 1) { pt_set_error("a tile list is rendered with rank 0 of world 1 (split a frame by making lists): rank=%d world=%d", prm->rank, prm->world); return PT_ERR_INVALID; }
    if (n_tiles < 1 || n_tiles > d.n_tiles_total) { pt_set_error("n_tiles=%d: a list holds 1 .. %d tiles of a %dx%d frame", n_tiles, d.n_tiles_total, cam->W, cam->H); return PT_ERR_INVALID; }
    d.n_tiles_local = n_tiles;
    d.n_units = n_tiles * prm->passes;      // <= the full frame's, which pt_fill_params has bounded
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
    return pt_job_work_bytes(d);
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
    if (!pt_has_light(s)) return PT_ERR_NO_LIGHT;
    job.src.kind = ptd::WfSource::kTileList;
    pt_fill_camera(cam, job.src.list.cam);

    job.stream = (hipStream_t)hip_stream;
    HIPCHK(hipSetDevice(s->device));
    // the previous list render on this scene has drained (one render at a time per scene), so nothing reads the old buffer
    HIPCHK(s->tile_list.reserve(n_tiles, 1024, 4));
    // stream-ordered before wf_init_list; the render below returns only once it has drained, so h_tiles is not read after the call
    HIPCHK(hipMemcpyAsync(s->tile_list.as<>(), h_tiles, (size_t)n_tiles * 4, hipMemcpyHostToDevice, job.stream));
    // always the queue-driven pipeline (pt_set_mode, the counting build and the PTAMD_TSTAT diagnostics do not apply); no per-launch trace events
    job.work = d_work; job.src.list.tiles = s->tile_list.as<int32_t>();
    return pt_run_job(s, job, /*traceEvents=*/false, /*traceStat=*/false, d_tiles);
}

// ---- a batch of cameras in one pipeline run -----------------------------------------------------------------------------------------
// DevParams of a batch: a world of one whose "frame" has n_views x tiles tiles (tiles_x / tiles_y / n_tiles_total stay those of one view:
// wf_init_views turns a local tile into (view, tile of the view) with them) — the pipeline only counts units.  first_pass: the
// largest of the batch, so that pt_fill_params' seed limit covers every view (W and H are shared).
static int fill_views_params(const PtCamera* cam0, const PtParams* prm, int32_t n_views, int32_t max_first_pass, ptd::DevParams& d)
{
    if (!cam0 || !prm) { pt_set_error("NULL camera/params"); return PT_ERR_INVALID; }
    if (n_views < 1) { pt_set_error("n_views=%d: a batch holds at least one view", n_views); return PT_ERR_INVALID; }
    PtParams p = *prm; p.first_pass = max_first_pass;
    const int rc = pt_fill_params(cam0, &p, d);
    if (rc) return rc;
    if (prm->rank != 0 || prm->world != 1) { pt_set_error("a batch of views is rendered with rank 0 of world 1: rank=%d world=%d", prm->rank, prm->world); return PT_ERR_INVALID; }
    // what a single frame of that many tiles may have: pt_fill_params' own limit on the units, and 64 streams per unit below 2^31
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
    if (pt_fill_params(cam0, &p, d)) return -1;
    return (int64_t)n_views * d.n_tiles_total * ptd::kTilePixels * 3;
}

int64_t pt_views_work_bytes(const PtCamera* cam0, const PtParams* prm, int32_t n_views)
{
    ptd::DevParams d;
    if (fill_views_params(cam0, prm, n_views, prm ? prm->first_pass : 0, d)) return -1;
    return pt_job_work_bytes(d);
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
    if (!pt_has_light(s)) return PT_ERR_NO_LIGHT;
    job.stream = (hipStream_t)hip_stream;
    HIPCHK(hipSetDevice(s->device));
    // the previous batch on this scene has drained (one render at a time per scene), so nothing reads the old buffer;
    // stream-ordered before wf_init_views; the render below returns only once it has drained, so the callers' arrays are not read after the call
    PtViewTable t;
    const int urc = pt_upload_views(s, h_cams, n_views, prm->first_pass, h_first_pass, job.stream, t);
    if (urc) return urc;
    // always the queue-driven pipeline (pt_set_mode, the counting build and the PTAMD_TSTAT diagnostics do not apply); per-launch trace events as for a frame
    job.work = d_work;
    job.src.kind = ptd::WfSource::kViews;
    job.src.views = {t.cams, t.firstPass, t.org};
    return pt_run_job(s, job, /*traceEvents=*/true, /*traceStat=*/false, d_tiles);
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
    DevBuf d_tiles, d_work, d_frames;
    HIPCHK(d_tiles.alloc((size_t)nt * 4));
    HIPCHK(d_work.alloc((size_t)wb));
    HIPCHK(d_frames.alloc(frame * 4 * (size_t)n_views));
    rc = pt_render_views(s, h_cams, n_views, prm, h_first_pass, d_tiles.as<float>(), d_work.as<>(), nullptr);
    for (int32_t v = 0; v < n_views && !rc; v++) rc = pt_untile(d_tiles.as<float>() + (size_t)v * perView, &h_cams[v], 1, d_frames.as<float>() + (size_t)v * frame, nullptr);
    if (!rc) HIPCHK(hipMemcpy(h_rgb, d_frames.as<>(), frame * 4 * (size_t)n_views, hipMemcpyDeviceToHost));
    return rc;
}

int pt_untile(const float* d_gathered, const PtCamera* cam, int32_t world, float* d_frame_rgb, void* hip_stream)
{
    if (!d_gathered || !cam || !d_frame_rgb || world < 1) { pt_set_error("pt_untile: bad argument"); return PT_ERR_INVALID; }
    const ptd::TileGrid g = ptd::tile_grid(cam->W, cam->H, world);
    const long long per_rank = (long long)g.per_rank * ptd::kTilePixels * 3;
    HIPCHK(ptk_untile(d_gathered, cam->W, cam->H, g.tiles_x, g.total, world, per_rank, d_frame_rgb, (hipStream_t)hip_stream));
    return PT_OK;
}

int pt_untile_views(const float* d_tiles, const PtCamera* cam0, int32_t n_views, float* d_frames_rgb, void* hip_stream)
{
    if (!d_tiles || !cam0 || !d_frames_rgb || n_views < 1) { pt_set_error("pt_untile_views: bad argument"); return PT_ERR_INVALID; }
    if (!ptd::frame_ok(cam0->W, cam0->H) || (int64_t)n_views * cam0->W * cam0->H > ptd::kMaxPixels) {
        pt_set_error("pt_untile_views: %d views of %dx%d: a frame below 2x2 or more than 2^28 pixels", n_views, cam0->W, cam0->H);
        return PT_ERR_INVALID;
    }
    const ptd::TileGrid g = ptd::tile_grid(cam0->W, cam0->H);
    HIPCHK(ptk_untile_views(d_tiles, cam0->W, cam0->H, g.tiles_x, g.total, n_views, d_frames_rgb, (hipStream_t)hip_stream));
    return PT_OK;
}

int pt_render(PtScene* s, const PtCamera* cam, const PtParams* prm, float* h_accum_rgb)
{
    if (!s || !h_accum_rgb || !prm) { pt_set_error("pt_render: NULL argument"); return PT_ERR_INVALID; }
    PtParams p = *prm; p.rank = 0; p.world = 1;
    const int64_t nt = pt_tiles_floats(cam, &p), wb = pt_work_bytes(cam, &p);
    if (nt < 0 || wb < 0) return PT_ERR_INVALID;
    HIPCHK(hipSetDevice(s->device));
    DevBuf d_tiles, d_work, d_frame;
    HIPCHK(d_tiles.alloc((size_t)nt * 4));
    HIPCHK(d_work.alloc((size_t)wb));
    HIPCHK(d_frame.alloc((size_t)cam->W * cam->H * 12));
    int rc = pt_render_tiles(s, cam, &p, d_tiles.as<float>(), d_work.as<>(), nullptr);
    if (!rc) rc = pt_untile(d_tiles.as<float>(), cam, 1, d_frame.as<float>(), nullptr);
    if (!rc) HIPCHK(hipMemcpy(h_accum_rgb, d_frame.as<>(), (size_t)cam->W * cam->H * 12, hipMemcpyDeviceToHost));
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
    HIPCHK(hipMemcpy(out8, s->counters.as<>(), 64, hipMemcpyDeviceToHost));
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
    s->trace_ev_used = 0;
    return PT_OK;
}
static int kernel_timing(PtScene* s, int first, double* sum_ms, int32_t* launches, double* max_ms)
{
    if (!s || !sum_ms || !launches) { pt_set_error("pt_trace_timing / pt_shade_timing: NULL"); return PT_ERR_INVALID; }
    HIPCHK(hipSetDevice(s->device));
    double sum = 0, mx = 0;
    for (int i = 0; i < s->trace_ev_used; i++) {
        const size_t k = (size_t)i * 3 + (size_t)first;
        float ms = 0.f;
        HIPCHK(hipEventSynchronize(s->trace_ev[k + 1]));
        HIPCHK(hipEventElapsedTime(&ms, s->trace_ev[k], s->trace_ev[k + 1]));
        sum += ms; if (ms > mx) mx = ms;
    }
    *sum_ms = sum; *launches = s->trace_ev_used; if (max_ms) *max_ms = mx;
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
    auto read = [&](void* dst, size_t byteOff, size_t bytes) { return hipMemcpy(dst, s->counters.as<const char>() + byteOff, bytes, hipMemcpyDeviceToHost); };
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

// ---- parity hooks ------------------------------------------------------------------------
int pt_dbg_raycast(PtScene* s, const float* rays8, int32_t n, float* out_hits29, int32_t* out_prim)
{
    if (!s || !rays8 || n < 0 || !out_hits29 || !out_prim) { pt_set_error("pt_dbg_raycast: bad argument"); return PT_ERR_INVALID; }
    return with_buffers(s->device, rays8, (size_t)n * 32, out_hits29, (size_t)n * 29 * 4, out_prim, (size_t)n * 4,
                        [&](void* i, void* o, void* o2) { return ptk_dbg_raycast(&s->dev, s->uv.as<float>(), (const float*)i, n, (float*)o, (int*)o2, nullptr); });
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
int pt_dbg_pixel_dir(int32_t device, const PtCamera* cam, const int32_t* pxpypass, int32_t n, float* out8)
{
    if (!cam || !pxpypass || !out8 || n < 0 || cam->W < 2 || cam->H < 2) { pt_set_error("pt_dbg_pixel_dir: bad argument"); return PT_ERR_INVALID; }
    ptd::DevCamera c;
    pt_fill_camera(cam, c);
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
