// pt_rays.hip — radiance along the caller's own rays (include/pt_api.h: pt_render_rays and friends).  DESIGN.md section 17.
//
// Ray i takes the place of a pixel: the render differs from a camera's in one kernel (pt_wavefront.hip: wf_init_rays seeds a stream and
// takes its primary ray from the caller's RAY8 buffer) and in where a sample that restarts at the cached first hit reads its origin
// (pt_stream.h: RayTable, the same buffer).  Streams are laid out in groups of 64 rays, a group being what a tile is to a frame, so the
// per-pass means and their sum are already in ray order: nothing comes after the pipeline but the sum of the passes.  This file holds
// the checks and the launch sequence; it has no device code.
#include <hip/hip_runtime.h>

#include "pt_scene.h"

// Every host-side check of a ray render (include/pt_api.h), before any HIP call, and the DevParams of it: a world of one whose "frame"
// has ceil(n / 64) tiles — the pipeline only counts units.
static int rays_params(const char* who, const PtParams* prm, int64_t n_rays, ptd::DevParams& d)
{
    if (!prm) { pt_set_error("%s: NULL params", who); return PT_ERR_INVALID; }
    if (n_rays < 1) { pt_set_error("%s: n_rays=%lld", who, (long long)n_rays); return PT_ERR_INVALID; }
    if (pt_check_params(prm)) return PT_ERR_INVALID;
    if (prm->rank != 0 || prm->world != 1) { pt_set_error("%s: rays are rendered with rank 0 of world 1: rank=%d world=%d", who, prm->rank, prm->world); return PT_ERR_INVALID; }
    // what a single frame of that many tiles may have: pt_render_tiles' own limit on the units, and 64 streams per unit below 2^31
    // (bit 31 of a ray-queue entry is the resume flag)
    const int64_t groups = (n_rays + 63) / 64;
    if (groups > 0x7fffffffLL || groups * prm->passes > 0x7fffffffLL || groups * prm->passes * 64 >= (1LL << 31)) {
        pt_set_error("%s: %lld rays x %d passes: too many work units for one pipeline run (64 x ceil(n / 64) x passes must stay below 2^31)", who, (long long)n_rays, prm->passes);
        return PT_ERR_INVALID;
    }
    ptd::path_params(prm, d);
    d.rank = 0; d.world = 1;
    d.tiles_x = (int)groups; d.tiles_y = 1; d.n_tiles_total = (int)groups; d.n_tiles_local = (int)groups;
    d.n_units = (int)(groups * prm->passes);
    d.unit_base = 0;
    return PT_OK;
}

static int rays_args(const char* who, const PtScene* s, const float* rays, int64_t n_rays, int32_t seed_stride, const PtParams* prm, const float* rgb,
                     const void* work, bool device, ptd::DevParams& d)
{
    const char* bad = !s ? "NULL scene" : !rays ? "NULL rays" : !rgb ? "NULL rgb" : (device && !work) ? "NULL work buffer" :
                      seed_stride < 0 ? "seed_stride < 0" :
                      (device && ((uintptr_t)rays & 15)) ? "rays must be 16-byte aligned" :
                      (device && ((uintptr_t)rgb & 15)) ? "rgb must be 16-byte aligned" : nullptr;
    if (bad) { pt_set_error("%s: %s", who, bad); return PT_ERR_INVALID; }
    return rays_params(who, prm, n_rays, d);
}

extern "C" {

int64_t pt_rays_floats(int64_t n_rays)
{
    if (n_rays < 1 || n_rays > (int64_t)1 << 31) { pt_set_error("pt_rays_floats: n_rays=%lld", (long long)n_rays); return -1; }      // beyond 2^31 rays no call can render them
    return (n_rays + 63) / 64 * ptd::kTilePixels * 3;
}

int64_t pt_rays_work_bytes(const PtParams* prm, int64_t n_rays)
{
    ptd::DevParams d;
    if (rays_params("pt_rays_work_bytes", prm, n_rays, d)) return -1;
    return pt_job_work_bytes(d);
}

int pt_render_rays(PtScene* s, const float* d_rays8, const int32_t* d_seed, int64_t n_rays, int32_t seed_stride, const PtParams* prm,
                   float* d_rgb, void* d_work, void* hip_stream)
{
    ptd::WfJob job{};
    const int rc = rays_args("pt_render_rays", s, d_rays8, n_rays, seed_stride, prm, d_rgb, d_work, true, job.prm);
    if (rc) return rc;
    if (!pt_has_light(s)) return PT_ERR_NO_LIGHT;
    job.stream = (hipStream_t)hip_stream;
    HIPCHK(hipSetDevice(s->device));
    // always the queue-driven pipeline (pt_set_mode, the counting build and the PTAMD_TSTAT diagnostics do not apply); the rays and seeds
    // are read where they are for as long as the call blocks: nothing is copied, nothing is allocated in the scene
    job.work = d_work;
    job.src.kind = ptd::WfSource::kRays;
    job.src.rays = {(const float4*)d_rays8, d_seed, seed_stride, (uint32_t)n_rays};
    return pt_run_job(s, job, /*traceEvents=*/false, /*traceStat=*/false, d_rgb);
}

int pt_render_rays_host(PtScene* s, const float* h_rays8, const int32_t* h_seed, int64_t n_rays, int32_t seed_stride, const PtParams* prm,
                        float* h_rgb)
{
    ptd::DevParams d;
    const int rc = rays_args("pt_render_rays_host", s, h_rays8, n_rays, seed_stride, prm, h_rgb, nullptr, false, d);
    if (rc) return rc;
    HIPCHK(hipSetDevice(s->device));
    DevBuf d_rays, d_seed, d_rgb, d_work;      // d_seed stays null when the caller gave no seeds
    HIPCHK(d_rays.upload(h_rays8, (size_t)n_rays * 32));
    if (h_seed) HIPCHK(d_seed.upload(h_seed, (size_t)n_rays * 4));
    HIPCHK(d_rgb.alloc((size_t)pt_rays_floats(n_rays) * 4));
    HIPCHK(d_work.alloc((size_t)pt_job_work_bytes(d)));
    const int r = pt_render_rays(s, d_rays.as<float>(), d_seed.as<int32_t>(), n_rays, seed_stride, prm, d_rgb.as<float>(), d_work.as<>(), nullptr);
    if (r) return r;
    HIPCHK(hipMemcpy(h_rgb, d_rgb.as<>(), (size_t)n_rays * 12, hipMemcpyDeviceToHost));      // the NULL stream: after the sum of the passes
    return PT_OK;
}

}  // extern "C"
