// pt_aov.hip — first-hit feature buffers over any pixel source (include/pt_api.h: pt_render_aov_window, pt_render_aov_views, pt_aov_rays).
// DESIGN.md section 28.  pt_render_aov (the full frame of one camera; entry point and definition of the eight floats in
// csrc/pt_denoise.hip) runs this file's kernel over the window of all its pixels; the same kernel computes them for a pixel window, for
// a batch of camera views and for the caller's own rays, bit for bit what pt_render_aov gives the same pixel (a ray: what one pass of
// it would give; the oracle pins the bits, tests/test_denoise.py).  Nothing here touches a render's state.
//
// One kernel, aov_source<SRC, QUAD>: one primary ray per lane, a wave is one 8x8 tile of the source's tile grid or 64 consecutive
// rays, workgroups are ONE wave as in pt_query.hip (a finished wave frees its slot at once).  SRC says where a lane's rays come from
// (aov_place / aov_primary are overloaded for it, as camera_origin is in pt_stream.h); QUAD picks the walk exactly as pt_trace_rays does:
// ray_setup + quad_step over the 4-wide tree with the 40-entry per-lane LDS stack when the tree fits it, else trace_closest on the binary
// tree.  Per pixel: the render's seed expression, two jitter draws inside pixel_direction,
// origin cam.pos, t_max 999999, float32 sums in pass order from 0, IEEE divisions at the end.  A ray runs the same expressions with one
// pass and draws nothing.  Only the nine accumulators live across a walk; make_surf follows it inside the pass loop.
#include <hip/hip_runtime.h>
#include "pt_device.h"
#include "pt_math.h"
#include "pt_bxdf.h"
#include "pt_trace.h"
#include "pt_shade.h"
#include "pt_scene.h"

namespace ptd {

// What a lane keeps to make its primary ray of pass j: its pixel and camera (the camera is the same for the whole wave), or the ray itself.
struct AovPixel { DevCamera cam; int px, py, first; };
struct AovRay { f3 org, dir; float tmax; };

// A pixel window of one camera.  Unit u is tile (tx0 + u % tiles_w, ty0 + u / tiles_w) of the FULL frame's tile grid, over the tiles
// that overlap the window; the output is window-relative, row-major.  The window lies inside the frame (checked on the host), so a
// lane inside it is inside the frame.  The whole frame as the window is pt_render_aov's own pixel set.
struct AovWindow {
    using Lane = AovPixel;
    DevCamera cam;
    int32_t first_pass, passes;
    int32_t x0, y0, x1, y1;
    int32_t tx0, ty0, tiles_w;
};
// A batch of views of one size.  Unit u -> (view = u / tilesPerView, tile of the view); camera and first pass from the table
// pt_render_views uploads (csrc/pt_api.hip: pt_upload_views); the output is view-major.
struct AovViews {
    using Lane = AovPixel;
    const DevCamera* cams;
    const int32_t* firstPass;
    int32_t passes, tiles_x;
    uint32_t tilesPerView;
};
// The caller's RAY8 records: lane i of the grid is ray i.  One "pass", no RNG.
struct AovRays {
    using Lane = AovRay;
    const float4* rays;
    uint32_t n;
};

// The lane's place in its source: false = the lane retires (outside the window, the frame or the ray set).  out = index of its record.
PT_DEV bool aov_place(const AovWindow& s, uint32_t unit, int lane, AovPixel& p, int& passes, size_t& out)
{
    p.px = (s.tx0 + (int)(unit % (uint32_t)s.tiles_w)) * kTile + (lane & 7);
    p.py = (s.ty0 + (int)(unit / (uint32_t)s.tiles_w)) * kTile + (lane >> 3);
    if (p.px < s.x0 || p.px >= s.x1 || p.py < s.y0 || p.py >= s.y1) return false;
    p.cam = s.cam; p.first = s.first_pass; passes = s.passes;
    out = (size_t)(p.py - s.y0) * (size_t)(s.x1 - s.x0) + (size_t)(p.px - s.x0);
    return true;
}
PT_DEV bool aov_place(const AovViews& s, uint32_t unit, int lane, AovPixel& p, int& passes, size_t& out)
{
    const uint32_t view = unit / s.tilesPerView, tile = unit % s.tilesPerView;
    p.cam = s.cams[view];
    p.px = (int)(tile % (uint32_t)s.tiles_x) * kTile + (lane & 7);
    p.py = (int)(tile / (uint32_t)s.tiles_x) * kTile + (lane >> 3);
    if (p.px >= p.cam.W || p.py >= p.cam.H) return false;
    p.first = s.firstPass[view]; passes = s.passes;
    out = (size_t)view * (size_t)p.cam.W * (size_t)p.cam.H + (size_t)p.py * (size_t)p.cam.W + (size_t)p.px;
    return true;
}
PT_DEV bool aov_place(const AovRays& s, uint32_t unit, int lane, AovRay& r, int& passes, size_t& out)
{
    const uint32_t i = unit * 64u + (uint32_t)lane;
    if (i >= s.n) return false;
    const float4 a = s.rays[2 * (size_t)i], b = s.rays[2 * (size_t)i + 1];      // org.xyz dir.x | dir.yz reserved tmax
    r.org = f3(a.x, a.y, a.z); r.dir = f3(a.w, b.x, b.y); r.tmax = b.w;
    passes = 1;
    out = i;
    return true;
}

// The primary ray of the lane's j-th pass: StartRender's expressions for a pixel (srcs/pathtracer.cu:70-74), the record itself for a ray.
PT_DEV void aov_primary(const AovPixel& p, int j, f3& org, f3& dir, float& tmax)
{
    const int pass = p.first + j;
    Rng rng;
    rng.init((uint64_t)(int64_t)(p.py * p.cam.W + p.px + pass * p.cam.W * p.cam.H));      // srcs/pathtracer.cu:70-71
    float u1, u2;
    dir = pixel_direction(p.cam, p.px, p.py, rng, u1, u2);
    org = f3(p.cam.pos[0], p.cam.pos[1], p.cam.pos[2]);
    tmax = 999999.f;
}
PT_DEV void aov_primary(const AovRay& r, int, f3& org, f3& dir, float& tmax) { org = r.org; dir = r.dir; tmax = r.tmax; }

template <class SRC, bool QUAD>
__global__ __launch_bounds__(64, kQueryWaves)
void aov_source(DevScene sc, SRC src, float4* __restrict__ aov, int* __restrict__ prim_out)
{
    __shared__ int lds_stack[(QUAD ? kQueryStack : kStackDepth) * 64];
    typename SRC::Lane ln;
    int passes;
    size_t i;
    if (!aov_place(src, blockIdx.x, (int)threadIdx.x, ln, passes, i)) return;
    int* stack = &lds_stack[threadIdx.x];
    f3 alb(0.f, 0.f, 0.f), nrm(0.f, 0.f, 0.f);
    float tsum = 0.f;
    int hits = 0, prim0 = -1;
    for (int j = 0; j < passes; j++) {
        f3 org, dir; float t;
        aov_primary(ln, j, org, dir, t);
        int prim;
        if (QUAD) {
            f3 inv; float cscale; bool degenerate;
            ray_setup(dir, inv, cscale, degenerate);
            int cur = 0, sp = 0;
            prim = -1;
            while (!quad_step(sc, org, dir, inv, cscale, degenerate, -__builtin_inff(), stack, cur, sp, t, prim)) {}
            spheres_closest<false>(sc, org, dir, t, prim);
        } else {
            TraceStats st{0, 0, 0};
            const float tmax = t;
            prim = trace_closest<false>(sc, org, dir, tmax, stack, t, st);
        }
        if (j == 0) prim0 = prim;
        if (prim >= 0) {
            Surf s;
            make_surf(sc, prim, t, org, dir, s);
            alb += s.m.albedo;
            nrm += s.fr.n;
            tsum += t;
            hits++;
        }
    }
    const float fp = (float)passes;
    aov[2 * i] = make_float4(alb.x / fp, alb.y / fp, alb.z / fp, nrm.x / fp);
    aov[2 * i + 1] = make_float4(nrm.y / fp, nrm.z / fp, hits ? tsum / (float)hits : 0.f, (float)hits / fp);
    if (prim_out) prim_out[i] = prim0;
}

}  // namespace ptd

// `units` one-wave workgroups of src on `stream`; the walk is chosen as pt_trace_rays chooses it (pt_scene.h: pt_query_walks_quad)
template <class SRC>
static hipError_t launch_aov(const PtScene* s, const SRC& src, uint32_t units, float* d_aov, int32_t* d_prim, hipStream_t stream)
{
    if (pt_query_walks_quad(s)) hipLaunchKernelGGL((ptd::aov_source<SRC, true>), dim3(units), dim3(64), 0, stream, s->dev, src, (float4*)d_aov, d_prim);
    else hipLaunchKernelGGL((ptd::aov_source<SRC, false>), dim3(units), dim3(64), 0, stream, s->dev, src, (float4*)d_aov, d_prim);
    return hipGetLastError();
}

// ---- entry points (include/pt_api.h): every argument check comes before the first HIP call ----------------------------------------
static int out_args(const char* who, const PtScene* s, const float* aov)
{
    if (!s || !aov) { pt_set_error("%s: NULL argument", who); return PT_ERR_INVALID; }
    if ((uintptr_t)aov % 16) { pt_set_error("%s: d_aov is not 16-byte aligned", who); return PT_ERR_INVALID; }
    return PT_OK;
}

static int window_aov_args(const char* who, const PtCamera* cam, const PtParams* prm, int32_t x0, int32_t y0, int32_t x1, int32_t y1)
{
    int rc = pt_aov_args(cam, prm);
    if (!rc) rc = pt_window_args(who, cam, x0, y0, x1, y1);
    return rc;
}

// the checks of pt_render_views that bear on feature buffers (only passes and first_pass of prm are read), and the pixel limit of the batch
static int views_aov_args(const char* who, const PtCamera* h_cams, int32_t n_views, const PtParams* prm, const int32_t* h_first_pass)
{
    if (!h_cams || !prm) { pt_set_error("%s: NULL argument", who); return PT_ERR_INVALID; }
    if (n_views < 1) { pt_set_error("%s: n_views=%d", who, n_views); return PT_ERR_INVALID; }
    for (int32_t v = 0; v < n_views; v++) {
        if (h_cams[v].W != h_cams[0].W || h_cams[v].H != h_cams[0].H) {
            pt_set_error("%s: view %d is %dx%d, view 0 is %dx%d (all views of a batch share W and H)", who, v, h_cams[v].W, h_cams[v].H, h_cams[0].W, h_cams[0].H);
            return PT_ERR_INVALID;
        }
        if (h_first_pass && h_first_pass[v] < 0) { pt_set_error("%s: first_pass of view %d is %d", who, v, h_first_pass[v]); return PT_ERR_INVALID; }
        PtParams p = *prm;
        if (h_first_pass) p.first_pass = h_first_pass[v];
        const int rc = pt_aov_args(&h_cams[v], &p);      // the frame, passes >= 1, first_pass >= 0, the seed limit of this view
        if (rc) return rc;
    }
    if ((int64_t)n_views * h_cams[0].W * h_cams[0].H > ptd::kMaxPixels) {
        pt_set_error("%s: %d views of %dx%d are more than 2^28 pixels", who, n_views, h_cams[0].W, h_cams[0].H);
        return PT_ERR_INVALID;
    }
    return PT_OK;
}

static int rays_aov_args(const char* who, const PtScene* s, const float* rays, int64_t n, const float* aov, const int32_t* prim, bool device)
{
    const char* bad = !s ? "NULL scene" : !rays ? "NULL rays" : !aov ? "NULL aov" : n < 0 ? "n < 0" :
                      (device && ((uintptr_t)rays & 15)) ? "rays must be 16-byte aligned" :
                      (device && ((uintptr_t)aov & 15)) ? "aov must be 16-byte aligned" :
                      (device && ((uintptr_t)prim & 3)) ? "prim must be 4-byte aligned" : nullptr;
    if (bad) { pt_set_error("%s: %s", who, bad); return PT_ERR_INVALID; }
    return PT_OK;
}

extern "C" {

int64_t pt_aov_window_floats(const PtCamera* cam, int32_t x0, int32_t y0, int32_t x1, int32_t y1)
{
    if (!cam || !ptd::frame_ok(cam->W, cam->H)) { pt_set_error("pt_aov_window_floats: bad camera"); return -1; }
    if (pt_window_args("pt_aov_window_floats", cam, x0, y0, x1, y1)) return -1;
    return (int64_t)(y1 - y0) * (x1 - x0) * 8;
}

int pt_render_aov_window(PtScene* s, const PtCamera* cam, const PtParams* prm, int32_t x0, int32_t y0, int32_t x1, int32_t y1,
                         float* d_aov, int32_t* d_prim, void* hip_stream)
{
    int rc = out_args("pt_render_aov_window", s, d_aov);
    if (!rc) rc = window_aov_args("pt_render_aov_window", cam, prm, x0, y0, x1, y1);
    if (rc) return rc;
    ptd::AovWindow src;
    pt_fill_camera(cam, src.cam);
    src.first_pass = prm->first_pass; src.passes = prm->passes;
    src.x0 = x0; src.y0 = y0; src.x1 = x1; src.y1 = y1;
    src.tx0 = x0 / ptd::kTile; src.ty0 = y0 / ptd::kTile;
    src.tiles_w = (x1 - 1) / ptd::kTile - src.tx0 + 1;
    const int tiles_h = (y1 - 1) / ptd::kTile - src.ty0 + 1;
    HIPCHK(hipSetDevice(s->device));
    HIPCHK(launch_aov(s, src, (uint32_t)(src.tiles_w * tiles_h), d_aov, d_prim, (hipStream_t)hip_stream));
    return PT_OK;
}

int pt_aov_window(PtScene* s, const PtCamera* cam, const PtParams* prm, int32_t x0, int32_t y0, int32_t x1, int32_t y1, float* h_aov, int32_t* h_prim)
{
    if (!s || !h_aov) { pt_set_error("pt_aov_window: NULL argument"); return PT_ERR_INVALID; }
    int rc = window_aov_args("pt_aov_window", cam, prm, x0, y0, x1, y1);
    if (rc) return rc;
    const size_t n = (size_t)(y1 - y0) * (size_t)(x1 - x0);
    HIPCHK(hipSetDevice(s->device));
    DevBuf d_aov, d_prim;      // d_prim stays null when the caller asked for no primitive ids
    HIPCHK(d_aov.alloc(n * 32));
    if (h_prim) HIPCHK(d_prim.alloc(n * 4));
    rc = pt_render_aov_window(s, cam, prm, x0, y0, x1, y1, d_aov.as<float>(), d_prim.as<int32_t>(), nullptr);
    if (rc) return rc;
    HIPCHK(hipMemcpy(h_aov, d_aov.as<>(), n * 32, hipMemcpyDeviceToHost));
    if (h_prim) HIPCHK(hipMemcpy(h_prim, d_prim.as<>(), n * 4, hipMemcpyDeviceToHost));
    return PT_OK;
}

int64_t pt_aov_views_floats(const PtCamera* cam0, int32_t n_views)
{
    if (!cam0 || !ptd::frame_ok(cam0->W, cam0->H) || n_views < 1 || (int64_t)n_views * cam0->W * cam0->H > ptd::kMaxPixels) {
        pt_set_error("pt_aov_views_floats: bad camera, n_views=%d, or more than 2^28 pixels", n_views);
        return -1;
    }
    return (int64_t)n_views * cam0->W * cam0->H * 8;
}

int pt_render_aov_views(PtScene* s, const PtCamera* h_cams, int32_t n_views, const PtParams* prm, const int32_t* h_first_pass,
                        float* d_aov, int32_t* d_prim, void* hip_stream)
{
    int rc = out_args("pt_render_aov_views", s, d_aov);
    if (!rc) rc = views_aov_args("pt_render_aov_views", h_cams, n_views, prm, h_first_pass);
    if (rc) return rc;
    hipStream_t stream = (hipStream_t)hip_stream;
    HIPCHK(hipSetDevice(s->device));
    PtViewTable t;
    rc = pt_upload_views(s, h_cams, n_views, prm->first_pass, h_first_pass, stream, t);
    if (rc) return rc;
    // unlike a render, this call does not block until its kernel is done: the scene's host image of the table (and the callers' arrays)
    // are free once the copy has run
    HIPCHK(hipStreamSynchronize(stream));
    const ptd::TileGrid g = ptd::tile_grid(h_cams[0].W, h_cams[0].H);
    ptd::AovViews src;
    src.cams = t.cams; src.firstPass = t.firstPass;
    src.passes = prm->passes; src.tiles_x = g.tiles_x; src.tilesPerView = (uint32_t)g.total;
    HIPCHK(launch_aov(s, src, (uint32_t)n_views * (uint32_t)g.total, d_aov, d_prim, stream));
    return PT_OK;
}

int pt_aov_views(PtScene* s, const PtCamera* h_cams, int32_t n_views, const PtParams* prm, const int32_t* h_first_pass, float* h_aov, int32_t* h_prim)
{
    if (!s || !h_aov) { pt_set_error("pt_aov_views: NULL argument"); return PT_ERR_INVALID; }
    int rc = views_aov_args("pt_aov_views", h_cams, n_views, prm, h_first_pass);
    if (rc) return rc;
    const size_t n = (size_t)n_views * (size_t)h_cams[0].W * (size_t)h_cams[0].H;
    HIPCHK(hipSetDevice(s->device));
    DevBuf d_aov, d_prim;
    HIPCHK(d_aov.alloc(n * 32));
    if (h_prim) HIPCHK(d_prim.alloc(n * 4));
    rc = pt_render_aov_views(s, h_cams, n_views, prm, h_first_pass, d_aov.as<float>(), d_prim.as<int32_t>(), nullptr);
    if (rc) return rc;
    HIPCHK(hipMemcpy(h_aov, d_aov.as<>(), n * 32, hipMemcpyDeviceToHost));
    if (h_prim) HIPCHK(hipMemcpy(h_prim, d_prim.as<>(), n * 4, hipMemcpyDeviceToHost));
    return PT_OK;
}

int pt_aov_rays(PtScene* s, const float* d_rays8, int64_t n_rays, float* d_aov, int32_t* d_prim, void* hip_stream)
{
    const int rc = rays_aov_args("pt_aov_rays", s, d_rays8, n_rays, d_aov, d_prim, true);
    if (rc) return rc;
    if (n_rays == 0) return PT_OK;
    HIPCHK(hipSetDevice(s->device));
    HIPCHK(pt_query_batches(n_rays, [&](int64_t off, uint32_t m) {
        const ptd::AovRays src{(const float4*)(d_rays8 + off * 8), m};
        return launch_aov(s, src, (m + 63u) / 64u, d_aov + off * 8, d_prim ? d_prim + off : nullptr, (hipStream_t)hip_stream);
    }));
    return PT_OK;
}

int pt_aov_rays_host(PtScene* s, const float* h_rays8, int64_t n_rays, float* h_aov, int32_t* h_prim)
{
    int rc = rays_aov_args("pt_aov_rays_host", s, h_rays8, n_rays, h_aov, h_prim, false);
    if (rc) return rc;
    if (n_rays == 0) return PT_OK;
    HIPCHK(hipSetDevice(s->device));
    DevBuf d_rays, d_aov, d_prim;
    HIPCHK(d_rays.upload(h_rays8, (size_t)n_rays * 32));
    HIPCHK(d_aov.alloc((size_t)n_rays * 32));
    if (h_prim) HIPCHK(d_prim.alloc((size_t)n_rays * 4));
    if ((rc = pt_aov_rays(s, d_rays.as<float>(), n_rays, d_aov.as<float>(), d_prim.as<int32_t>(), nullptr)) != PT_OK) return rc;
    HIPCHK(hipMemcpy(h_aov, d_aov.as<>(), (size_t)n_rays * 32, hipMemcpyDeviceToHost));
    if (h_prim) HIPCHK(hipMemcpy(h_prim, d_prim.as<>(), (size_t)n_rays * 4, hipMemcpyDeviceToHost));
    return PT_OK;
}

}  // extern "C"
