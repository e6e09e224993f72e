// pt_denoise.hip — first-hit feature buffers ("AOVs") of the full frame and the edge-aware denoiser guided by them (include/pt_api.h:
// pt_render_aov, pt_denoise).  New ground: the reference has neither.  Nothing here touches a render's state.
//
// AOVs: per pixel of the full frame, the camera ray of the FIRST path of each pass first_pass + j of the call
// (the render's seed expression, two jitter draws, pixel_direction, origin cam.pos, t_max 999999 — as dbg_pixel_dir), traced to
// its closest hit and given its surface by make_surf (as dbg_raycast).  Float32 sums in pass order, one IEEE division at the end:
//   [0..2] sum albedo / passes   [3..5] sum shading normal (ray-facing, not renormalised) / passes
//   [6] sum t / hits (0 if none) [7] hits / passes
// The host restates it bit for bit from the oracle (tests/denoise_ref.py: aov_from_oracle).  The kernel is pt_aov.hip's, which takes its
// pixels from any source: the full frame is the window of all its pixels (measured against the kernel this file used to hold, one
// wave per tile in 256-thread workgroups on trace_closest: 0.89 against 2.91 ms at 1080p).
//
// Denoiser: edge-avoiding a-trous wavelet filter (Dammertz et al. 2010) with albedo demodulation.  Definition (tests/denoise_ref.py
// states it in numpy twice: `denoise` in float64, `denoise32` in float32 with every operation rounded once in the order of the code
// below — on inputs whose every exp argument is 0 the kernels return denoise32's bits, tests/test_denoise_exact.py).  The albedo is
// compared in float32 against the float32 nearest 1e-3 (1e-3f = 0.001000000047...: that value and below divide by 1); the cutoff is
// inclusive (E == 80 is used, a NaN E is not); a NaN in the normal, or a depth of +inf, makes every E of the pixel NaN, so it keeps its
// value and is nobody's tap; max(z_p, z_q) is the select of the code below and adds a depth term only when > 0 (misses, negative
// depths: none; a NaN depth as a tap: none); kc = 0 (sc^2 overflows) switches the colour term off, kc = inf (sc^2 underflows, or kc
// overflows on the way) makes the centre tap's 0 * inf NaN and keeps every finite pixel (include/pt_api.h has all of it).
//   c_p = rgb_p / sample_cnt;  div_p = albedo_p where > 1e-3f else 1 (per channel; 1 without demodulation);  e_p = c_p / div_p
//   finite_p = all three components of c_p are finite (after an iteration: of e'_p)
//   iteration i = 0 .. L-1, step s = 2^i, taps q = p + s (dx, dy), dx, dy in -2..2 (dy outer, dx inner), inside the frame and finite_q:
//     w = h(dx) h(dy) exp(-E),  h = (1/16, 1/4, 3/8, 1/4, 1/16)
//     E = |e_p - e_q|^2 / (sc^2 4^-i)  (left out when !finite_p)  + |n_p - n_q|^2 / sn^2
//       + |z_p - z_q| / (sz max(z_p, z_q))  (0 when both depths are 0);   w = 0 exactly when E > 80
//   e'_p = sum w e_q / sum w, or e_p when sum w = 0 (a NaN pixel with a finite neighbour becomes finite; a NaN is never spread);
//   n (AOV 3..5) and z (AOV 6) are not filtered;  out_p = e_p^(L) div_p sample_cnt;  L = 0 is a plain copy.
// A stack of n frames of one size (pt_denoise_batch) is filtered by the same launches: the frame is blockIdx.z, every buffer is offset by
// frame x W*H at the top of a kernel, and a tap is tested against the frame's own W and H — it never crosses into a neighbour.
// Kernels: pack (demodulate once: colour float4 (e.rgb, finite), feature float4 (n.xyz, z)), L x atrous (ping-pong of the colour
// float4s in the work buffer), finish (remodulate, write RGB).  256-thread blocks, each wave an 8x8 pixel tile, plain 16-byte loads:
// the 48 B/pixel working set (100 MB at 1080p) stays in the Infinity Cache, the 5x5 footprint of a wave in L2.
#include <hip/hip_runtime.h>
#include <cmath>
#include "pt_device.h"
#include "pt_math.h"
#include "pt_scene.h"

namespace ptd {

// pixel of this thread: blocks of 16x16 pixels, wave w of the block on the 8x8 quadrant (w & 1, w >> 1); blockIdx.z is the frame of a
// stack, `frame` the index of its pixel 0
PT_DEV void dn_pixel(int W, int H, int& px, int& py, size_t& frame)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    px = blockIdx.x * 16 + (wave & 1) * kTile + (lane & 7);
    py = blockIdx.y * 16 + (wave >> 1) * kTile + (lane >> 3);
    frame = (size_t)blockIdx.z * (size_t)W * (size_t)H;
}

PT_DEV bool finite3(float a, float b, float c) { return __builtin_isfinite(a) && __builtin_isfinite(b) && __builtin_isfinite(c); }

PT_DEV f3 demod_div(const float4 a0, int demodulate)
{
    if (!demodulate) return f3(1.f, 1.f, 1.f);
    return f3(a0.x > 1e-3f ? a0.x : 1.f, a0.y > 1e-3f ? a0.y : 1.f, a0.z > 1e-3f ? a0.z : 1.f);
}

__global__ __launch_bounds__(256)
void dn_pack(const float* __restrict__ rgb, const float4* __restrict__ aov, int W, int H, float sample_cnt, int demodulate,
             float4* __restrict__ color, float4* __restrict__ feat)
{
    int px, py; size_t frame; dn_pixel(W, H, px, py, frame);
    if (px >= W || py >= H) return;
    const size_t i = frame + (size_t)py * W + px;
    const float4 a0 = aov[2 * i], a1 = aov[2 * i + 1];
    const f3 c(rgb[3 * i] / sample_cnt, rgb[3 * i + 1] / sample_cnt, rgb[3 * i + 2] / sample_cnt);
    const f3 d = demod_div(a0, demodulate);
    color[i] = make_float4(c.x / d.x, c.y / d.y, c.z / d.z, finite3(c.x, c.y, c.z) ? 1.f : 0.f);
    feat[i] = make_float4(a0.w, a1.x, a1.y, a1.z);
}

// one a-trous iteration at step s; kc = 4^i / sc^2, kn = 1 / sn^2, kz = 1 / sz
__global__ __launch_bounds__(256)
void dn_atrous(const float4* __restrict__ cin, const float4* __restrict__ feat, int W, int H, int s, float kc, float kn, float kz,
               float4* __restrict__ cout)
{
    int px, py; size_t frame; dn_pixel(W, H, px, py, frame);
    if (px >= W || py >= H) return;
    const float h[5] = {1.f / 16.f, 1.f / 4.f, 3.f / 8.f, 1.f / 4.f, 1.f / 16.f};
    const size_t i = frame + (size_t)py * W + px;
    const float4 cp = cin[i], fp = feat[i];
    const bool finP = cp.w != 0.f;
    float ax = 0.f, ay = 0.f, az = 0.f, wsum = 0.f;
#pragma unroll
    for (int dy = -2; dy <= 2; dy++) {
        const int qy = py + s * dy;
        if (qy < 0 || qy >= H) continue;
#pragma unroll
        for (int dx = -2; dx <= 2; dx++) {
            const int qx = px + s * dx;
            if (qx < 0 || qx >= W) continue;
            const size_t q = frame + (size_t)qy * W + qx;
            const float4 cq = cin[q];
            if (cq.w == 0.f) continue;
            const float4 fq = feat[q];
            float E = 0.f;
            if (finP) {
                const float ex = cp.x - cq.x, ey = cp.y - cq.y, ez = cp.z - cq.z;
                E = (ex * ex + ey * ey + ez * ez) * kc;
            }
            const float nx = fp.x - fq.x, ny = fp.y - fq.y, nz = fp.z - fq.z;
            E += (nx * nx + ny * ny + nz * nz) * kn;
            const float mz = fp.w > fq.w ? fp.w : fq.w;
            if (mz > 0.f) E += __builtin_fabsf(fp.w - fq.w) * kz / mz;
            if (!(E <= 80.f)) continue;                  // weight exactly 0
            const float w = (h[dx + 2] * h[dy + 2]) * expf(-E);
            ax += w * cq.x; ay += w * cq.y; az += w * cq.z;
            wsum += w;
        }
    }
    float4 o = cp;
    if (wsum > 0.f) {
        o.x = ax / wsum; o.y = ay / wsum; o.z = az / wsum;
        o.w = finite3(o.x, o.y, o.z) ? 1.f : 0.f;
    }
    cout[i] = o;
}

__global__ __launch_bounds__(256)
void dn_finish(const float4* __restrict__ color, const float4* __restrict__ aov, int W, int H, float sample_cnt, int demodulate,
               float* __restrict__ out)
{
    int px, py; size_t frame; dn_pixel(W, H, px, py, frame);
    if (px >= W || py >= H) return;
    const size_t i = frame + (size_t)py * W + px;
    const float4 e = color[i];
    const f3 d = demod_div(aov[2 * i], demodulate);
    out[3 * i] = (e.x * d.x) * sample_cnt;
    out[3 * i + 1] = (e.y * d.y) * sample_cnt;
    out[3 * i + 2] = (e.z * d.z) * sample_cnt;
}

}  // namespace ptd

// ---- entry points (include/pt_api.h): every argument check comes before the first HIP call ----------------------------------------
using ptd::frame_ok;
using ptd::kMaxPixels;

int pt_aov_args(const PtCamera* cam, const PtParams* prm)
{
    if (!cam || !prm) { pt_set_error("NULL camera/params"); return PT_ERR_INVALID; }
    if (!frame_ok(cam->W, cam->H)) { pt_set_error("frame %dx%d out of range", cam->W, cam->H); return PT_ERR_INVALID; }
    if (prm->passes < 1 || prm->first_pass < 0) { pt_set_error("bad params: passes=%d first_pass=%d", prm->passes, prm->first_pass); return PT_ERR_INVALID; }
    if (!ptd::seed_in_range(cam, prm->first_pass, prm->passes)) return PT_ERR_INVALID;
    return PT_OK;
}

static bool overlaps(const void* a, size_t na, const void* b, size_t nb)
{
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + nb && y < x + na;
}

// n_frames frames of W x H, stacked: the checks of one frame with every extent multiplied by n_frames
static int denoise_args(const void* rgb, const void* aov, int32_t W, int32_t H, int32_t n_frames, int32_t sample_cnt, const PtDenoiseParams* p,
                        const void* out, const void* work, bool device)
{
    if (!rgb || !aov || !p || !out || (device && !work)) { pt_set_error("pt_denoise: NULL argument"); return PT_ERR_INVALID; }
    if (!frame_ok(W, H)) { pt_set_error("pt_denoise: frame %dx%d out of range", W, H); return PT_ERR_INVALID; }
    if (n_frames < 1 || n_frames > 65535 || (int64_t)n_frames * W * H > kMaxPixels) {
        pt_set_error("pt_denoise: %d frames of %dx%d: 1 .. 65535 frames, at most 2^28 pixels in all", n_frames, W, H); return PT_ERR_INVALID;
    }
    if (sample_cnt <= 0) { pt_set_error("pt_denoise: sample_cnt %d <= 0", sample_cnt); return PT_ERR_INVALID; }
    if (p->iterations < 0 || p->iterations > 12) { pt_set_error("pt_denoise: iterations %d outside 0..12", p->iterations); return PT_ERR_INVALID; }
    if (!(p->sigma_color > 0.f) || !(p->sigma_normal > 0.f) || !(p->sigma_depth > 0.f) ||
        !std::isfinite(p->sigma_color) || !std::isfinite(p->sigma_normal) || !std::isfinite(p->sigma_depth)) {
        pt_set_error("pt_denoise: sigmas must be finite and > 0"); return PT_ERR_INVALID;
    }
    const size_t n = (size_t)W * H * (size_t)n_frames;
    if (overlaps(out, n * 12, rgb, n * 12) || overlaps(out, n * 12, aov, n * 32) || (work && overlaps(out, n * 12, work, n * 48))) {
        pt_set_error("pt_denoise: the output overlaps an input or the work buffer"); return PT_ERR_INVALID;
    }
    if (device && (((uintptr_t)aov % 16) || ((uintptr_t)work % 16) || overlaps(work, n * 48, rgb, n * 12) || overlaps(work, n * 48, aov, n * 32))) {
        pt_set_error("pt_denoise: d_aov / d_work not 16-byte aligned, or d_work overlaps an input"); return PT_ERR_INVALID;
    }
    return PT_OK;
}

extern "C" {

int64_t pt_aov_floats(const PtCamera* cam)
{
    if (!cam || !frame_ok(cam->W, cam->H)) { pt_set_error("pt_aov_floats: bad camera"); return -1; }
    return (int64_t)cam->W * cam->H * 8;
}

int pt_render_aov(PtScene* s, const PtCamera* cam, const PtParams* prm, float* d_aov, int32_t* d_prim, void* hip_stream)
{
    if (!s || !d_aov) { pt_set_error("pt_render_aov: NULL argument"); return PT_ERR_INVALID; }
    if ((uintptr_t)d_aov % 16) { pt_set_error("pt_render_aov: d_aov is not 16-byte aligned"); return PT_ERR_INVALID; }
    int rc = pt_aov_args(cam, prm);
    if (rc) return rc;
    // the whole frame is the window of all its pixels: one kernel for every pixel source (pt_aov.hip)
    return pt_render_aov_window(s, cam, prm, 0, 0, cam->W, cam->H, d_aov, d_prim, hip_stream);
}

int pt_aov(PtScene* s, const PtCamera* cam, const PtParams* prm, float* h_aov, int32_t* h_prim)
{
    if (!s || !h_aov) { pt_set_error("pt_aov: NULL argument"); return PT_ERR_INVALID; }
    int rc = pt_aov_args(cam, prm);
    if (rc) return rc;
    const size_t n = (size_t)cam->W * cam->H;
    HIPCHK(hipSetDevice(s->device));
    DevBuf d_aov, d_prim;      // d_prim stays null when the caller asked for no primitive ids
    HIPCHK(d_aov.alloc(n * 32));
    if (h_prim) HIPCHK(d_prim.alloc(n * 4));
    rc = pt_render_aov(s, cam, prm, d_aov.as<float>(), d_prim.as<int32_t>(), nullptr);
    if (rc) return rc;
    HIPCHK(hipMemcpy(h_aov, d_aov.as<>(), n * 32, hipMemcpyDeviceToHost));
    if (h_prim) HIPCHK(hipMemcpy(h_prim, d_prim.as<>(), n * 4, hipMemcpyDeviceToHost));
    return PT_OK;
}

int64_t pt_denoise_work_bytes(int32_t W, int32_t H)
{
    if (!frame_ok(W, H)) { pt_set_error("pt_denoise_work_bytes: frame %dx%d out of range", W, H); return -1; }
    return (int64_t)W * H * 48;
}

int64_t pt_denoise_batch_work_bytes(int32_t W, int32_t H, int32_t n_frames)
{
    if (!frame_ok(W, H) || n_frames < 1 || n_frames > 65535 || (int64_t)n_frames * W * H > kMaxPixels) {
        pt_set_error("pt_denoise_batch_work_bytes: %d frames of %dx%d out of range", n_frames, W, H); return -1;
    }
    return (int64_t)W * H * 48 * n_frames;
}

int pt_denoise_batch(const float* d_rgb, const float* d_aov, int32_t W, int32_t H, int32_t n_frames, int32_t sample_cnt, const PtDenoiseParams* p,
                     float* d_out, void* d_work, void* hip_stream)
{
    const int rc = denoise_args(d_rgb, d_aov, W, H, n_frames, sample_cnt, p, d_out, d_work, true);
    if (rc) return rc;
    const hipStream_t stream = (hipStream_t)hip_stream;
    // d_work: 3 x n_frames*W*H float4 (colour ping, colour pong, features), each frame-major like the inputs
    const size_t n = (size_t)W * H * (size_t)n_frames;
    if (p->iterations == 0) { HIPCHK(hipMemcpyAsync(d_out, d_rgb, n * 12, hipMemcpyDeviceToDevice, stream)); return PT_OK; }
    float4* c0 = (float4*)d_work;
    float4* c1 = c0 + n;
    float4* feat = c1 + n;
    const dim3 grid((unsigned)((W + 15) / 16), (unsigned)((H + 15) / 16), (unsigned)n_frames), block(256);
    const float sc = (float)sample_cnt;
    const int demodulate = p->demodulate ? 1 : 0;
    hipLaunchKernelGGL(ptd::dn_pack, grid, block, 0, stream, d_rgb, (const float4*)d_aov, W, H, sc, demodulate, c0, feat);
    const float kn = 1.f / (p->sigma_normal * p->sigma_normal), kz = 1.f / p->sigma_depth;
    float kc = 1.f / (p->sigma_color * p->sigma_color);
    for (int it = 0; it < p->iterations; it++) {
        hipLaunchKernelGGL(ptd::dn_atrous, grid, block, 0, stream, (const float4*)c0, (const float4*)feat, W, H, 1 << it, kc, kn, kz, c1);
        float4* t = c0; c0 = c1; c1 = t;
        kc *= 4.f;
    }
    hipLaunchKernelGGL(ptd::dn_finish, grid, block, 0, stream, (const float4*)c0, (const float4*)d_aov, W, H, sc, demodulate, d_out);
    HIPCHK(hipGetLastError());
    return PT_OK;
}

// one frame is the batch of one: one code path
int pt_denoise(const float* d_rgb, const float* d_aov, int32_t W, int32_t H, int32_t sample_cnt, const PtDenoiseParams* p,
               float* d_out, void* d_work, void* hip_stream)
{
    return pt_denoise_batch(d_rgb, d_aov, W, H, 1, sample_cnt, p, d_out, d_work, hip_stream);
}

int pt_denoise_batch_host(int32_t device, const float* h_rgb, const float* h_aov, int32_t W, int32_t H, int32_t n_frames, int32_t sample_cnt,
                          const PtDenoiseParams* p, float* h_out)
{
    int rc = denoise_args(h_rgb, h_aov, W, H, n_frames, sample_cnt, p, h_out, nullptr, false);
    if (rc) return rc;
    const size_t n = (size_t)W * H * (size_t)n_frames;
    HIPCHK(hipSetDevice(device));
    DevBuf buf;      // one allocation: rgb | aov | out | work
    HIPCHK(buf.alloc(n * (12 + 32 + 12 + 48) + 64));
    char* d = buf.as<char>();
    float* d_rgb = (float*)d;
    float* d_aov = (float*)(d + ((n * 12 + 15) & ~(size_t)15));
    float* d_out = (float*)((char*)d_aov + n * 32);
    void* d_work = (char*)d_aov + ((n * 44 + 15) & ~(size_t)15);
    HIPCHK(hipMemcpy(d_rgb, h_rgb, n * 12, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d_aov, h_aov, n * 32, hipMemcpyHostToDevice));
    rc = pt_denoise_batch(d_rgb, d_aov, W, H, n_frames, sample_cnt, p, d_out, d_work, nullptr);
    if (rc) return rc;
    HIPCHK(hipMemcpy(h_out, d_out, n * 12, hipMemcpyDeviceToHost));
    return PT_OK;
}

int pt_denoise_host(int32_t device, const float* h_rgb, const float* h_aov, int32_t W, int32_t H, int32_t sample_cnt,
                    const PtDenoiseParams* p, float* h_out)
{
    return pt_denoise_batch_host(device, h_rgb, h_aov, W, H, 1, sample_cnt, p, h_out);
}

// ---- the exact windowed denoise (host only): how far a pixel of the L-iteration filter looks, and a window grown by that much ----
int32_t pt_denoise_margin(int32_t iterations)
{
    if (iterations < 0 || iterations > 12) { pt_set_error("pt_denoise_margin: iterations %d outside 0..12", iterations); return -1; }
    return 2 * ((1 << iterations) - 1);      // the sum of the reaches 2 * 2^i of iterations 0 .. L-1
}

int pt_window_expand(const PtCamera* cam, const int32_t window[4], int32_t margin, int32_t expanded[4])
{
    if (!window || !expanded) { pt_set_error("pt_window_expand: NULL argument"); return PT_ERR_INVALID; }
    const int rc = pt_window_args("pt_window_expand", cam, window[0], window[1], window[2], window[3]);
    if (rc) return rc;
    if (margin < -1) { pt_set_error("pt_window_expand: margin %d (-1: the margin of the default iterations, else >= 0)", margin); return PT_ERR_INVALID; }
    if (margin == -1) { PtDenoiseParams p; pt_denoise_params_default(&p); margin = pt_denoise_margin(p.iterations); }
    const int64_t m = margin, x0 = window[0] - m, y0 = window[1] - m, x1 = window[2] + m, y1 = window[3] + m;
    expanded[0] = (int32_t)(x0 < 0 ? 0 : x0); expanded[1] = (int32_t)(y0 < 0 ? 0 : y0);
    expanded[2] = (int32_t)(x1 > cam->W ? cam->W : x1); expanded[3] = (int32_t)(y1 > cam->H ? cam->H : y1);
    return PT_OK;
}

}  // extern "C"
