// pt_denoise.hip — first-hit feature buffers ("AOVs") and the edge-aware denoiser guided by them (include/pt_api.h:
// pt_render_aov, pt_denoise).  New ground: the reference has neither.  Nothing here touches a render's state.
//
// AOVs (aov_kernel): per pixel of the full frame, the camera ray of the FIRST path of each pass first_pass + j of the call
// (the render's seed expression, two jitter draws, pixel_direction, origin cam.pos, t_max 999999 — as dbg_pixel_dir), traced to
// its closest hit with trace_closest + make_surf (as dbg_raycast).  Float32 sums in pass order, one IEEE division at the end:
//   [0..2] sum albedo / passes   [3..5] sum shading normal (ray-facing, not renormalised) / passes
//   [6] sum t / hits (0 if none) [7] hits / passes
// The host restates it bit for bit from the oracle (tests/denoise_ref.py: aov_from_oracle).  One thread per pixel, one wave per
// 8x8 tile (ray coherence), the LDS traversal stack of dbg_raycast.
//
// Denoiser: edge-avoiding a-trous wavelet filter (Dammertz et al. 2010) with albedo demodulation.  Definition (tests/denoise_ref.py
// states it in numpy, float64):
//   c_p = rgb_p / sample_cnt;  div_p = albedo_p where > 1e-3 else 1 (per channel; 1 without demodulation);  e_p = c_p / div_p
//   finite_p = all three components of c_p are finite (after an iteration: of e'_p)
//   iteration i = 0 .. L-1, step s = 2^i, taps q = p + s (dx, dy), dx, dy in -2..2 (dy outer, dx inner), inside the frame and finite_q:
//     w = h(dx) h(dy) exp(-E),  h = (1/16, 1/4, 3/8, 1/4, 1/16)
//     E = |e_p - e_q|^2 / (sc^2 4^-i)  (left out when !finite_p)  + |n_p - n_q|^2 / sn^2
//       + |z_p - z_q| / (sz max(z_p, z_q))  (0 when both depths are 0);   w = 0 exactly when E > 80
//   e'_p = sum w e_q / sum w, or e_p when sum w = 0 (a NaN pixel with a finite neighbour becomes finite; a NaN is never spread);
//   n (AOV 3..5) and z (AOV 6) are not filtered;  out_p = e_p^(L) div_p sample_cnt;  L = 0 is a plain copy.
// Kernels: pack (demodulate once: colour float4 (e.rgb, finite), feature float4 (n.xyz, z)), L x atrous (ping-pong of the colour
// float4s in the work buffer), finish (remodulate, write RGB).  256-thread blocks, each wave an 8x8 pixel tile, plain 16-byte loads:
// the 48 B/pixel working set (100 MB at 1080p) stays in the Infinity Cache, the 5x5 footprint of a wave in L2.
#include <hip/hip_runtime.h>
#include "pt_device.h"
#include "pt_math.h"
#include "pt_bxdf.h"
#include "pt_trace.h"
#include "pt_shade.h"
#include "pt_internal.h"

namespace ptd {

__global__ __launch_bounds__(kBlockThreads)
void aov_kernel(DevScene sc, DevCamera cam, int first_pass, int passes, int tiles_x, int n_tiles,
                float4* __restrict__ aov, int* __restrict__ prim_out)
{
    __shared__ int lds_stack[kWavesPerBlock][kStackDepth * 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int* stack = &lds_stack[wave][lane];
    const int tile = blockIdx.x * kWavesPerBlock + wave;
    const int px = (tile % tiles_x) * kTile + (lane & 7), py = (tile / tiles_x) * kTile + (lane >> 3);
    if (tile >= n_tiles || px >= cam.W || py >= cam.H) return;
    const f3 org(cam.pos[0], cam.pos[1], cam.pos[2]);
    f3 alb(0.f, 0.f, 0.f), nrm(0.f, 0.f, 0.f);
    float tsum = 0.f;
    int hits = 0, prim0 = -1;
    for (int j = 0; j < passes; j++) {
        const int pass = first_pass + j;
        Rng rng;
        rng.init((uint64_t)(int64_t)(py * cam.W + px + pass * cam.W * cam.H));      // srcs/pathtracer.cu:70-71
        float u1, u2;
        const f3 dir = pixel_direction(cam, px, py, rng, u1, u2);
        float t; TraceStats st{0, 0, 0};
        const int prim = trace_closest<false>(sc, org, dir, 999999.f, stack, t, st);
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
    const size_t i = (size_t)py * cam.W + px;
    aov[2 * i] = make_float4(alb.x / fp, alb.y / fp, alb.z / fp, nrm.x / fp);
    aov[2 * i + 1] = make_float4(nrm.y / fp, nrm.z / fp, hits ? tsum / (float)hits : 0.f, (float)hits / fp);
    if (prim_out) prim_out[i] = prim0;
}

// pixel of this thread: blocks of 16x16 pixels, wave w of the block on the 8x8 quadrant (w & 1, w >> 1)
PT_DEV void dn_pixel(int& px, int& py)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    px = blockIdx.x * 16 + (wave & 1) * kTile + (lane & 7);
    py = blockIdx.y * 16 + (wave >> 1) * kTile + (lane >> 3);
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
    int px, py; dn_pixel(px, py);
    if (px >= W || py >= H) return;
    const size_t i = (size_t)py * W + px;
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
    int px, py; dn_pixel(px, py);
    if (px >= W || py >= H) return;
    const float h[5] = {1.f / 16.f, 1.f / 4.f, 3.f / 8.f, 1.f / 4.f, 1.f / 16.f};
    const size_t i = (size_t)py * W + px;
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
            const size_t q = (size_t)qy * W + qx;
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
    int px, py; dn_pixel(px, py);
    if (px >= W || py >= H) return;
    const size_t i = (size_t)py * W + px;
    const float4 e = color[i];
    const f3 d = demod_div(aov[2 * i], demodulate);
    out[3 * i] = (e.x * d.x) * sample_cnt;
    out[3 * i + 1] = (e.y * d.y) * sample_cnt;
    out[3 * i + 2] = (e.z * d.z) * sample_cnt;
}

}  // namespace ptd

// ---------------------------------------------------------------------------------------
// Launchers (called from pt_api.hip)
// ---------------------------------------------------------------------------------------
extern "C" {

hipError_t ptk_aov(const ptd::DevScene* sc, const ptd::DevCamera* cam, int first_pass, int passes, float* aov, int* prim, hipStream_t stream)
{
    const int tiles_x = (cam->W + ptd::kTile - 1) / ptd::kTile, tiles_y = (cam->H + ptd::kTile - 1) / ptd::kTile;
    const int n_tiles = tiles_x * tiles_y;
    const int nb = (n_tiles + ptd::kWavesPerBlock - 1) / ptd::kWavesPerBlock;
    if (nb > 0) hipLaunchKernelGGL(ptd::aov_kernel, dim3(nb), dim3(ptd::kBlockThreads), 0, stream, *sc, *cam, first_pass, passes, tiles_x, n_tiles,
                                   (float4*)aov, prim);
    return hipGetLastError();
}

// work: 3 x W*H float4 (colour ping, colour pong, features); iterations >= 1
hipError_t ptk_denoise(const float* rgb, const float* aov, int W, int H, int sample_cnt, int iterations, float sigma_color,
                       float sigma_normal, float sigma_depth, int demodulate, float* out, void* work, hipStream_t stream)
{
    const size_t n = (size_t)W * H;
    float4* c0 = (float4*)work;
    float4* c1 = c0 + n;
    float4* feat = c1 + n;
    const dim3 grid((unsigned)((W + 15) / 16), (unsigned)((H + 15) / 16)), block(256);
    const float sc = (float)sample_cnt;
    hipLaunchKernelGGL(ptd::dn_pack, grid, block, 0, stream, rgb, (const float4*)aov, W, H, sc, demodulate, c0, feat);
    const float kn = 1.f / (sigma_normal * sigma_normal), kz = 1.f / sigma_depth;
    float kc = 1.f / (sigma_color * sigma_color);
    for (int it = 0; it < iterations; it++) {
        hipLaunchKernelGGL(ptd::dn_atrous, grid, block, 0, stream, (const float4*)c0, (const float4*)feat, W, H, 1 << it, kc, kn, kz, c1);
        float4* t = c0; c0 = c1; c1 = t;
        kc *= 4.f;
    }
    hipLaunchKernelGGL(ptd::dn_finish, grid, block, 0, stream, (const float4*)c0, (const float4*)aov, W, H, sc, demodulate, out);
    return hipGetLastError();
}

}  // extern "C"
