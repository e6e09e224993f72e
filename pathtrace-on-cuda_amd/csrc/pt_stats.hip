// pt_stats.hip — per-pixel moments over passes and the error estimate reduced from them (include/pt_api.h:
// pt_accumulate_passes, pt_variance, pt_error_estimate).  New ground: the reference has neither.  Nothing here touches a
// render's state: the kernels only READ the per-pass means a render left at the start of its work buffer.
//
// Why passes are the unit: the reference draws ONE jittered direction per pixel per pass and sends all spp_per_pass paths
// down it (srcs/pathtracer.cu:74-80), so the samples inside a pass share their anti-aliasing term; the per-pass means are the
// independent draws, and there are exactly `passes` of them per float in the staging slab (pass-major, then the layout of
// d_tiles) that sum_passes adds up.
//
// Fold (st_fold), per float, pass k = n_before + 1, ... with mean m, every operation IEEE float32 in this order:
//   S_prev = S;  S = S_prev + m                                                   (k = 1: S = 0 + m)
//   k >= 2:  d1 = m - S_prev / (k - 1);  d2 = m - S / k;  M2 = M2 + d1 * d2       (k = 1: M2 = 0)
// Welford's update with the means taken from S: S is bit for bit what sum_passes returns for the same passes, however they
// were split over calls, and M2 (the sum of squared deviations of the means from THEIR mean) never goes through the
// cancelling Q - S^2 / n.  tests/stats_ref.py restates it in numpy float32.
// Variance of S (st_variance):  Var = max(M2, 0) * n / (n - 1)   (M2 / (n (n - 1)) is the variance of the mean of the passes,
// S = n x that mean); a NaN M2 stays NaN.
// Estimate (st_estimate): per pixel, float32 terms as written, summed in float64 —
//   sum Var_c, sum S_c * S_c over the three channels;  sqrt((Var_r + Var_g) + Var_b) / (((|S_r| + |S_g|) + |S_b|) + 0.03 n)
// over the in-frame pixels whose S and M2 are all finite.  Deterministic: a fixed grid, each thread a fixed stride of pixels,
// each block a fixed shuffle + LDS tree, one partial per block; the host adds the partials in block order.  No atomics.
// Kernels: pure streams, 256-thread blocks, one float4 per thread where the buffers are 16-byte aligned (a render's tile
// buffers always are: pt_tiles_floats() is a multiple of 192), plain 16-byte loads and stores.
#include <hip/hip_runtime.h>
#include <cmath>
#include <vector>
#include "pt_device.h"
#include "pt_scene.h"

namespace ptd {

struct StPartial { double var, s2, se; long long pixels, skipped; };      // 40 bytes: one per block of st_estimate
constexpr int kStBlocks = 1024;      // grid cap of st_estimate (4 blocks per CU)

#define PT_ST_DEV __device__ __forceinline__

// one pass mean m folded into (S, M2); k = passes folded in once this one is (1-based)
PT_ST_DEV void st_fold1(float m, int k, float& S, float& M2)
{
    const float Sp = S;
    S = Sp + m;
    if (k >= 2) {
        const float d1 = m - Sp / (float)(k - 1);
        const float d2 = m - S / (float)k;
        M2 = M2 + d1 * d2;
    }
}
PT_ST_DEV void st_fold1(const float4 m, int k, float4& S, float4& M2)
{
    st_fold1(m.x, k, S.x, M2.x); st_fold1(m.y, k, S.y, M2.y); st_fold1(m.z, k, S.z, M2.z); st_fold1(m.w, k, S.w, M2.w);
}
PT_ST_DEV void st_zero(float& v) { v = 0.f; }
PT_ST_DEV void st_zero(float4& v) { v = make_float4(0.f, 0.f, 0.f, 0.f); }

// Var = max(M2, 0) * n / (n - 1); written so that a NaN M2 stays NaN (fmaxf would drop it)
PT_ST_DEV float st_var(float m2, float nf, float nf1) { return ((m2 < 0.f ? 0.f : m2) * nf) / nf1; }

// V = float4 (n = floats / 4) or float
template <class V>
__global__ __launch_bounds__(256)
void st_fold(const V* __restrict__ staging, int passes, long long n, int n_before, V* __restrict__ sum, V* __restrict__ m2)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    V S, M;
    if (n_before == 0) { st_zero(S); st_zero(M); }
    else { S = sum[i]; M = m2[i]; }
    for (int p = 0; p < passes; p++) st_fold1(staging[(long long)p * n + i], n_before + p + 1, S, M);
    sum[i] = S;
    m2[i] = M;
}

__global__ __launch_bounds__(256)
void st_variance4(const float4* __restrict__ m2, long long n, float nf, float nf1, float4* __restrict__ var)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float4 m = m2[i];
    var[i] = make_float4(st_var(m.x, nf, nf1), st_var(m.y, nf, nf1), st_var(m.z, nf, nf1), st_var(m.w, nf, nf1));
}
__global__ __launch_bounds__(256)
void st_variance1(const float* __restrict__ m2, long long n, float nf, float nf1, float* __restrict__ var)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    var[i] = st_var(m2[i], nf, nf1);
}

// Each thread takes groups of 4 pixels (12 floats = 3 float4 of each buffer when VEC), group g = thread + j * (threads of the grid).
// A pixel of the tile layout is in the frame when its tile exists and its (px, py) lies inside W x H (padding pixels are 0 in
// both buffers after a render; they are left out of the COUNT here and would add 0 to every sum).
template <bool VEC>
__global__ __launch_bounds__(256)
void st_estimate(const float* __restrict__ sum, const float* __restrict__ m2, long long n_groups, float nf, float nf1,
                 int W, int H, int tiles_x, int n_tiles_total, int rank, int world, StPartial* __restrict__ partial)
{
    double aVar = 0.0, aS2 = 0.0, aSe = 0.0;
    long long nPix = 0, nSkip = 0;
    const float bias = 0.03f * nf;
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x; g < n_groups; g += stride) {
        float s[12], m[12];
        if (VEC) {
            const float4* s4 = (const float4*)sum + 3 * g;
            const float4* m4 = (const float4*)m2 + 3 * g;
#pragma unroll
            for (int j = 0; j < 3; j++) {
                const float4 a = s4[j], b = m4[j];
                s[4 * j] = a.x; s[4 * j + 1] = a.y; s[4 * j + 2] = a.z; s[4 * j + 3] = a.w;
                m[4 * j] = b.x; m[4 * j + 1] = b.y; m[4 * j + 2] = b.z; m[4 * j + 3] = b.w;
            }
        } else {
#pragma unroll
            for (int j = 0; j < 12; j++) { s[j] = sum[12 * g + j]; m[j] = m2[12 * g + j]; }
        }
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const long long q = 4 * g + j;                         // pixel of the tile layout
            const long long tile = (q >> 6) * world + rank;
            const int lane = (int)(q & 63);
            if (tile >= n_tiles_total) continue;
            const int px = (int)(tile % tiles_x) * kTile + (lane & 7), py = (int)(tile / tiles_x) * kTile + (lane >> 3);
            if (px >= W || py >= H) continue;
            const float sr = s[3 * j], sg = s[3 * j + 1], sb = s[3 * j + 2];
            const float mr = m[3 * j], mg = m[3 * j + 1], mb = m[3 * j + 2];
            if (!(__builtin_isfinite(sr) && __builtin_isfinite(sg) && __builtin_isfinite(sb) &&
                  __builtin_isfinite(mr) && __builtin_isfinite(mg) && __builtin_isfinite(mb))) { nSkip++; continue; }
            const float vr = st_var(mr, nf, nf1), vg = st_var(mg, nf, nf1), vb = st_var(mb, nf, nf1);
            aVar += (double)vr; aVar += (double)vg; aVar += (double)vb;
            aS2 += (double)(sr * sr); aS2 += (double)(sg * sg); aS2 += (double)(sb * sb);
            const float den = ((__builtin_fabsf(sr) + __builtin_fabsf(sg)) + __builtin_fabsf(sb)) + bias;
            aSe += (double)(__builtin_sqrtf((vr + vg) + vb) / den);
            nPix++;
        }
    }
    // fixed tree: lanes of a wave by shuffle, then the 4 waves in order
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        aVar += __shfl_down(aVar, o); aS2 += __shfl_down(aS2, o); aSe += __shfl_down(aSe, o);
        nPix += __shfl_down(nPix, o); nSkip += __shfl_down(nSkip, o);
    }
    __shared__ StPartial w[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) w[wave] = StPartial{aVar, aS2, aSe, nPix, nSkip};
    __syncthreads();
    if (threadIdx.x == 0) {
        StPartial r = w[0];
        for (int k = 1; k < 4; k++) { r.var += w[k].var; r.s2 += w[k].s2; r.se += w[k].se; r.pixels += w[k].pixels; r.skipped += w[k].skipped; }
        partial[blockIdx.x] = r;
    }
}

static inline bool st_aligned16(const void* a, const void* b, const void* c)
{
    return (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c) & 15) == 0;
}
}  // namespace ptd

// ---- launchers ----------------------------------------------------------------------------------------------------------------------
// staging: passes x n floats (pass-major); sum, m2: n floats each
static hipError_t launch_fold(const float* staging, int passes, long long n, int n_before, float* sum, float* m2, hipStream_t stream)
{
    if (n <= 0) return hipSuccess;
    if (n % 4 == 0 && ptd::st_aligned16(staging, sum, m2)) {
        const long long n4 = n / 4, nb = (n4 + 255) / 256;
        hipLaunchKernelGGL(ptd::st_fold<float4>, dim3((unsigned)nb), dim3(256), 0, stream, (const float4*)staging, passes, n4, n_before,
                           (float4*)sum, (float4*)m2);
    } else {
        const long long nb = (n + 255) / 256;
        hipLaunchKernelGGL(ptd::st_fold<float>, dim3((unsigned)nb), dim3(256), 0, stream, staging, passes, n, n_before, sum, m2);
    }
    return hipGetLastError();
}

static hipError_t launch_variance(const float* m2, long long n, int n_passes, float* var, hipStream_t stream)
{
    if (n <= 0) return hipSuccess;
    const float nf = (float)n_passes, nf1 = (float)(n_passes - 1);
    if (n % 4 == 0 && ptd::st_aligned16(m2, var, nullptr)) {
        const long long n4 = n / 4, nb = (n4 + 255) / 256;
        hipLaunchKernelGGL(ptd::st_variance4, dim3((unsigned)nb), dim3(256), 0, stream, (const float4*)m2, n4, nf, nf1, (float4*)var);
    } else {
        const long long nb = (n + 255) / 256;
        hipLaunchKernelGGL(ptd::st_variance1, dim3((unsigned)nb), dim3(256), 0, stream, m2, n, nf, nf1, var);
    }
    return hipGetLastError();
}

// blocks of st_estimate for n floats (n a multiple of 192): one StPartial each
static int estimate_blocks(long long n)
{
    const long long nb = (n / 12 + 255) / 256;
    return nb < 1 ? 1 : nb > ptd::kStBlocks ? ptd::kStBlocks : (int)nb;
}

static hipError_t launch_estimate(const float* sum, const float* m2, long long n, int n_passes, int W, int H, int tiles_x, int n_tiles_total,
                                  int rank, int world, void* partial, hipStream_t stream)
{
    const float nf = (float)n_passes, nf1 = (float)(n_passes - 1);
    const int nb = estimate_blocks(n);
    if (ptd::st_aligned16(sum, m2, nullptr))
        hipLaunchKernelGGL(ptd::st_estimate<true>, dim3(nb), dim3(256), 0, stream, sum, m2, n / 12, nf, nf1, W, H, tiles_x, n_tiles_total,
                           rank, world, (ptd::StPartial*)partial);
    else
        hipLaunchKernelGGL(ptd::st_estimate<false>, dim3(nb), dim3(256), 0, stream, sum, m2, n / 12, nf, nf1, W, H, tiles_x, n_tiles_total,
                           rank, world, (ptd::StPartial*)partial);
    return hipGetLastError();
}


// ---- entry points (include/pt_api.h): every argument check comes before the first HIP call ----------------------------------------
extern "C" {

int pt_accumulate_passes(const void* d_work, const PtCamera* cam, const PtParams* prm, int32_t n_before, float* d_sum, float* d_m2,
                         void* hip_stream)
{
    if (!d_work || !d_sum || !d_m2) { pt_set_error("pt_accumulate_passes: NULL argument"); return PT_ERR_INVALID; }
    if (n_before < 0 || (prm && (long long)n_before + prm->passes > 0x7fffffffLL)) { pt_set_error("pt_accumulate_passes: bad n_before %d", n_before); return PT_ERR_INVALID; }
    ptd::DevParams d;
    const int rc = pt_fill_params(cam, prm, d);
    if (rc) return rc;
    const long long perPass = (long long)d.n_tiles_local * ptd::kTilePixels * 3;
    // both render modes leave the per-pass means at the start of the work buffer (pt_render_tiles: what sum_passes reads)
    HIPCHK(launch_fold(ptk_wf_staging(const_cast<void*>(d_work)), d.passes, perPass, n_before, d_sum, d_m2, (hipStream_t)hip_stream));
    return PT_OK;
}

int pt_variance(const float* d_m2, int64_t n_floats, int32_t n_passes, float* d_var, void* hip_stream)
{
    if (!d_m2 || !d_var || n_floats < 1 || n_passes < 2) { pt_set_error("pt_variance: NULL buffer, n_floats < 1 or n_passes < 2"); return PT_ERR_INVALID; }
    HIPCHK(launch_variance(d_m2, n_floats, n_passes, d_var, (hipStream_t)hip_stream));
    return PT_OK;
}

int64_t pt_error_scratch_bytes(int64_t n_floats)
{
    if (n_floats < 1) { pt_set_error("pt_error_scratch_bytes: n_floats < 1"); return -1; }
    const int64_t nb = (n_floats + 3071) / 3072;
    return (nb > 1024 ? 1024 : nb) * (int64_t)sizeof(ptd::StPartial);
}

int pt_error_estimate(const float* d_sum, const float* d_m2, const PtCamera* cam, const PtParams* prm, int32_t n_passes,
                      void* d_scratch, PtErrorEstimate* h_out, void* hip_stream)
{
    if (!d_sum || !d_m2 || !d_scratch || !h_out) { pt_set_error("pt_error_estimate: NULL argument"); return PT_ERR_INVALID; }
    if (n_passes < 2) { pt_set_error("pt_error_estimate: n_passes %d < 2", n_passes); return PT_ERR_INVALID; }
    if (!cam || !prm) { pt_set_error("NULL camera/params"); return PT_ERR_INVALID; }
    PtParams p = *prm; p.passes = 1; p.first_pass = 0;      // only the geometry of the split is read
    ptd::DevParams d;
    const int rc = pt_fill_params(cam, &p, d);
    if (rc) return rc;
    const long long n = (long long)d.n_tiles_local * ptd::kTilePixels * 3;
    const hipStream_t stream = (hipStream_t)hip_stream;
    HIPCHK(launch_estimate(d_sum, d_m2, n, n_passes, cam->W, cam->H, d.tiles_x, d.n_tiles_total, d.rank, d.world, d_scratch, stream));
    std::vector<ptd::StPartial> part((size_t)estimate_blocks(n));
    HIPCHK(hipMemcpyAsync(part.data(), d_scratch, part.size() * sizeof(ptd::StPartial), hipMemcpyDeviceToHost, stream));
    HIPCHK(hipStreamSynchronize(stream));
    double var = 0.0, s2 = 0.0, se = 0.0; long long pixels = 0, skipped = 0;
    for (const ptd::StPartial& q : part) { var += q.var; s2 += q.s2; se += q.se; pixels += q.pixels; skipped += q.skipped; }      // block order
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
    const size_t frameBytes = (size_t)cam->W * cam->H * 12;
    DevBuf b_tiles, b_sum, b_m2, b_work, b_scratch, b_frame;
    HIPCHK(b_tiles.alloc((size_t)nt * 4));
    HIPCHK(b_sum.alloc((size_t)nt * 4));
    HIPCHK(b_m2.alloc((size_t)nt * 4));
    HIPCHK(b_work.alloc((size_t)wb));
    HIPCHK(b_scratch.alloc((size_t)pt_error_scratch_bytes(nt)));
    HIPCHK(b_frame.alloc(frameBytes));
    float *d_tiles = b_tiles.as<float>(), *d_sum = b_sum.as<float>(), *d_m2 = b_m2.as<float>(), *d_frame = b_frame.as<float>();
    void *d_work = b_work.as<>(), *d_scratch = b_scratch.as<>();
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
}

}  // extern "C"
