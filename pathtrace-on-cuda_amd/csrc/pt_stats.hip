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
#include "pt_device.h"
#include "pt_internal.h"

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

// ---------------------------------------------------------------------------------------
// Launchers (called from pt_api.hip)
// ---------------------------------------------------------------------------------------
extern "C" {

// staging: passes x n floats (pass-major); sum, m2: n floats each
hipError_t ptk_stats_fold(const float* staging, int passes, long long n, int n_before, float* sum, float* m2, hipStream_t stream)
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

hipError_t ptk_stats_variance(const float* m2, long long n, int n_passes, float* var, hipStream_t stream)
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

// blocks of st_estimate for n floats (n a multiple of 192): one partial of ptk_stats_partial_bytes() bytes each
int ptk_stats_blocks(long long n)
{
    const long long nb = (n / 12 + 255) / 256;
    return nb < 1 ? 1 : nb > ptd::kStBlocks ? ptd::kStBlocks : (int)nb;
}
int ptk_stats_partial_bytes(void) { return (int)sizeof(ptd::StPartial); }

hipError_t ptk_stats_estimate(const float* sum, const float* m2, long long n, int n_passes, int W, int H, int tiles_x, int n_tiles_total,
                              int rank, int world, void* partial, hipStream_t stream)
{
    const float nf = (float)n_passes, nf1 = (float)(n_passes - 1);
    const int nb = ptk_stats_blocks(n);
    if (ptd::st_aligned16(sum, m2, nullptr))
        hipLaunchKernelGGL(ptd::st_estimate<true>, dim3(nb), dim3(256), 0, stream, sum, m2, n / 12, nf, nf1, W, H, tiles_x, n_tiles_total,
                           rank, world, (ptd::StPartial*)partial);
    else
        hipLaunchKernelGGL(ptd::st_estimate<false>, dim3(nb), dim3(256), 0, stream, sum, m2, n / 12, nf, nf1, W, H, tiles_x, n_tiles_total,
                           rank, world, (ptd::StPartial*)partial);
    return hipGetLastError();
}

}  // extern "C"
