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
// buffers always are: pt_tiles_floats() is a multiple of 192), plain 16-byte loads and stores; the scalar twins (st_fold<float>,
// st_variance1, st_estimate<false>) give the same bits for buffers that are only 4-byte aligned.  tests/stats_ref.py: estimate32
// restates st_estimate and the host sum in their order; tests/test_stats_exact.py holds every kernel here to its restatement.
//
// Adaptive sampling (pt_accumulate_tile_list, pt_tile_errors, pt_finish_tiles, pt_render_adaptive) builds on the same fold and variance:
// st_fold_list folds the staging slab of a tile-LIST render into frame-layout moments (entry i -> tile list[i]), st_tile_errors reduces the
// mean_rel_se term over the 64 pixels of each listed tile (one wave per tile, a fixed shuffle tree, no atomics), st_finish_tiles divides
// by each tile's own pass count.  pt_render_adaptive is the host loop that shrinks the list.  tests/adaptive_ref.py restates them.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstring>
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
// what the entry points require of their buffers: 4 bytes for float / int32, 8 for the records that hold a double, 16 where a kernel
// has no scalar twin (the list calls).  NULL passes: whether a pointer may be NULL is its own check.
static inline bool st_aligned(unsigned bytes, const void* a, const void* b = nullptr, const void* c = nullptr, const void* d = nullptr)
{
    return (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c | (uintptr_t)d) & (bytes - 1)) == 0;
}

// ---- adaptive sampling: the moments of a tile LIST, an error figure per tile, the frame of tiles with unequal pass counts ----------
// "Frame tile layout" = the layout of pt_render_tiles with rank 0 of world 1: tile t owns floats 192 t .. 192 t + 191 (48 float4).
constexpr int kTileVec = kTilePixels * 3 / 4;      // float4 per tile

// st_fold of a list render's staging slab (passes x n_tiles x 192 floats, pass-major, list order) into frame-layout S / M2: list entry
// e goes to tile list[e].  One thread per float4 of the list; tiles not listed are not touched.  An entry outside the frame is skipped
// (it would be a write out of bounds); a tile listed twice is the caller's race.
__global__ __launch_bounds__(256)
void st_fold_list(const float4* __restrict__ staging, int passes, long long n4, const int32_t* __restrict__ list, int n_tiles_total,
                  int n_before, float4* __restrict__ sum, float4* __restrict__ m2, int32_t* __restrict__ tile_passes)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n4) return;
    const int e = (int)(i / kTileVec), j = (int)(i - (long long)e * kTileVec);
    const int tile = list[e];
    if ((unsigned)tile >= (unsigned)n_tiles_total) return;
    const long long o = (long long)tile * kTileVec + j;
    float4 S, M;
    if (n_before == 0) { st_zero(S); st_zero(M); }
    else { S = sum[o]; M = m2[o]; }
    for (int p = 0; p < passes; p++) st_fold1(staging[(long long)p * n4 + i], n_before + p + 1, S, M);
    sum[o] = S;
    m2[o] = M;
    if (tile_passes && j == 0) tile_passes[tile] = n_before + passes;
}

struct StTileError { double mean_rel_se; int32_t pixels, skipped; };      // PtTileError
static_assert(sizeof(StTileError) == 16 && sizeof(PtTileError) == 16, "PtTileError is 16 bytes");

// One wave per list entry, lane = pixel of the tile (4 entries per block; no LDS, no barrier, no atomics).  The term of a pixel is
// st_estimate's mean_rel_se term; a lane that is not used adds 0.0.  Fixed order: o = 32 .. 1, lane l < o adds lane l + o (what lanes
// >= o hold after a step is never read again).  list == nullptr: entry e is tile e.
__global__ __launch_bounds__(256)
void st_tile_errors(const float* __restrict__ sum, const float* __restrict__ m2, const int32_t* __restrict__ list, int n_tiles,
                    float nf, float nf1, int W, int H, int tiles_x, int n_tiles_total, StTileError* __restrict__ err)
{
    const int lane = threadIdx.x & 63;
    const int e = blockIdx.x * 4 + (threadIdx.x >> 6);      // uniform over the wave
    if (e >= n_tiles) return;
    const int tile = list ? list[e] : e;
    if ((unsigned)tile >= (unsigned)n_tiles_total) {         // no such tile: nothing is read
        if (lane == 0) err[e] = StTileError{0.0, 0, 0};
        return;
    }
    const int px = (tile % tiles_x) * kTile + (lane & 7), py = (tile / tiles_x) * kTile + (lane >> 3);
    const bool inFrame = px < W && py < H;
    const long long at = ((long long)tile * kTilePixels + lane) * 3;
    const float sr = sum[at], sg = sum[at + 1], sb = sum[at + 2];
    const float mr = m2[at], mg = m2[at + 1], mb = m2[at + 2];
    const bool used = inFrame && __builtin_isfinite(sr) && __builtin_isfinite(sg) && __builtin_isfinite(sb) &&
                      __builtin_isfinite(mr) && __builtin_isfinite(mg) && __builtin_isfinite(mb);
    double a = 0.0;
    if (used) {
        const float vr = st_var(mr, nf, nf1), vg = st_var(mg, nf, nf1), vb = st_var(mb, nf, nf1);
        const float den = ((__builtin_fabsf(sr) + __builtin_fabsf(sg)) + __builtin_fabsf(sb)) + 0.03f * nf;
        a = (double)(__builtin_sqrtf((vr + vg) + vb) / den);
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) a += __shfl_down(a, o);
    const int pixels = __popcll(__ballot(used)), skipped = __popcll(__ballot(inFrame && !used));
    if (lane == 0) err[e] = StTileError{pixels ? a / (double)pixels : 0.0, pixels, skipped};
}

// mean = S / n and Var = max(M2, 0) * n / (n - 1) with n the tile's own pass count; n == 0: +0 in both.  One thread per float4 of the
// frame tile layout; either output may be nullptr.
__global__ __launch_bounds__(256)
void st_finish_tiles(const float4* __restrict__ sum, const float4* __restrict__ m2, const int32_t* __restrict__ tile_passes, long long n4,
                     float4* __restrict__ mean, float4* __restrict__ var)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n4) return;
    const int n = tile_passes[i / kTileVec];
    float4 a, v;
    st_zero(a); st_zero(v);
    if (n != 0) {
        const float nf = (float)n, nf1 = (float)(n - 1);
        if (mean) { const float4 s = sum[i]; a = make_float4(s.x / nf, s.y / nf, s.z / nf, s.w / nf); }
        if (var) { const float4 m = m2[i]; v = make_float4(st_var(m.x, nf, nf1), st_var(m.y, nf, nf1), st_var(m.z, nf, nf1), st_var(m.w, nf, nf1)); }
    }
    if (mean) mean[i] = a;
    if (var) var[i] = v;
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
    if (!ptd::st_aligned(4, d_work, d_sum, d_m2)) { pt_set_error("pt_accumulate_passes: a float buffer is not 4-byte aligned"); return PT_ERR_INVALID; }
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
    if (!ptd::st_aligned(4, d_m2, d_var)) { pt_set_error("pt_variance: a float buffer is not 4-byte aligned"); return PT_ERR_INVALID; }
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
    if (!ptd::st_aligned(4, d_sum, d_m2) || !ptd::st_aligned(8, d_scratch)) { pt_set_error("pt_error_estimate: d_sum / d_m2 not 4-byte or d_scratch not 8-byte aligned"); return PT_ERR_INVALID; }
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

// ---- adaptive sampling ---------------------------------------------------------------------------------------------------------------
// the tile grid of a whole frame (rank 0 of world 1), or PT_ERR_INVALID for a camera pt_tiles_floats rejects
static int whole_frame_grid(const PtCamera* cam, ptd::DevParams& d)
{
    PtParams p;
    pt_params_default(&p);
    p.passes = 1; p.first_pass = 0; p.rank = 0; p.world = 1;      // only the geometry is read
    return pt_fill_params(cam, &p, d);
}

int pt_accumulate_tile_list(const void* d_work, const PtCamera* cam, const PtParams* prm, const int32_t* d_list, int32_t n_tiles,
                            int32_t n_before, float* d_sum, float* d_m2, int32_t* d_tile_passes, void* hip_stream)
{
    if (!d_work || !d_list || !d_sum || !d_m2) { pt_set_error("pt_accumulate_tile_list: NULL argument"); return PT_ERR_INVALID; }
    if (!ptd::st_aligned(16, d_work, d_sum, d_m2) || !ptd::st_aligned(4, d_list, d_tile_passes)) {      // st_fold_list has no scalar twin
        pt_set_error("pt_accumulate_tile_list: d_work / d_sum / d_m2 not 16-byte or d_list / d_tile_passes not 4-byte aligned"); return PT_ERR_INVALID;
    }
    if (n_before < 0 || (prm && (long long)n_before + prm->passes > 0x7fffffffLL)) { pt_set_error("pt_accumulate_tile_list: bad n_before %d", n_before); return PT_ERR_INVALID; }
    ptd::DevParams d;
    const int rc = pt_fill_params(cam, prm, d);
    if (rc) return rc;
    if (prm->rank != 0 || prm->world != 1) { pt_set_error("pt_accumulate_tile_list: a tile list belongs to rank 0 of world 1: rank=%d world=%d", prm->rank, prm->world); return PT_ERR_INVALID; }
    if (n_tiles < 1 || n_tiles > d.n_tiles_total) { pt_set_error("pt_accumulate_tile_list: n_tiles=%d, the frame has %d tiles", n_tiles, d.n_tiles_total); return PT_ERR_INVALID; }
    const long long n4 = (long long)n_tiles * ptd::kTileVec;
    hipLaunchKernelGGL(ptd::st_fold_list, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, (hipStream_t)hip_stream,
                       (const float4*)ptk_wf_staging(const_cast<void*>(d_work)), d.passes, n4, d_list, d.n_tiles_total, n_before,
                       (float4*)d_sum, (float4*)d_m2, d_tile_passes);
    HIPCHK(hipGetLastError());
    return PT_OK;
}

int pt_tile_errors(const float* d_sum, const float* d_m2, const PtCamera* cam, const int32_t* d_list, int32_t n_tiles, int32_t n_passes,
                   PtTileError* d_err, void* hip_stream)
{
    if (!d_sum || !d_m2 || !d_err) { pt_set_error("pt_tile_errors: NULL argument"); return PT_ERR_INVALID; }
    if (!ptd::st_aligned(4, d_sum, d_m2, d_list) || !ptd::st_aligned(8, d_err)) { pt_set_error("pt_tile_errors: d_sum / d_m2 / d_list not 4-byte or d_err not 8-byte aligned"); return PT_ERR_INVALID; }
    if (n_passes < 2) { pt_set_error("pt_tile_errors: n_passes %d < 2", n_passes); return PT_ERR_INVALID; }
    ptd::DevParams d;
    const int rc = whole_frame_grid(cam, d);
    if (rc) return rc;
    if (n_tiles < 1 || n_tiles > d.n_tiles_total) { pt_set_error("pt_tile_errors: n_tiles=%d, the frame has %d tiles", n_tiles, d.n_tiles_total); return PT_ERR_INVALID; }
    hipLaunchKernelGGL(ptd::st_tile_errors, dim3((unsigned)((n_tiles + 3) / 4)), dim3(256), 0, (hipStream_t)hip_stream, d_sum, d_m2, d_list, n_tiles,
                       (float)n_passes, (float)(n_passes - 1), cam->W, cam->H, d.tiles_x, d.n_tiles_total, (ptd::StTileError*)d_err);
    HIPCHK(hipGetLastError());
    return PT_OK;
}

int pt_finish_tiles(const float* d_sum, const float* d_m2, const int32_t* d_tile_passes, const PtCamera* cam, float* d_mean, float* d_var,
                    void* hip_stream)
{
    if (!d_sum || !d_m2 || !d_tile_passes) { pt_set_error("pt_finish_tiles: NULL argument"); return PT_ERR_INVALID; }
    if (!d_mean && !d_var) { pt_set_error("pt_finish_tiles: neither a mean nor a variance buffer"); return PT_ERR_INVALID; }
    if (!ptd::st_aligned(16, d_sum, d_m2, d_mean, d_var) || !ptd::st_aligned(4, d_tile_passes)) {      // st_finish_tiles has no scalar twin
        pt_set_error("pt_finish_tiles: d_sum / d_m2 / d_mean / d_var not 16-byte or d_tile_passes not 4-byte aligned"); return PT_ERR_INVALID;
    }
    ptd::DevParams d;
    const int rc = whole_frame_grid(cam, d);
    if (rc) return rc;
    const long long n4 = (long long)d.n_tiles_total * ptd::kTileVec;
    hipLaunchKernelGGL(ptd::st_finish_tiles, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, (hipStream_t)hip_stream,
                       (const float4*)d_sum, (const float4*)d_m2, d_tile_passes, n4, (float4*)d_mean, (float4*)d_var);
    HIPCHK(hipGetLastError());
    return PT_OK;
}

int pt_render_adaptive(PtScene* s, const PtCamera* cam, const PtParams* prm, double target, int32_t min_passes, int32_t max_passes,
                       float* h_accum_rgb, float* h_mean_rgb, float* h_var_rgb, int32_t* h_tile_passes, double* h_tile_err,
                       PtAdaptiveReport* report)
{
    if (!s || !prm || !h_accum_rgb || !h_tile_passes || !report) { pt_set_error("pt_render_adaptive: NULL argument"); return PT_ERR_INVALID; }
    PtParams p = *prm; p.rank = 0; p.world = 1;
    if (p.passes < 1) { pt_set_error("pt_render_adaptive: batch of %d passes", p.passes); return PT_ERR_INVALID; }
    if (p.passes > max_passes) p.passes = max_passes;
    const int batch = p.passes;
    if (min_passes < 2) min_passes = 2;
    if (min_passes > max_passes || !(target >= 0.0)) { pt_set_error("pt_render_adaptive: need 2 <= min_passes %d <= max_passes %d and a target >= 0", min_passes, max_passes); return PT_ERR_INVALID; }
    PtParams all = p; all.passes = max_passes;              // the seed limit for the last pass that may be rendered
    const int64_t nt = pt_tiles_floats(cam, &all);
    if (nt < 0) return PT_ERR_INVALID;
    const int total = (int)(nt / (ptd::kTilePixels * 3));
    int64_t wb = pt_tile_list_work_bytes(cam, &p, total);   // the largest round: every tile x a full batch ...
    if (wb < 0) return PT_ERR_INVALID;
    if (max_passes % batch) {                               // ... or the shortened last batch
        PtParams q = p; q.passes = max_passes % batch;
        const int64_t w2 = pt_tile_list_work_bytes(cam, &q, total);
        if (w2 < 0) return PT_ERR_INVALID;
        if (w2 > wb) wb = w2;
    }
    HIPCHK(hipSetDevice(s->device));
    const size_t frameBytes = (size_t)cam->W * cam->H * 12;
    DevBuf b_tiles, b_sum, b_m2, b_var, b_work, b_list, b_np, b_err, b_frame;
    HIPCHK(b_tiles.alloc((size_t)nt * 4));                  // a round's list-major sums, then the mean
    HIPCHK(b_sum.alloc((size_t)nt * 4));
    HIPCHK(b_m2.alloc((size_t)nt * 4));
    if (h_var_rgb) HIPCHK(b_var.alloc((size_t)nt * 4));
    HIPCHK(b_work.alloc((size_t)wb));
    HIPCHK(b_list.alloc((size_t)total * 4));
    HIPCHK(b_np.alloc((size_t)total * 4));
    HIPCHK(b_err.alloc((size_t)total * sizeof(PtTileError)));
    HIPCHK(b_frame.alloc(frameBytes));
    float *d_tiles = b_tiles.as<float>(), *d_sum = b_sum.as<float>(), *d_m2 = b_m2.as<float>(), *d_frame = b_frame.as<float>();
    int32_t *d_list = b_list.as<int32_t>(), *d_np = b_np.as<int32_t>();

    std::vector<int32_t> active((size_t)total);
    for (int t = 0; t < total; t++) active[(size_t)t] = t;
    std::vector<PtTileError> errs((size_t)total);
    std::vector<double> lastErr((size_t)total, 0.0);
    PtAdaptiveReport rep{};
    rep.tiles = total;
    int done = 0;
    while (!active.empty() && done < max_passes) {
        const int n = (int)active.size();
        p.first_pass = prm->first_pass + done;              // every active tile holds exactly `done` passes
        p.passes = max_passes - done < batch ? max_passes - done : batch;
        HIPCHK(hipMemcpy(d_list, active.data(), (size_t)n * 4, hipMemcpyHostToDevice));
        int r = pt_render_tile_list(s, cam, &p, active.data(), n, d_tiles, b_work.as<>(), nullptr);
        if (!r) r = pt_accumulate_tile_list(b_work.as<>(), cam, &p, d_list, n, done, d_sum, d_m2, d_np, nullptr);
        if (r) return r;
        done += p.passes;
        rep.rounds++;
        rep.tile_passes += (int64_t)n * p.passes;
        if (done < min_passes) continue;
        r = pt_tile_errors(d_sum, d_m2, cam, d_list, n, done, b_err.as<PtTileError>(), nullptr);
        if (r) return r;
        HIPCHK(hipMemcpy(errs.data(), b_err.as<>(), (size_t)n * sizeof(PtTileError), hipMemcpyDeviceToHost));
        size_t keep = 0;
        for (int i = 0; i < n; i++) {
            const int32_t t = active[(size_t)i];
            const double e = errs[(size_t)i].mean_rel_se;
            lastErr[(size_t)t] = e;
            if (!(e <= target)) active[keep++] = t;         // a NaN stays active; the order is kept
        }
        active.resize(keep);
    }
    for (int t = 0; t < total; t++) {
        if (lastErr[(size_t)t] <= target) rep.tiles_converged++;
        if (lastErr[(size_t)t] > rep.max_tile_err) rep.max_tile_err = lastErr[(size_t)t];
    }
    HIPCHK(hipMemcpy(h_tile_passes, d_np, (size_t)total * 4, hipMemcpyDeviceToHost));
    if (h_tile_err) memcpy(h_tile_err, lastErr.data(), (size_t)total * sizeof(double));
    *report = rep;
    int r = pt_untile(d_sum, cam, 1, d_frame, nullptr);
    if (r) return r;
    HIPCHK(hipMemcpy(h_accum_rgb, d_frame, frameBytes, hipMemcpyDeviceToHost));
    if (h_mean_rgb || h_var_rgb) {
        r = pt_finish_tiles(d_sum, d_m2, d_np, cam, h_mean_rgb ? d_tiles : nullptr, h_var_rgb ? b_var.as<float>() : nullptr, nullptr);
        if (r) return r;
    }
    if (h_mean_rgb) {
        r = pt_untile(d_tiles, cam, 1, d_frame, nullptr);
        if (r) return r;
        HIPCHK(hipMemcpy(h_mean_rgb, d_frame, frameBytes, hipMemcpyDeviceToHost));
    }
    if (h_var_rgb) {
        r = pt_untile(b_var.as<float>(), cam, 1, d_frame, nullptr);
        if (r) return r;
        HIPCHK(hipMemcpy(h_var_rgb, d_frame, frameBytes, hipMemcpyDeviceToHost));
    }
    return PT_OK;
}

}  // extern "C"
