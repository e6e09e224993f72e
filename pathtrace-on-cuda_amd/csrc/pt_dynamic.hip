// pt_dynamic.hip — moving the triangles of an uploaded scene: every array a render reads that depends on a vertex is recomputed
// from the new positions, on the caller's stream (include/pt_api.h: "Dynamic geometry").
//
// The RESULT of a render is defined by the triangles and the reference leaf boxes (host/accel_build.cpp); the traversal trees only
// steer the search, and any conservative box gives the same frame.  So the topology of both trees is kept (a refit) and
//   * the records (surf, tri, tripair, leafbox, lights) are the host's own expressions (host/bvh_build.cpp: flatten_tri, build) on
//     the new vertices — the library is compiled without contraction and with correctly rounded divide / sqrt, so they come out
//     bit for bit as pt_bvh_build_sah + pt_scene_create would write them;
//   * the binary traversal tree is refit bottom up into a scratch array of UNPADDED boxes per builder node, one launch per height
//     over a height-sorted node list (a kernel boundary is the only ordering between a node and its children);
//   * `nodes` and `quad` are re-derived from the unpadded boxes with the padding and the outward 8-bit quantisation of
//     host/accel_build.cpp (Emit::run), one thread per record, child refs untouched;
//   * the core box (scheduling hint) is recomputed over the triangles classified small at upload.
// Selections are written as comparisons (pt_dyn_device.h: min2 / max2), not fminf, so that the sign of a zero comes out as on the host.
#include <hip/hip_runtime.h>
#include <cfloat>
#include <cmath>
#include <cstring>
#include <utility>
#include <vector>

#include "pt_scene.h"
#include "pt_dyn_device.h"
#include "../host/accel_build.h"

namespace {

using ptd::DynScene;
using ptd::Tri9;
using ptd::Edges;
using ptd::load_tri;
using ptd::edges_of;
using ptd::min2;
using ptd::max2;

__device__ __forceinline__ float pad_lo(float v) { return v - (fabsf(v) * 1.52587890625e-5f + 1e-30f); }      // accel_build.cpp
__device__ __forceinline__ float pad_hi(float v) { return v + (fabsf(v) * 1.52587890625e-5f + 1e-30f); }

__device__ __forceinline__ void grow(float* mn, float* mx, const Tri9& t)
{
    for (int d = 0; d < 3; d++) {
        mn[d] = min2(mn[d], min2(t.v0[d], min2(t.v1[d], t.v2[d])));      // bvh_build.cpp: build
        mx[d] = max2(mx[d], max2(t.v0[d], max2(t.v1[d], t.v2[d])));
    }
}

// ---- records ----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void dyn_leafbox(DynScene s, const float* __restrict__ pos)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= s.n_leaves) return;
    const int2 r = s.leaf_range[i];
    float mn[3] = {FLT_MAX, FLT_MAX, FLT_MAX}, mx[3] = {-FLT_MAX, -FLT_MAX, -FLT_MAX};
    for (int k = 0; k < r.y; k++) grow(mn, mx, load_tri(pos, r.x + k));
    s.leafbox[(size_t)i * 2] = make_float4(mn[0], mn[1], mn[2], mx[0]);
    s.leafbox[(size_t)i * 2 + 1] = make_float4(mx[1], mx[2], 0.f, 0.f);
}

// ... and the scene's own copy of the positions (`keep`): a material update makes light records from it (pt_material.hip)
__global__ __launch_bounds__(256) void dyn_surf(DynScene s, const float* __restrict__ pos, const float* __restrict__ frames, float* __restrict__ keep)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= s.n_tris) return;
    const Tri9 t = load_tri(pos, i);
    float* k9 = keep + (size_t)i * 9;
    for (int k = 0; k < 3; k++) { k9[k] = t.v0[k]; k9[3 + k] = t.v1[k]; k9[6 + k] = t.v2[k]; }
    const Edges e = edges_of(t);
    float4* rec = s.surf + (size_t)i * 12;
    rec[0] = make_float4(t.v0[0], t.v0[1], t.v0[2], e.e1[0]);
    rec[1] = make_float4(e.e1[1], e.e1[2], e.e2[0], e.e2[1]);
    if (frames) {
        const float* f = frames + (size_t)i * 27;
        rec[2] = make_float4(e.e2[2], f[0], f[1], f[2]);
        for (int k = 0; k < 6; k++) rec[3 + k] = make_float4(f[3 + 4 * k], f[4 + 4 * k], f[5 + 4 * k], f[6 + 4 * k]);
    } else {
        float4 keep = rec[2];
        keep.x = e.e2[2];
        rec[2] = keep;
    }
}

// tri record q and pair record q (triangles q and q + 1 interleaved + their reference leaf boxes: dyn_leafbox has run)
__global__ __launch_bounds__(256) void dyn_tri(DynScene s, const float* __restrict__ pos)
{
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= s.n_tris) return;
    const int2 ma = s.tmap[q];
    const int2 mc = s.tmap[q + 1 < s.n_tris ? q + 1 : q];
    const Tri9 ta = load_tri(pos, ma.x), tc = load_tri(pos, mc.x);
    const Edges ea = edges_of(ta), ec = edges_of(tc);
    float4* a = s.tri + (size_t)q * 3;
    a[0] = make_float4(ta.v0[0], ta.v0[1], ta.v0[2], __int_as_float(ma.x));
    a[1] = make_float4(ea.e1[0], ea.e1[1], ea.e1[2], __int_as_float(ma.y));
    a[2] = make_float4(ea.e2[0], ea.e2[1], ea.e2[2], 0.f);
    const float4 la0 = s.leafbox[(size_t)ma.y * 2], la1 = s.leafbox[(size_t)ma.y * 2 + 1];
    const float4 lc0 = s.leafbox[(size_t)mc.y * 2], lc1 = s.leafbox[(size_t)mc.y * 2 + 1];
    float4* r = s.tripair + (size_t)q * 8;
    r[0] = make_float4(ta.v0[0], tc.v0[0], ta.v0[1], tc.v0[1]);
    r[1] = make_float4(ta.v0[2], tc.v0[2], ea.e1[0], ec.e1[0]);
    r[2] = make_float4(ea.e1[1], ec.e1[1], ea.e1[2], ec.e1[2]);
    r[3] = make_float4(ea.e2[0], ec.e2[0], ea.e2[1], ec.e2[1]);
    r[4] = make_float4(ea.e2[2], ec.e2[2], __int_as_float(ma.x), __int_as_float(mc.x));
    r[5] = la0;
    r[6] = make_float4(la1.x, la1.y, lc0.x, lc0.y);
    r[7] = make_float4(lc0.z, lc0.w, lc1.x, lc1.y);
}

__global__ __launch_bounds__(64) void dyn_lights(DynScene s, const float* __restrict__ pos)
{
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= s.n_lights) return;
    ptd::write_light(s.lights + (size_t)i * 4, load_tri(pos, s.light_prim[i]));
}

// ---- binary traversal tree: unpadded boxes, one launch per height -------------------------------------------------------------
__global__ __launch_bounds__(256) void dyn_refit_level(DynScene s, const float* __restrict__ pos, int first, int count)
{
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= count) return;
    const int node = s.order[first + j];
    const int4 n = s.bn[node];
    float mn[3], mx[3];
    if (n.w > 0) {
        for (int d = 0; d < 3; d++) { mn[d] = FLT_MAX; mx[d] = -FLT_MAX; }
        for (int k = 0; k < n.w; k++) grow(mn, mx, load_tri(pos, s.tmap[n.z + k].x));
    } else {
        const float4 l0 = s.bbox[(size_t)n.x * 2], l1 = s.bbox[(size_t)n.x * 2 + 1];
        const float4 r0 = s.bbox[(size_t)n.y * 2], r1 = s.bbox[(size_t)n.y * 2 + 1];
        mn[0] = min2(l0.x, r0.x); mn[1] = min2(l0.y, r0.y); mn[2] = min2(l0.z, r0.z);
        mx[0] = max2(l1.x, r1.x); mx[1] = max2(l1.y, r1.y); mx[2] = max2(l1.z, r1.z);
    }
    s.bbox[(size_t)node * 2] = make_float4(mn[0], mn[1], mn[2], 0.f);
    s.bbox[(size_t)node * 2 + 1] = make_float4(mx[0], mx[1], mx[2], 0.f);
    if (node == 0) {
        // the largest |coordinate| of any node is the root's: the 4-wide tree's absolute pad needs nothing from the host
        float m = 0.f;
        for (int d = 0; d < 3; d++) m = max2(m, max2(fabsf(mn[d]), fabsf(mx[d])));
        *s.maxabs = m;
    }
}

// ---- `nodes`: padded boxes of the two children of every record ----------------------------------------------------------------
__global__ __launch_bounds__(256) void dyn_nodes(DynScene s)
{
    const int w = blockIdx.x * 256 + threadIdx.x;
    if (w >= s.n_wide) return;
    const int2 c = s.wide_bn[w];
    const float4 l0 = s.bbox[(size_t)c.x * 2], l1 = s.bbox[(size_t)c.x * 2 + 1];
    const float4 r0 = s.bbox[(size_t)c.y * 2], r1 = s.bbox[(size_t)c.y * 2 + 1];
    float4* r = s.nodes + (size_t)w * 4;
    r[0] = make_float4(pad_lo(l0.x), pad_lo(l0.y), pad_lo(l0.z), pad_hi(l1.x));
    r[1] = make_float4(pad_hi(l1.y), pad_hi(l1.z), pad_lo(r0.x), pad_lo(r0.y));
    r[2] = make_float4(pad_lo(r0.z), pad_hi(r1.x), pad_hi(r1.y), pad_hi(r1.z));
}

// ---- `quad`: origin, power-of-two scale and outward 8-bit boxes of the 2-4 children (accel_build.cpp: Emit::run) ---------------
__global__ __launch_bounds__(256) void dyn_quad(DynScene s)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= s.n_quad) return;
    const int4 c4 = s.quad_bn[i];
    const int ch[4] = {c4.x, c4.y, c4.z, c4.w};
    const float absPad = *s.maxabs * 9.5367431640625e-7f;      // 2^-20
    int nc = 0;
    float lo[4][3], hi[4][3];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        if (ch[k] < 0) continue;
        nc = k + 1;
        const float4 b0 = s.bbox[(size_t)ch[k] * 2], b1 = s.bbox[(size_t)ch[k] * 2 + 1];
        lo[k][0] = pad_lo(b0.x) - absPad; lo[k][1] = pad_lo(b0.y) - absPad; lo[k][2] = pad_lo(b0.z) - absPad;
        hi[k][0] = pad_hi(b1.x) + absPad; hi[k][1] = pad_hi(b1.y) + absPad; hi[k][2] = pad_hi(b1.z) + absPad;
    }
    float org[3], scl[3];
    uint32_t qlo[3], qhi[3];
#pragma unroll
    for (int a = 0; a < 3; a++) {
        float mn = lo[0][a], mx = hi[0][a];
#pragma unroll
        for (int k = 1; k < 4; k++) if (k < nc) { mn = min2(mn, lo[k][a]); mx = max2(mx, hi[k][a]); }
        org[a] = mn;
        int ex = -100;
        if (mx > mn) { int t; (void)frexpf((mx - mn) / 255.f, &t); ex = t - 1 > -100 ? t - 1 : -100; }
        for (;;) {
            const float sc = ldexpf(1.f, ex);
            bool ok = true;
            uint32_t wl = 0, wh = 0;
#pragma unroll
            for (int k = 0; k < 4; k++) {
                if (!ok) continue;
                int ql, qh;
                if (k < nc) {
                    ql = (int)floorf((lo[k][a] - mn) / sc);
                    if (ql < 0) ql = 0;
                    while (ql > 0 && mn + sc * (float)ql > lo[k][a]) ql--;
                    qh = (int)ceilf((hi[k][a] - mn) / sc);
                    if (qh < ql) qh = ql;
                    while (qh <= 255 && mn + sc * (float)qh < hi[k][a]) qh++;
                    if (qh > 255 || ql > 255) { ok = false; continue; }
                } else { ql = 255; qh = 0; }      // no child: an inverted box
                wl |= (uint32_t)ql << (8 * k); wh |= (uint32_t)qh << (8 * k);
            }
            // finite positions always fit at some exponent; the bound only ends the search for an input outside the contract
            if (ok || ex >= 127) { qlo[a] = wl; qhi[a] = wh; scl[a] = sc; break; }
            ex++;
        }
    }
    uint4* q = s.quad + (size_t)i * 4;      // q[1] = the child refs: as built
    q[0] = make_uint4(__float_as_uint(org[0]), __float_as_uint(org[1]), __float_as_uint(org[2]), __float_as_uint(scl[0]));
    q[2] = make_uint4(qlo[0], qlo[1], qlo[2], qhi[0]);
    q[3] = make_uint4(qhi[1], qhi[2], __float_as_uint(scl[1]), __float_as_uint(scl[2]));
}

// ---- core box: the box of the triangles classified small at upload, padded as pt_scene_create pads it ------------------------------
__device__ __forceinline__ void block_minmax6(float* v, float* lds)      // v[0..2] min, v[3..5] max; result in lds[0..5] of thread 0's view
{
    for (int off = 32; off > 0; off >>= 1)
        for (int k = 0; k < 6; k++) {
            const float o = __shfl_down(v[k], off, 64);
            v[k] = k < 3 ? fminf(v[k], o) : fmaxf(v[k], o);
        }
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) for (int k = 0; k < 6; k++) lds[wave * 6 + k] = v[k];
    __syncthreads();
    if (threadIdx.x == 0)
        for (int w = 1; w < 4; w++) for (int k = 0; k < 6; k++) lds[k] = k < 3 ? fminf(lds[k], lds[w * 6 + k]) : fmaxf(lds[k], lds[w * 6 + k]);
}

__global__ __launch_bounds__(256) void dyn_core_partial(DynScene s, const float* __restrict__ pos)
{
    __shared__ float lds[24];
    float v[6] = {1e30f, 1e30f, 1e30f, -1e30f, -1e30f, -1e30f};
    for (int i = blockIdx.x * 256 + threadIdx.x; i < s.n_tris; i += ptd::kCoreBlocks * 256) {
        if (!s.small[i]) continue;
        const Tri9 t = load_tri(pos, i);
        for (int k = 0; k < 3; k++) {
            v[k] = fminf(v[k], fminf(t.v0[k], fminf(t.v1[k], t.v2[k])));
            v[3 + k] = fmaxf(v[3 + k], fmaxf(t.v0[k], fmaxf(t.v1[k], t.v2[k])));
        }
    }
    block_minmax6(v, lds);
    if (threadIdx.x == 0) for (int k = 0; k < 6; k++) s.core_partial[blockIdx.x * 8 + k] = lds[k];
}

__global__ __launch_bounds__(256) void dyn_core_final(DynScene s)
{
    __shared__ float lds[24];
    float v[6];
    for (int k = 0; k < 6; k++) v[k] = s.core_partial[threadIdx.x * 8 + k];      // kCoreBlocks == the block size
    block_minmax6(v, lds);
    if (threadIdx.x == 0) {
        const float4 b0 = s.bbox[0], b1 = s.bbox[1];      // the root box = the scene's
        const float dx = b1.x - b0.x, dy = b1.y - b0.y, dz = b1.z - b0.z;
        const float sd = sqrtf(dx * dx + dy * dy + dz * dz);
        for (int k = 0; k < 3; k++) {
            const float pad = 0.01f * (lds[3 + k] - lds[k]) + 1e-4f * sd;      // pt_scene.hip: core_box
            s.core[k] = lds[k] - pad;
            s.core[3 + k] = lds[3 + k] + pad;
        }
    }
}

// ---- sum of the box areas (pt_scene_tree_inflation), in the order of host/accel_build.cpp: pt_accel_area_sum ---------------------
__global__ __launch_bounds__(256) void dyn_area(DynScene s)
{
    __shared__ double v[256];
    const int base = blockIdx.x * kAreaBlock + threadIdx.x * 4;
    double acc = 0.0;
    for (int j = 0; j < 4; j++) {
        const int i = base + j;
        if (i < s.n_bn) {
            const float4 b0 = s.bbox[(size_t)i * 2], b1 = s.bbox[(size_t)i * 2 + 1];
            acc += (double)ptd::box_area(b1.x - b0.x, b1.y - b0.y, b1.z - b0.z);
        }
    }
    v[threadIdx.x] = acc;
    __syncthreads();
    for (int st = 128; st > 0; st >>= 1) {
        if ((int)threadIdx.x < st) v[threadIdx.x] += v[threadIdx.x + st];
        __syncthreads();
    }
    if (threadIdx.x == 0) s.area_partial[blockIdx.x] = v[0];
}

inline unsigned blocks_of(int n, int per) { return (unsigned)((n + per - 1) / per); }

}  // namespace

static_assert(ptd::kCoreBlocks == 256, "dyn_core_final reads one partial per thread of a 256-thread block");
static_assert(kAreaBlock == 1024, "dyn_area folds 4 boxes per thread of a 256-thread block");

// Enqueues the whole update on `stream` (pt_scene.h).  level_start: host array of n_levels + 1 offsets into `order` (height h = one launch).
hipError_t pt_dyn_launch_update(const DynScene& s, const float* d_pos, const float* d_frames, float* d_keep, const int32_t* level_start, int n_levels,
                                bool trees_only, hipStream_t stream)
{
    // records: the leaf boxes first, the pair records carry them inline
    if (!trees_only) {
        hipLaunchKernelGGL(dyn_leafbox, dim3(blocks_of(s.n_leaves, 256)), dim3(256), 0, stream, s, d_pos);
        hipLaunchKernelGGL(dyn_surf, dim3(blocks_of(s.n_tris, 256)), dim3(256), 0, stream, s, d_pos, d_frames, d_keep);
    }
    hipLaunchKernelGGL(dyn_tri, dim3(blocks_of(s.n_tris, 256)), dim3(256), 0, stream, s, d_pos);
    if (!trees_only && s.n_lights > 0) hipLaunchKernelGGL(dyn_lights, dim3(blocks_of(s.n_lights, 64)), dim3(64), 0, stream, s, d_pos);
    // binary tree, bottom up
    for (int h = 0; h < n_levels; h++) {
        const int first = level_start[h], count = level_start[h + 1] - first;
        if (count > 0) hipLaunchKernelGGL(dyn_refit_level, dim3(blocks_of(count, 256)), dim3(256), 0, stream, s, d_pos, first, count);
    }
    hipLaunchKernelGGL(dyn_nodes, dim3(blocks_of(s.n_wide, 256)), dim3(256), 0, stream, s);
    hipLaunchKernelGGL(dyn_quad, dim3(blocks_of(s.n_quad, 256)), dim3(256), 0, stream, s);
    if (!trees_only && s.core && s.small) {
        hipLaunchKernelGGL(dyn_core_partial, dim3(ptd::kCoreBlocks), dim3(256), 0, stream, s, d_pos);
        hipLaunchKernelGGL(dyn_core_final, dim3(1), dim3(256), 0, stream, s);
    }
    return hipGetLastError();
}

hipError_t pt_dyn_launch_area(const DynScene& s, hipStream_t stream)
{
    hipLaunchKernelGGL(dyn_area, dim3(blocks_of(s.n_bn, kAreaBlock)), dim3(256), 0, stream, s);
    return hipGetLastError();
}

// First update of a scene, of its vertices or of its materials: the maps of the build and the positions go to the device and the
// scratch is allocated; the host copies are dropped.
int pt_dyn_prepare(PtScene* s)
{
    if (s->dyn_ready) return PT_OK;
    PtScene::DynHost& h = s->dyn_host;
    ptd::DynScene& d = s->dyn;
    const size_t area_blocks = ((size_t)d.n_bn + kAreaBlock - 1) / kAreaBlock;
    const size_t mat_blocks = ((size_t)d.n_tris + kMatBlock - 1) / kMatBlock;
    // in the order of enum DynAlloc: the maps and the positions with their host source, then the scratch (area_partial: (n_bn + 1023) / 1024
    // doubles; the material update's partials: one int2 per kMatBlock triangles and one for the total)
    const struct { const void* src; size_t bytes; } plan[kDynAllocs] = {
        {h.bn.data(), h.bn.size() * 4}, {h.order.data(), h.order.size() * 4}, {h.wide_bn.data(), h.wide_bn.size() * 4}, {h.quad_bn.data(), h.quad_bn.size() * 4},
        {h.leaf_range.data(), h.leaf_range.size() * 4}, {h.tmap.data(), h.tmap.size() * 4}, {h.light_prim.data(), h.light_prim.size() * 4}, {h.small.data(), h.small.size()},
        {h.pos.data(), h.pos.size() * 4},
        {nullptr, (size_t)d.n_bn * 32}, {nullptr, 16}, {nullptr, (size_t)ptd::kCoreBlocks * 32}, {nullptr, area_blocks * 8}, {nullptr, (mat_blocks + 1) * 8}};
    // built beside the scene and moved in only once all of them exist: a failure frees what it got and leaves the scene as it was,
    // byte count included, and a later update may try again
    DevBuf fresh[kDynAllocs];
    int64_t bytes = 0;
    for (int k = 0; k < kDynAllocs; k++) {
        if (k == kDynSmall && h.small.empty()) continue;      // no core box: dyn.small stays null
        HIPCHK(k < kDynBbox ? fresh[k].upload(plan[k].src, plan[k].bytes) : fresh[k].alloc(plan[k].bytes));
        bytes += (int64_t)fresh[k].held();
    }
    if (!s->h_mat) HIPCHK(hipHostMalloc((void**)&s->h_mat, 8, hipHostMallocDefault));
    DevBuf* b = s->dyn_buf;
    for (int k = 0; k < kDynAllocs; k++) b[k] = std::move(fresh[k]);
    s->bytes += bytes;
    d.bn = b[kDynBn].as<const int4>(); d.order = b[kDynOrder].as<const int32_t>(); d.wide_bn = b[kDynWideBn].as<const int2>(); d.quad_bn = b[kDynQuadBn].as<const int4>();
    d.leaf_range = b[kDynLeafRange].as<const int2>(); d.tmap = b[kDynTmap].as<const int2>(); d.light_prim = b[kDynLightPrim].as<const int32_t>();
    d.small = b[kDynSmall].as<const uint8_t>();
    d.bbox = b[kDynBbox].as<float4>(); d.maxabs = b[kDynMaxabs].as<float>(); d.core_partial = b[kDynCorePartial].as<float>(); d.area_partial = b[kDynAreaPartial].as<double>();
    s->h_area.assign(area_blocks, 0.0);
    for (std::vector<int32_t>* v : {&h.bn, &h.order, &h.wide_bn, &h.quad_bn, &h.leaf_range, &h.tmap, &h.light_prim}) std::vector<int32_t>().swap(*v);
    std::vector<uint8_t>().swap(h.small);      // level_start stays: the launch sequence reads it
    std::vector<float>().swap(h.pos);
    s->dyn_ready = true;
    return PT_OK;
}

// ---- entry points (include/pt_api.h): every argument check comes before the first HIP call ----------------------------------------
extern "C" {

int pt_scene_update_vertices(PtScene* s, const float* d_pos, const float* d_frames, void* hip_stream)
{
    if (!s || !d_pos) { pt_set_error("pt_scene_update_vertices: NULL %s", !s ? "scene" : "d_pos"); return PT_ERR_INVALID; }
    HIPCHK(hipSetDevice(s->device));
    int rc;
    if ((rc = pt_dyn_prepare(s)) != PT_OK) return rc;
    hipStream_t st = (hipStream_t)hip_stream;
    HIPCHK(pt_dyn_launch_update(s->dyn, d_pos, d_frames, s->dyn_buf[kDynPos].as<float>(), s->dyn_host.level_start.data(), (int)s->dyn_host.level_start.size() - 1,
                                /*trees_only=*/false, st));
    s->updated = true;
    return PT_OK;
}

int pt_scene_update_vertices_host(PtScene* s, const float* h_pos, const float* h_frames)
{
    if (!s || !h_pos) { pt_set_error("pt_scene_update_vertices_host: NULL %s", !s ? "scene" : "h_pos"); return PT_ERR_INVALID; }
    HIPCHK(hipSetDevice(s->device));
    const size_t n = (size_t)s->dev.n_tris;
    DevBuf d_pos, d_frames;      // d_frames stays null when the caller passed no frames
    HIPCHK(d_pos.upload(h_pos, n * 36));
    if (h_frames) HIPCHK(d_frames.upload(h_frames, n * 108));
    const int rc = pt_scene_update_vertices(s, d_pos.as<float>(), d_frames.as<float>(), nullptr);
    if (rc != PT_OK) return rc;
    HIPCHK(hipStreamSynchronize(nullptr));
    return PT_OK;
}

int pt_scene_update_spheres(PtScene* s, const PtSphere* h_spheres, int32_t n_spheres)
{
    if (!s || !h_spheres) { pt_set_error("pt_scene_update_spheres: NULL %s", !s ? "scene" : "h_spheres"); return PT_ERR_INVALID; }
    if (n_spheres != s->dev.n_spheres || n_spheres < 1) {
        pt_set_error("pt_scene_update_spheres: %d spheres given, the scene has %d", n_spheres, s->dev.n_spheres);
        return PT_ERR_INVALID;
    }
    for (int i = 0; i < n_spheres; i++)      // h_spheres: as uploaded, or as the last pt_scene_update_sphere_materials left them
        if (memcmp(&h_spheres[i].mat, &s->h_spheres[(size_t)i * 16 + 4], sizeof(PtMaterial)) != 0) {
            pt_set_error("pt_scene_update_spheres: the material of sphere %d differs from the uploaded one (only centre and radius may change)", i);
            return PT_ERR_INVALID;
        }
    HIPCHK(hipSetDevice(s->device));
    for (int i = 0; i < n_spheres; i++) {
        float* a = &s->h_spheres[(size_t)i * 16];
        a[0] = h_spheres[i].center[0]; a[1] = h_spheres[i].center[1]; a[2] = h_spheres[i].center[2]; a[3] = h_spheres[i].rad;
    }
    HIPCHK(hipMemcpy(s->arr[kArrSpheres].as<>(), s->h_spheres.data(), (size_t)n_spheres * 64, hipMemcpyHostToDevice));      // ordered on the NULL stream
    return PT_OK;
}

int pt_scene_tree_inflation(PtScene* s, double* ratio)
{
    if (!s || !ratio) { pt_set_error("pt_scene_tree_inflation: NULL %s", !s ? "scene" : "ratio"); return PT_ERR_INVALID; }
    *ratio = 1.0;
    if (!s->updated) return PT_OK;
    HIPCHK(hipSetDevice(s->device));
    HIPCHK(hipDeviceSynchronize());      // the stream of the last update may be gone by now: wait for the device, reduce on the NULL stream
    HIPCHK(pt_dyn_launch_area(s->dyn, nullptr));
    HIPCHK(hipMemcpy(s->h_area.data(), s->dyn.area_partial, s->h_area.size() * 8, hipMemcpyDeviceToHost));
    double sum = 0.0;
    for (double v : s->h_area) sum += v;      // block sums in index order (host/accel_build.cpp: pt_accel_area_sum)
    *ratio = sum / s->dyn_host.area_sum;
    return PT_OK;
}

}  // extern "C"
