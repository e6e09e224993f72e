// pt_knearest.hip — the K nearest primitives within a radius, sorted, and the number of primitives within a radius, for the caller's points
// on an uploaded scene (include/pt_api.h: pt_nearest_k, pt_count_within).  DESIGN.md section 30.
//
// Both are DEFINED without a tree, over C(p) = { k : f(p, k) <= r2 } with the f of pt_nearest.h: the first K members of C in the order
// (f ascending, among equal f the larger index first), and |C|.  The walks only have to find them, by the inequality of section 29,
// f(p, k) >= boxdist2(p, box of k) >= boxdist2(p, any box that contains it), exact in float32: a child whose boxdist2 exceeds the bound
// holds no member that could enter.  The bound is r2 while the list holds fewer than K, then the f of its last slot (it only ever
// decreases); for the count it is r2 throughout.  What the closest query did not need: every triangle sits below exactly ONE leaf of
// the tree walked — a list would hold a triangle met twice in two slots, a count would count it twice.
//
// Shape: nearest_points' (pt_nearest.hip), the walk pt_nearest.h's knear_point — one point per lane, one-wave workgroups, the per-lane
// LDS stack of (bound, ref) entries with entry e at stack[e * 64].  Beside it the per-lane candidate list, sorted (pt_lists.h: SlotList),
// slot j at list[j * kSlotRow + lane] as int2 (f's bits, prim): squared distances are >= 0, so their bits order as ints.  The count and
// the bound live in registers.
#include <hip/hip_runtime.h>
#include "pt_device.h"
#include "pt_math.h"
#include "pt_trace.h"
#include "pt_scene.h"
#include "pt_nearest.h"
#include "pt_lists.h"

namespace ptd {

// The list of the K nearest: pt_lists.h's SlotList<false> (f's bits order as ints).  The count of C(p): pt_lists.h's KCount, the bound r2.

// KC: the capacity class of the list (pt_scene.h: pt_kc_dispatch).  The wave's 64 points own the 64 * k consecutive records from
// out[blockIdx.x * 64 * k]; every lane pads its list with miss records and the wave copies the block
// out of LDS in record order, 64 consecutive records (512 bytes) per store.
template <int KC, bool QUAD>
__global__ __launch_bounds__(64)
void nearest_k(DevScene sc, const float4* __restrict__ points, uint32_t n, int k, int2* __restrict__ out)
{
    __shared__ int2 lds_stack[(QUAD ? kQueryStack : kStackDepth) * 64];
    __shared__ int2 lds_list[KC * kSlotRow];
    if (k < 1 || k > KC) return;      // the launcher's choice of KC, restated where the list is indexed
    const uint32_t lane = threadIdx.x, base = blockIdx.x * 64u, i = base + lane;
    int2* list = &lds_list[lane];
    int cnt = 0;
    if (i < n) {
        const float4 q = points[i];
        SlotList<false> s{list, k, 0, q.w * q.w, -1};
        knear_point<QUAD>(sc, q, &lds_stack[lane], s);
        cnt = s.cnt;
    }
    for (int j = cnt; j < k; j++) list[j * kSlotRow] = make_int2(0, -1);      // a miss is (0, -1)
    __syncthreads();
    const uint32_t live = (n - base < 64u) ? n - base : 64u, total = live * (uint32_t)k;
    int2* dst = out + (size_t)base * (size_t)k;
    const int q64 = 64 / k, m64 = 64 % k;
    int t = (int)lane / k, j = (int)lane % k;      // record r is slot j of point t: r = t * k + j, t < live <= 64
    for (uint32_t r = lane; r < total; r += 64u) {
        dst[r] = lds_list[j * kSlotRow + t];
        j += m64;
        t += q64;
        if (j >= k) { j -= k; t++; }
    }
}

template <bool QUAD>
__global__ __launch_bounds__(64)
void count_within(DevScene sc, const float4* __restrict__ points, uint32_t n, int32_t* __restrict__ out)
{
    __shared__ int2 lds_stack[(QUAD ? kQueryStack : kStackDepth) * 64];
    const uint32_t i = blockIdx.x * 64u + threadIdx.x;
    if (i >= n) return;
    const float4 q = points[i];
    KCount s{0, q.w * q.w};
    knear_point<QUAD>(sc, q, &lds_stack[threadIdx.x], s);
    out[i] = s.cnt;
}

// The 8-float detail record of the header for every finished slot, one thread per slot; zeros for a miss slot.  Slot t belongs to point t / k.
// A launch covers the slots from `first` on (pt_scene.h: pt_detail_chunks).
__global__ __launch_bounds__(256)
void nearest_k_detail(DevScene sc, const float4* __restrict__ points, uint64_t first, uint64_t slots, uint32_t k, const int2* __restrict__ res, float* __restrict__ out8)
{
    const uint64_t t = first + (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (t >= slots) return;
    const int prim = res[t].y;
    float* o = out8 + t * 8;
    if (prim < 0) { for (int c = 0; c < 8; c++) o[c] = 0.f; return; }
    near_detail(sc, points[t / k], prim, o);
}

// ---- every primitive within the radius: the fill of pt_within_radius_list (pt_lists.h says which code sorts
// which segment) ----
// One point per lane, nearest_k's shape with the list of class kListLds and the sink SlotSeg, whose long segments take KCount's
// members.  A lane whose segment is empty walks nothing.  Nothing outside [0, cap) is written: list_segment clamps.
template <bool QUAD>
__global__ __launch_bounds__(64)
void near_list(DevScene sc, const float4* __restrict__ points, uint32_t n, const int64_t* __restrict__ off, int64_t cap, int2* __restrict__ out)
{
    __shared__ int2 lds_stack[(QUAD ? kQueryStack : kStackDepth) * 64];
    __shared__ int2 lds_list[kListLds * kSlotRow];
    const uint32_t lane = threadIdx.x, i = blockIdx.x * 64u + lane;
    if (i >= n) return;
    int64_t b, e;
    list_segment(off, i, cap, b, e);
    const int64_t m = e - b;
    if (m == 0) return;
    const float4 q = points[i];
    int2* list = &lds_list[lane];
    int2* dst = out + b;
    SlotSeg<false, KCount> s(list, dst, m, q.w * q.w);
    knear_point<QUAD>(sc, q, &lds_stack[lane], s);
    fill_write_out(list, dst, m, s.cnt, s.append);
}

// The detail records of every segment, after the sort: near_detail per member slot (pt_lists.h: segments_detail)
__global__ __launch_bounds__(kSegThreads)
void near_list_detail(DevScene sc, const float4* __restrict__ points, uint32_t n, uint32_t per, const int64_t* __restrict__ off, int64_t cap,
                      const int2* __restrict__ res, float* __restrict__ out8)
{
    segments_detail<8>(off, n, per, cap, res, out8, [&](uint32_t i) { return points[i]; },
                       [&](const float4& q, int2 h, float* o) { near_detail(sc, q, h.y, o); });
}

// ---- the filtered forms (include/pt_api.h: "Query filters") ----------------------------------------------------
// The kernels above with their sink behind pt_lists.h's Filtered: the same walk, the same one-wave workgroups and LDS layouts, the
// same capacity classes.  A point query has no near bound.

// pt_closest_points_f: the first member of C' — the shared point walk over the one-slot sink —, or (ANY) some member
template <bool ANY, bool QUAD>
__global__ __launch_bounds__(64)
void near_one_f(DevScene sc, const float4* __restrict__ points, uint32_t n, QFilter flt, float2* __restrict__ out)
{
    __shared__ int2 lds_stack[(QUAD ? kQueryStack : kStackDepth) * 64];
    const uint32_t i = blockIdx.x * 64u + threadIdx.x;
    if (i >= n) return;
    const float4 q = points[i];
    Filtered<SlotOne<ANY>> s{{q.w * q.w, -1, 0.f, -1}, lane_filter(flt, i, 0.f)};
    knear_point<QUAD>(sc, q, &lds_stack[threadIdx.x], s);
    out[i] = make_float2(s.key, __int_as_float(s.prim));      // a miss is (0, -1)
}

template <int KC, bool QUAD>
__global__ __launch_bounds__(64)
void nearest_k_f(DevScene sc, const float4* __restrict__ points, uint32_t n, int k, QFilter flt, int2* __restrict__ out)
{
    __shared__ int2 lds_stack[(QUAD ? kQueryStack : kStackDepth) * 64];
    __shared__ int2 lds_list[KC * kSlotRow];
    if (k < 1 || k > KC) return;      // the launcher's choice of KC, restated where the list is indexed
    const uint32_t lane = threadIdx.x, base = blockIdx.x * 64u, i = base + lane;
    int2* list = &lds_list[lane];
    int cnt = 0;
    if (i < n) {
        const float4 q = points[i];
        Filtered<SlotList<false>> s{{list, k, 0, q.w * q.w, -1}, lane_filter(flt, i, 0.f)};
        knear_point<QUAD>(sc, q, &lds_stack[lane], s);
        cnt = s.cnt;
    }
    for (int j = cnt; j < k; j++) list[j * kSlotRow] = make_int2(0, -1);      // a miss is (0, -1)
    __syncthreads();
    klist_copy_out(lds_list, out, base, n, k);
}

template <bool QUAD>
__global__ __launch_bounds__(64)
void count_within_f(DevScene sc, const float4* __restrict__ points, uint32_t n, QFilter flt, int32_t* __restrict__ out)
{
    __shared__ int2 lds_stack[(QUAD ? kQueryStack : kStackDepth) * 64];
    const uint32_t i = blockIdx.x * 64u + threadIdx.x;
    if (i >= n) return;
    const float4 q = points[i];
    Filtered<KCount> s{{0, q.w * q.w}, lane_filter(flt, i, 0.f)};
    knear_point<QUAD>(sc, q, &lds_stack[threadIdx.x], s);
    out[i] = s.cnt;
}

// The fill: a long segment's appended members are Filtered<KCount>'s members, the filtered count's
template <bool QUAD>
__global__ __launch_bounds__(64)
void near_list_f(DevScene sc, const float4* __restrict__ points, uint32_t n, QFilter flt, const int64_t* __restrict__ off, int64_t cap,
                 int2* __restrict__ out)
{
    __shared__ int2 lds_stack[(QUAD ? kQueryStack : kStackDepth) * 64];
    __shared__ int2 lds_list[kListLds * kSlotRow];
    const uint32_t lane = threadIdx.x, i = blockIdx.x * 64u + lane;
    if (i >= n) return;
    int64_t b, e;
    list_segment(off, i, cap, b, e);
    const int64_t m = e - b;
    if (m == 0) return;
    const float4 q = points[i];
    int2* list = &lds_list[lane];
    int2* dst = out + b;
    Filtered<SlotSeg<false, KCount>> s{SlotSeg<false, KCount>(list, dst, m, q.w * q.w), lane_filter(flt, i, 0.f)};
    knear_point<QUAD>(sc, q, &lds_stack[lane], s);
    fill_write_out(list, dst, m, s.cnt, s.append);
}

}  // namespace ptd

// Enqueues one batch of n <= 2^30 points on `stream`: k records per point, then the detail records if asked for
static hipError_t launch_nearest_k(const ptd::DevScene& sc, const float* d_points4, uint32_t n, int k, bool quad, PtNearest* d_out, float* d_detail8, hipStream_t stream)
{
    const float4* pts = (const float4*)d_points4;
    int2* out = (int2*)d_out;
    const dim3 blocks((n + 63u) / 64u);
    pt_kc_dispatch(k, [&](auto kc) {
        if (quad) hipLaunchKernelGGL((ptd::nearest_k<kc, true>), blocks, dim3(64), 0, stream, sc, pts, n, k, out);
        else hipLaunchKernelGGL((ptd::nearest_k<kc, false>), blocks, dim3(64), 0, stream, sc, pts, n, k, out);
    });
    if (d_detail8)
        pt_detail_chunks((uint64_t)n * (uint64_t)k, [&](uint64_t first, dim3 grid) {
            hipLaunchKernelGGL(ptd::nearest_k_detail, grid, dim3(256), 0, stream, sc, pts, first, (uint64_t)n * (uint64_t)k, (uint32_t)k, (const int2*)out, d_detail8);
        });
    return hipGetLastError();
}

static hipError_t launch_count_within(const ptd::DevScene& sc, const float* d_points4, uint32_t n, bool quad, int32_t* d_count, hipStream_t stream)
{
    const dim3 blocks((n + 63u) / 64u);
    if (quad) hipLaunchKernelGGL((ptd::count_within<true>), blocks, dim3(64), 0, stream, sc, (const float4*)d_points4, n, d_count);
    else hipLaunchKernelGGL((ptd::count_within<false>), blocks, dim3(64), 0, stream, sc, (const float4*)d_points4, n, d_count);
    return hipGetLastError();
}

// Enqueues one batch of n <= 2^30 points of pt_within_radius_list on `stream`: the fill, the sort of the segments longer than kListLds,
// then the detail records if asked for.  off: the batch's first offset; the records are addressed from d_out whatever the batch.
static hipError_t launch_near_list(const ptd::DevScene& sc, const float* d_points4, uint32_t n, bool quad, const int64_t* off, int64_t cap,
                                   PtNearest* d_out, float* d_detail8, hipStream_t stream)
{
    const dim3 blocks((n + 63u) / 64u);
    const float4* pts = (const float4*)d_points4;
    int2* out = (int2*)d_out;
    if (quad) hipLaunchKernelGGL((ptd::near_list<true>), blocks, dim3(64), 0, stream, sc, pts, n, off, cap, out);
    else hipLaunchKernelGGL((ptd::near_list<false>), blocks, dim3(64), 0, stream, sc, pts, n, off, cap, out);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    if ((e = ptk_list_sort(off, n, cap, out, false, stream)) != hipSuccess) return e;
    if (d_detail8) {
        uint32_t per, grid;
        pt_list_grid(n, per, grid);
        hipLaunchKernelGGL(ptd::near_list_detail, dim3(grid), dim3(ptd::kSegThreads), 0, stream, sc, pts, n, per, off, cap, (const int2*)out, d_detail8);
    }
    return hipGetLastError();
}

// ---- the filtered forms' launchers: as the ones above, over the _f kernels ---------------------------------------------------------
// pt_nearest.hip's pt_closest_points_f: (dist2, prim) per point; its detail records are that file's
hipError_t ptk_near_one_f(const ptd::DevScene& sc, const float* d_points4, uint32_t n, bool any, bool quad, const ptd::QFilter& flt, PtNearest* d_out,
                          hipStream_t stream)
{
    const dim3 blocks((n + 63u) / 64u);
    const float4* pts = (const float4*)d_points4;
    float2* out = (float2*)d_out;
    if (quad) {
        if (any) hipLaunchKernelGGL((ptd::near_one_f<true, true>), blocks, dim3(64), 0, stream, sc, pts, n, flt, out);
        else hipLaunchKernelGGL((ptd::near_one_f<false, true>), blocks, dim3(64), 0, stream, sc, pts, n, flt, out);
    } else {
        if (any) hipLaunchKernelGGL((ptd::near_one_f<true, false>), blocks, dim3(64), 0, stream, sc, pts, n, flt, out);
        else hipLaunchKernelGGL((ptd::near_one_f<false, false>), blocks, dim3(64), 0, stream, sc, pts, n, flt, out);
    }
    return hipGetLastError();
}

static hipError_t launch_nearest_k_f(const ptd::DevScene& sc, const float* d_points4, uint32_t n, int k, bool quad, const ptd::QFilter& flt, PtNearest* d_out,
                                     float* d_detail8, hipStream_t stream)
{
    const float4* pts = (const float4*)d_points4;
    int2* out = (int2*)d_out;
    const dim3 blocks((n + 63u) / 64u);
    pt_kc_dispatch(k, [&](auto kc) {
        if (quad) hipLaunchKernelGGL((ptd::nearest_k_f<kc, true>), blocks, dim3(64), 0, stream, sc, pts, n, k, flt, out);
        else hipLaunchKernelGGL((ptd::nearest_k_f<kc, false>), blocks, dim3(64), 0, stream, sc, pts, n, k, flt, out);
    });
    if (d_detail8)
        pt_detail_chunks((uint64_t)n * (uint64_t)k, [&](uint64_t first, dim3 grid) {
            hipLaunchKernelGGL(ptd::nearest_k_detail, grid, dim3(256), 0, stream, sc, pts, first, (uint64_t)n * (uint64_t)k, (uint32_t)k, (const int2*)out, d_detail8);
        });
    return hipGetLastError();
}

static hipError_t launch_count_within_f(const ptd::DevScene& sc, const float* d_points4, uint32_t n, bool quad, const ptd::QFilter& flt, int32_t* d_count,
                                        hipStream_t stream)
{
    const dim3 blocks((n + 63u) / 64u);
    if (quad) hipLaunchKernelGGL((ptd::count_within_f<true>), blocks, dim3(64), 0, stream, sc, (const float4*)d_points4, n, flt, d_count);
    else hipLaunchKernelGGL((ptd::count_within_f<false>), blocks, dim3(64), 0, stream, sc, (const float4*)d_points4, n, flt, d_count);
    return hipGetLastError();
}

static hipError_t launch_near_list_f(const ptd::DevScene& sc, const float* d_points4, uint32_t n, bool quad, const ptd::QFilter& flt, const int64_t* off,
                                     int64_t cap, PtNearest* d_out, float* d_detail8, hipStream_t stream)
{
    const dim3 blocks((n + 63u) / 64u);
    const float4* pts = (const float4*)d_points4;
    int2* out = (int2*)d_out;
    if (quad) hipLaunchKernelGGL((ptd::near_list_f<true>), blocks, dim3(64), 0, stream, sc, pts, n, flt, off, cap, out);
    else hipLaunchKernelGGL((ptd::near_list_f<false>), blocks, dim3(64), 0, stream, sc, pts, n, flt, off, cap, out);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    if ((e = ptk_list_sort(off, n, cap, out, false, stream)) != hipSuccess) return e;
    if (d_detail8) {
        uint32_t per, grid;
        pt_list_grid(n, per, grid);
        hipLaunchKernelGGL(ptd::near_list_detail, dim3(grid), dim3(ptd::kSegThreads), 0, stream, sc, pts, n, per, off, cap, (const int2*)out, d_detail8);
    }
    return hipGetLastError();
}

// ---- entry points (include/pt_api.h): every argument check comes before the first HIP call ----------------------------------------
// has_k: pt_nearest_k and its host variant (PtNearest records), else the counts
static int knear_args_ok(const char* who, const PtScene* s, const float* points, int64_t n, bool has_k, int32_t k, const void* out,
                         const float* detail, bool device, const PtQueryFilter* filter = nullptr)
{
    const char* param = (has_k && (k < 1 || k > PT_NEAREST_KMAX)) ? "k must be in 1 .. PT_NEAREST_KMAX" : nullptr;
    return pt_query_args(who, s, n, device, {"points", points, "out", out, has_k ? "out" : "count", has_k ? 8 : 4, "detail", detail, param, false, nullptr, 0,
                                             filter, false});
}

// pt_within_radius_list and its host variant
static int near_list_args_ok(const char* who, const PtScene* s, const float* points, int64_t n, const int64_t* offsets, int64_t cap,
                             const void* out, const float* detail, bool device, const PtQueryFilter* filter = nullptr)
{
    return pt_query_args(who, s, n, device, {"points", points, "out", out, "out", 8, "detail", detail, nullptr, true, offsets, cap, filter, false});
}

extern "C" {

int pt_nearest_k(PtScene* s, const float* d_points4, int64_t n, int32_t k, PtNearest* d_out, float* d_detail8, void* hip_stream)
{
    int rc;
    if ((rc = knear_args_ok("pt_nearest_k", s, d_points4, n, true, k, d_out, d_detail8, true)) != PT_OK) return rc;
    if (n == 0) return PT_OK;
    HIPCHK(hipSetDevice(s->device));
    const bool quad = pt_query_walks_quad(s);
    HIPCHK(pt_query_batches(n, [&](int64_t off, uint32_t m) {
        return launch_nearest_k(s->dev, d_points4 + off * 4, m, k, quad, d_out + off * k, d_detail8 ? d_detail8 + off * k * 8 : nullptr, (hipStream_t)hip_stream);
    }));
    return PT_OK;
}

int pt_nearest_k_host(PtScene* s, const float* h_points4, int64_t n, int32_t k, PtNearest* h_out, float* h_detail8)
{
    int rc;
    if ((rc = knear_args_ok("pt_nearest_k_host", s, h_points4, n, true, k, h_out, h_detail8, false)) != PT_OK) return rc;
    if (n == 0) return PT_OK;
    HIPCHK(hipSetDevice(s->device));
    const size_t slots = (size_t)n * (size_t)k;
    return pt_host_query(h_points4, (size_t)n * 16, h_out, slots * 8, h_detail8, slots * 32, [&](float* d_pts, void* d_out, float* d_det) {
        return pt_nearest_k(s, d_pts, n, k, (PtNearest*)d_out, d_det, nullptr);
    });
}

int pt_count_within(PtScene* s, const float* d_points4, int64_t n, int32_t* d_count, void* hip_stream)
{
    int rc;
    if ((rc = knear_args_ok("pt_count_within", s, d_points4, n, false, 0, d_count, nullptr, true)) != PT_OK) return rc;
    if (n == 0) return PT_OK;
    HIPCHK(hipSetDevice(s->device));
    const bool quad = pt_query_walks_quad(s);
    HIPCHK(pt_query_batches(n, [&](int64_t off, uint32_t m) {
        return launch_count_within(s->dev, d_points4 + off * 4, m, quad, d_count + off, (hipStream_t)hip_stream);
    }));
    return PT_OK;
}

int pt_count_within_host(PtScene* s, const float* h_points4, int64_t n, int32_t* h_count)
{
    int rc;
    if ((rc = knear_args_ok("pt_count_within_host", s, h_points4, n, false, 0, h_count, nullptr, false)) != PT_OK) return rc;
    if (n == 0) return PT_OK;
    HIPCHK(hipSetDevice(s->device));
    return pt_host_query(h_points4, (size_t)n * 16, h_count, (size_t)n * 4, nullptr, 0, [&](float* d_pts, void* d_count, float*) {
        return pt_count_within(s, d_pts, n, (int32_t*)d_count, nullptr);
    });
}

int pt_within_radius_list(PtScene* s, const float* d_points4, int64_t n, const int64_t* d_offsets, int64_t cap, PtNearest* d_out, float* d_detail8,
                          void* hip_stream)
{
    int rc;
    if ((rc = near_list_args_ok("pt_within_radius_list", s, d_points4, n, d_offsets, cap, d_out, d_detail8, true)) != PT_OK) return rc;
    if (n == 0) return PT_OK;
    HIPCHK(hipSetDevice(s->device));
    const bool quad = pt_query_walks_quad(s);
    HIPCHK(pt_query_batches(n, [&](int64_t off, uint32_t m) {
        return launch_near_list(s->dev, d_points4 + off * 4, m, quad, d_offsets + off, cap, d_out, d_detail8, (hipStream_t)hip_stream);
    }));
    return PT_OK;
}

int pt_within_radius_list_host(PtScene* s, const float* h_points4, int64_t n, int64_t* h_offsets, int64_t cap, PtNearest* h_out, float* h_detail8)
{
    int rc;
    if ((rc = near_list_args_ok("pt_within_radius_list_host", s, h_points4, n, h_offsets, cap, h_out, h_detail8, false)) != PT_OK) return rc;
    if (n == 0) { h_offsets[0] = 0; return PT_OK; }
    HIPCHK(hipSetDevice(s->device));
    return pt_host_list("pt_within_radius_list_host", h_points4, n, 16, h_offsets, cap, h_out, h_detail8, 32,
                        [&](float* d_pts, int32_t* d_count) { return pt_count_within(s, d_pts, n, d_count, nullptr); },
                        [&](float* d_pts, int64_t* d_off, int64_t total, void* d_out, float* d_det) {
                            return pt_within_radius_list(s, d_pts, n, d_off, total, (PtNearest*)d_out, d_det, nullptr);
                        });
}

// ---- the filtered forms: the twin's checks, then the filter's; a neutral filter enqueues the twin itself ---------------------------
int pt_nearest_k_f(PtScene* s, const float* d_points4, int64_t n, int32_t k, const PtQueryFilter* filter, PtNearest* d_out, float* d_detail8,
                   void* hip_stream)
{
    int rc;
    if ((rc = knear_args_ok("pt_nearest_k_f", s, d_points4, n, true, k, d_out, d_detail8, true, filter)) != PT_OK) return rc;
    if (n == 0) return PT_OK;
    if (pt_filter_neutral(filter)) return pt_nearest_k(s, d_points4, n, k, d_out, d_detail8, hip_stream);
    HIPCHK(hipSetDevice(s->device));
    const bool quad = pt_query_walks_quad(s);
    HIPCHK(pt_query_batches(n, [&](int64_t off, uint32_t m) {
        return launch_nearest_k_f(s->dev, d_points4 + off * 4, m, k, quad, pt_filter_dev(filter, off), d_out + off * k,
                                  d_detail8 ? d_detail8 + off * k * 8 : nullptr, (hipStream_t)hip_stream);
    }));
    return PT_OK;
}

int pt_count_within_f(PtScene* s, const float* d_points4, int64_t n, const PtQueryFilter* filter, int32_t* d_count, void* hip_stream)
{
    int rc;
    if ((rc = knear_args_ok("pt_count_within_f", s, d_points4, n, false, 0, d_count, nullptr, true, filter)) != PT_OK) return rc;
    if (n == 0) return PT_OK;
    if (pt_filter_neutral(filter)) return pt_count_within(s, d_points4, n, d_count, hip_stream);
    HIPCHK(hipSetDevice(s->device));
    const bool quad = pt_query_walks_quad(s);
    HIPCHK(pt_query_batches(n, [&](int64_t off, uint32_t m) {
        return launch_count_within_f(s->dev, d_points4 + off * 4, m, quad, pt_filter_dev(filter, off), d_count + off, (hipStream_t)hip_stream);
    }));
    return PT_OK;
}

int pt_within_radius_list_f(PtScene* s, const float* d_points4, int64_t n, const int64_t* d_offsets, int64_t cap, const PtQueryFilter* filter,
                            PtNearest* d_out, float* d_detail8, void* hip_stream)
{
    int rc;
    if ((rc = near_list_args_ok("pt_within_radius_list_f", s, d_points4, n, d_offsets, cap, d_out, d_detail8, true, filter)) != PT_OK) return rc;
    if (n == 0) return PT_OK;
    if (pt_filter_neutral(filter)) return pt_within_radius_list(s, d_points4, n, d_offsets, cap, d_out, d_detail8, hip_stream);
    HIPCHK(hipSetDevice(s->device));
    const bool quad = pt_query_walks_quad(s);
    HIPCHK(pt_query_batches(n, [&](int64_t off, uint32_t m) {
        return launch_near_list_f(s->dev, d_points4 + off * 4, m, quad, pt_filter_dev(filter, off), d_offsets + off, cap, d_out, d_detail8,
                                  (hipStream_t)hip_stream);
    }));
    return PT_OK;
}

}  // extern "C"
