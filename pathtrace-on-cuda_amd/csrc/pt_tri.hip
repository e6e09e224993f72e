// pt_tri.hip — which primitives of an uploaded scene the caller's own triangles cut, and along which segments (include/pt_api.h:
// pt_tri_count, pt_tri_any, pt_tri_list).  DESIGN.md section 44.
//
// All three are DEFINED without a tree, over M(T) = { k : key(T, k) = 1 } with the float32 key of pt_tri.h (1 member, +inf none): |M|,
// some member, and M with the larger index first (the lists' one order among equal keys: slot_before<false>).  The walk only has to find
// the members; pt_tri.h says why its cull never disagrees with the key.
//
// Shape: pt_box.hip's — one query per lane, one-wave workgroups, a per-lane LDS stack of bare refs, entry e at stack[e * 64]: 10 KB a
// workgroup on the 4-wide tree, 8 KB on the binary one.  A lane keeps qa, qb, n, its box and the three edge normals in 24 registers.
// The sinks are pt_lists.h's: KCount, SlotOne<true>, SlotSeg<false, KCount> with fill_write_out and ptk_list_sort, Filtered around each
// (FLT).  The segments of a list are a second pass over the filled and sorted slots (segments_detail): the key again for (query, prim)
// from the scene's current records.
#include <hip/hip_runtime.h>
#include "pt_device.h"
#include "pt_math.h"
#include "pt_trace.h"
#include "pt_scene.h"
#include "pt_tri.h"
#include "pt_lists.h"

namespace ptd {

// Query i of the caller's TRI12 records (a.xyz | - | b.xyz | - | c.xyz | -), as three 16-byte loads
struct TriQuery {
    TriLane L;
    f3 qc;
};
PT_DEV TriQuery load_tri(const float4* __restrict__ tris, size_t i)
{
    const float4 a = tris[3 * i], b = tris[3 * i + 1], c = tris[3 * i + 2];
    TriQuery t;
    t.qc = f3(c.x, c.y, c.z);
    t.L = tri_lane(f3(a.x, a.y, a.z), f3(b.x, b.y, b.z), t.qc);
    return t;
}

// A sink of this file with or without the filter of query i around it
template <bool FLT, class SINK>
PT_DEV auto tri_sink(const SINK& s, const QFilter& flt, uint32_t i)
{
    if constexpr (FLT) return Filtered<SINK>{s, lane_filter(flt, i, 0.f)};
    else return s;
}

template <bool QUAD, bool FLT>
__global__ __launch_bounds__(64)
void tri_count(DevScene sc, const float4* __restrict__ tris, uint32_t n, QFilter flt, int32_t* __restrict__ out)
{
    __shared__ int lds_stack[(QUAD ? kQueryStack : kStackDepth) * 64];
    const uint32_t i = blockIdx.x * 64u + threadIdx.x;
    if (i >= n) return;
    const TriQuery t = load_tri(tris, i);
    auto s = tri_sink<FLT>(KCount{0, 1.f}, flt, i);
    tri_query<QUAD>(sc, t.L, t.qc, &lds_stack[threadIdx.x], s);
    out[i] = s.cnt;
}

// Some member: the walk ends at the first one the sink takes
template <bool QUAD, bool FLT>
__global__ __launch_bounds__(64)
void tri_any(DevScene sc, const float4* __restrict__ tris, uint32_t n, QFilter flt, float2* __restrict__ out)
{
    __shared__ int lds_stack[(QUAD ? kQueryStack : kStackDepth) * 64];
    const uint32_t i = blockIdx.x * 64u + threadIdx.x;
    if (i >= n) return;
    const TriQuery t = load_tri(tris, i);
    auto s = tri_sink<FLT>(SlotOne<true>{1.f, -1, 0.f, -1}, flt, i);
    tri_query<QUAD>(sc, t.L, t.qc, &lds_stack[threadIdx.x], s);
    out[i] = make_float2(s.key, __int_as_float(s.prim));      // a miss is (0, -1)
}

// The fill of pt_tri_list: box_list's shape.  A lane whose segment is empty walks nothing.  Nothing outside [0, cap) is written:
// list_segment clamps.
template <bool QUAD, bool FLT>
__global__ __launch_bounds__(64)
void tri_list(DevScene sc, const float4* __restrict__ tris, uint32_t n, QFilter flt, const int64_t* __restrict__ off, int64_t cap, int2* __restrict__ out)
{
    __shared__ int lds_stack[(QUAD ? kQueryStack : kStackDepth) * 64];
    __shared__ int2 lds_list[kListLds * kSlotRow];
    const uint32_t lane = threadIdx.x, i = blockIdx.x * 64u + lane;
    if (i >= n) return;
    int64_t b, e;
    list_segment(off, i, cap, b, e);
    const int64_t m = e - b;
    if (m == 0) return;
    const TriQuery t = load_tri(tris, i);
    int2* list = &lds_list[lane];
    int2* dst = out + b;
    auto s = tri_sink<FLT>(SlotSeg<false, KCount>(list, dst, m, 1.f), flt, i);
    tri_query<QUAD>(sc, t.L, t.qc, &lds_stack[lane], s);
    fill_write_out(list, dst, m, s.cnt, s.append);
}

// The detail records of every segment, after the sort: tri_detail per member slot, zeros for a miss (pt_lists.h: segments_detail)
__global__ __launch_bounds__(kSegThreads)
void tri_list_detail(DevScene sc, const float4* __restrict__ tris, uint32_t n, uint32_t per, const int64_t* __restrict__ off, int64_t cap,
                     const int2* __restrict__ res, float* __restrict__ out8)
{
    segments_detail<8>(off, n, per, cap, res, out8, [&](uint32_t i) { return load_tri(tris, i); },
                       [&](const TriQuery& t, int2 h, float* o) { tri_detail(sc, t.L, t.qc, h.y, o); });
}

}  // namespace ptd

// launch(quad, flt) with the two as compile-time constants
template <class LAUNCH>
static void tri_dispatch(bool quad, bool flt, LAUNCH launch)
{
    if (quad) { if (flt) launch(std::true_type(), std::true_type()); else launch(std::true_type(), std::false_type()); }
    else { if (flt) launch(std::false_type(), std::true_type()); else launch(std::false_type(), std::false_type()); }
}

// What a call of any of the three hands every batch: the walk, and whether the filter selects at all
struct TriCall {
    bool quad, flt;
    hipStream_t stream;
};

// Each enqueues one batch of n <= 2^30 queries
static hipError_t launch_tri_count(const ptd::DevScene& sc, const float* d_tris12, uint32_t n, const TriCall& c, const ptd::QFilter& flt, int32_t* d_count)
{
    const dim3 blocks((n + 63u) / 64u);
    tri_dispatch(c.quad, c.flt, [&](auto q, auto f) {
        hipLaunchKernelGGL((ptd::tri_count<q.value, f.value>), blocks, dim3(64), 0, c.stream, sc, (const float4*)d_tris12, n, flt, d_count);
    });
    return hipGetLastError();
}

static hipError_t launch_tri_any(const ptd::DevScene& sc, const float* d_tris12, uint32_t n, const TriCall& c, const ptd::QFilter& flt, PtBoxMember* d_out)
{
    const dim3 blocks((n + 63u) / 64u);
    tri_dispatch(c.quad, c.flt, [&](auto q, auto f) {
        hipLaunchKernelGGL((ptd::tri_any<q.value, f.value>), blocks, dim3(64), 0, c.stream, sc, (const float4*)d_tris12, n, flt, (float2*)d_out);
    });
    return hipGetLastError();
}

// The fill, the sort of the segments longer than kListLds, then the segments if asked for.  off: the batch's first offset; the records
// and the detail are addressed from d_out and d_detail8 whatever the batch.
static hipError_t launch_tri_list(const ptd::DevScene& sc, const float* d_tris12, uint32_t n, const TriCall& c, const ptd::QFilter& flt, const int64_t* off,
                                  int64_t cap, PtBoxMember* d_out, float* d_detail8)
{
    const dim3 blocks((n + 63u) / 64u);
    int2* out = (int2*)d_out;
    tri_dispatch(c.quad, c.flt, [&](auto q, auto f) {
        hipLaunchKernelGGL((ptd::tri_list<q.value, f.value>), blocks, dim3(64), 0, c.stream, sc, (const float4*)d_tris12, n, flt, off, cap, out);
    });
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    if ((e = ptk_list_sort(off, n, cap, out, false, c.stream)) != hipSuccess) return e;
    if (d_detail8) {
        uint32_t per, grid;
        pt_list_grid(n, per, grid);
        hipLaunchKernelGGL(ptd::tri_list_detail, dim3(grid), dim3(ptd::kSegThreads), 0, c.stream, sc, (const float4*)d_tris12, n, per, off, cap,
                           (const int2*)out, d_detail8);
    }
    return hipGetLastError();
}

// ---- entry points (include/pt_api.h): every argument check comes before the first HIP call ----------------------------------------
// outName / outAlign: "count" (4 bytes) or the PtBoxMember records "out" (8)
static int tri_args_ok(const char* who, const PtScene* s, const float* tris, int64_t n, const char* outName, int outAlign, const void* out, bool list,
                       const int64_t* offsets, int64_t cap, const float* detail, bool device, const PtQueryFilter* filter)
{
    return pt_query_args(who, s, n, device, {"tris", tris, outName, out, outName, outAlign, "detail", detail, nullptr, list, offsets, cap, filter, false});
}

static TriCall tri_call(const PtScene* s, const PtQueryFilter* filter, void* hip_stream)
{
    return TriCall{pt_query_walks_quad(s), !pt_filter_neutral(filter), (hipStream_t)hip_stream};
}

extern "C" {

int pt_tri_count(PtScene* s, const float* d_tris12, int64_t n, const PtQueryFilter* filter, int32_t* d_count, void* hip_stream)
{
    int rc;
    if ((rc = tri_args_ok("pt_tri_count", s, d_tris12, n, "count", 4, d_count, false, nullptr, 0, nullptr, true, filter)) != PT_OK) return rc;
    if (n == 0) return PT_OK;
    HIPCHK(hipSetDevice(s->device));
    const TriCall c = tri_call(s, filter, hip_stream);
    HIPCHK(pt_query_batches(n, [&](int64_t off, uint32_t m) {
        return launch_tri_count(s->dev, d_tris12 + off * 12, m, c, pt_filter_dev(c.flt ? filter : nullptr, off), d_count + off);
    }));
    return PT_OK;
}

int pt_tri_any(PtScene* s, const float* d_tris12, int64_t n, const PtQueryFilter* filter, PtBoxMember* d_out, void* hip_stream)
{
    int rc;
    if ((rc = tri_args_ok("pt_tri_any", s, d_tris12, n, "out", 8, d_out, false, nullptr, 0, nullptr, true, filter)) != PT_OK) return rc;
    if (n == 0) return PT_OK;
    HIPCHK(hipSetDevice(s->device));
    const TriCall c = tri_call(s, filter, hip_stream);
    HIPCHK(pt_query_batches(n, [&](int64_t off, uint32_t m) {
        return launch_tri_any(s->dev, d_tris12 + off * 12, m, c, pt_filter_dev(c.flt ? filter : nullptr, off), d_out + off);
    }));
    return PT_OK;
}

int pt_tri_list(PtScene* s, const float* d_tris12, int64_t n, const int64_t* d_offsets, int64_t cap, const PtQueryFilter* filter, PtBoxMember* d_out,
                float* d_detail8, void* hip_stream)
{
    int rc;
    if ((rc = tri_args_ok("pt_tri_list", s, d_tris12, n, "out", 8, d_out, true, d_offsets, cap, d_detail8, true, filter)) != PT_OK) return rc;
    if (n == 0) return PT_OK;
    HIPCHK(hipSetDevice(s->device));
    const TriCall c = tri_call(s, filter, hip_stream);
    HIPCHK(pt_query_batches(n, [&](int64_t off, uint32_t m) {
        return launch_tri_list(s->dev, d_tris12 + off * 12, m, c, pt_filter_dev(c.flt ? filter : nullptr, off), d_offsets + off, cap, d_out, d_detail8);
    }));
    return PT_OK;
}

int pt_tri_count_host(PtScene* s, const float* h_tris12, int64_t n, int32_t* h_count)
{
    int rc;
    if ((rc = tri_args_ok("pt_tri_count_host", s, h_tris12, n, "count", 4, h_count, false, nullptr, 0, nullptr, false, nullptr)) != PT_OK) return rc;
    if (n == 0) return PT_OK;
    HIPCHK(hipSetDevice(s->device));
    return pt_host_query(h_tris12, (size_t)n * 48, h_count, (size_t)n * 4, nullptr, 0, [&](float* d_tris, void* d_count, float*) {
        return pt_tri_count(s, d_tris, n, nullptr, (int32_t*)d_count, nullptr);
    });
}

int pt_tri_any_host(PtScene* s, const float* h_tris12, int64_t n, PtBoxMember* h_out)
{
    int rc;
    if ((rc = tri_args_ok("pt_tri_any_host", s, h_tris12, n, "out", 8, h_out, false, nullptr, 0, nullptr, false, nullptr)) != PT_OK) return rc;
    if (n == 0) return PT_OK;
    HIPCHK(hipSetDevice(s->device));
    return pt_host_query(h_tris12, (size_t)n * 48, h_out, (size_t)n * 8, nullptr, 0, [&](float* d_tris, void* d_out, float*) {
        return pt_tri_any(s, d_tris, n, nullptr, (PtBoxMember*)d_out, nullptr);
    });
}

int pt_tri_list_host(PtScene* s, const float* h_tris12, int64_t n, int64_t* h_offsets, int64_t cap, PtBoxMember* h_out, float* h_detail8)
{
    int rc;
    if ((rc = tri_args_ok("pt_tri_list_host", s, h_tris12, n, "out", 8, h_out, true, h_offsets, cap, h_detail8, false, nullptr)) != PT_OK) return rc;
    if (n == 0) { h_offsets[0] = 0; return PT_OK; }
    HIPCHK(hipSetDevice(s->device));
    return pt_host_list("pt_tri_list_host", h_tris12, n, 48, h_offsets, cap, h_out, h_detail8, 32,
                        [&](float* d_tris, int32_t* d_count) { return pt_tri_count(s, d_tris, n, nullptr, d_count, nullptr); },
                        [&](float* d_tris, int64_t* d_off, int64_t total, void* d_out, float* d_det) {
                            return pt_tri_list(s, d_tris, n, d_off, total, nullptr, (PtBoxMember*)d_out, d_det, nullptr);
                        });
}

}  // extern "C"
