// pt_box.hip — which primitives lie inside or touch the caller's axis-aligned boxes, on an uploaded scene (include/pt_api.h: pt_box_count,
// pt_box_any, pt_box_list).  DESIGN.md section 41.
//
// All three are DEFINED without a tree, over B(Q) = { k : g(Q, k) <= bound } with the class key g of pt_box.h (0 inside, 1 touching,
// +inf no member) and bound = 1 (PT_BOX_TOUCHING) or 0 (PT_BOX_INSIDE): |B|, some member, and B in the lists' one order (g ascending,
// among equal g the larger index first: slot_before<false>, the bits of 0 and 1.0f order as ints).  The walk only has to find the
// members, by box-box overlap (pt_box.h says why that never disagrees with g).
//
// Shape: count_within's and near_list's (pt_knearest.hip) — one box per lane, one-wave workgroups — over pt_box.h's walk, whose
// per-lane LDS stack holds bare refs, entry e at stack[e * 64]: 10 KB a workgroup on the 4-wide tree, 8 KB on the binary one.  The sinks
// are pt_lists.h's: KCount, SlotOne<true>, SlotSeg<false, KCount> with fill_write_out and ptk_list_sort, Filtered around each (FLT).
#include <hip/hip_runtime.h>
#include "pt_device.h"
#include "pt_math.h"
#include "pt_trace.h"
#include "pt_scene.h"
#include "pt_box.h"
#include "pt_lists.h"

namespace ptd {

// Box i of the caller's BOX8 records (lo.xyz | reserved | hi.xyz | reserved), as two 16-byte loads
PT_DEV void load_box(const float4* __restrict__ boxes, size_t i, f3& lo, f3& hi)
{
    const float4 a = boxes[2 * i], b = boxes[2 * i + 1];
    lo = f3(a.x, a.y, a.z);
    hi = f3(b.x, b.y, b.z);
}

// A sink of this file with or without the filter of query i around it
template <bool FLT, class SINK>
PT_DEV auto box_sink(const SINK& s, const QFilter& flt, uint32_t i)
{
    if constexpr (FLT) return Filtered<SINK>{s, lane_filter(flt, i, 0.f)};
    else return s;
}

template <bool QUAD, bool FLT>
__global__ __launch_bounds__(64)
void box_count(DevScene sc, const float4* __restrict__ boxes, uint32_t n, float bound, QFilter flt, int32_t* __restrict__ out)
{
    __shared__ int lds_stack[(QUAD ? kQueryStack : kStackDepth) * 64];
    const uint32_t i = blockIdx.x * 64u + threadIdx.x;
    if (i >= n) return;
    f3 lo, hi;
    load_box(boxes, i, lo, hi);
    auto s = box_sink<FLT>(KCount{0, bound}, flt, i);
    box_query<QUAD>(sc, lo, hi, &lds_stack[threadIdx.x], s);
    out[i] = s.cnt;
}

// Some member of B, with its own key: the walk ends at the first one the sink takes
template <bool QUAD, bool FLT>
__global__ __launch_bounds__(64)
void box_any(DevScene sc, const float4* __restrict__ boxes, uint32_t n, float bound, QFilter flt, float2* __restrict__ out)
{
    __shared__ int lds_stack[(QUAD ? kQueryStack : kStackDepth) * 64];
    const uint32_t i = blockIdx.x * 64u + threadIdx.x;
    if (i >= n) return;
    f3 lo, hi;
    load_box(boxes, i, lo, hi);
    auto s = box_sink<FLT>(SlotOne<true>{bound, -1, 0.f, -1}, flt, i);
    box_query<QUAD>(sc, lo, hi, &lds_stack[threadIdx.x], s);
    out[i] = make_float2(s.key, __int_as_float(s.prim));      // a miss is (0, -1)
}

// The fill of pt_box_list: near_list's shape.  A lane whose segment is empty walks nothing.  Nothing outside [0, cap) is written:
// list_segment clamps.
template <bool QUAD, bool FLT>
__global__ __launch_bounds__(64)
void box_list(DevScene sc, const float4* __restrict__ boxes, uint32_t n, float bound, QFilter flt, const int64_t* __restrict__ off, int64_t cap,
              int2* __restrict__ out)
{
    __shared__ int lds_stack[(QUAD ? kQueryStack : kStackDepth) * 64];
    __shared__ int2 lds_list[kListLds * kSlotRow];
    const uint32_t lane = threadIdx.x, i = blockIdx.x * 64u + lane;
    if (i >= n) return;
    int64_t b, e;
    list_segment(off, i, cap, b, e);
    const int64_t m = e - b;
    if (m == 0) return;
    f3 lo, hi;
    load_box(boxes, i, lo, hi);
    int2* list = &lds_list[lane];
    int2* dst = out + b;
    auto s = box_sink<FLT>(SlotSeg<false, KCount>(list, dst, m, bound), flt, i);
    box_query<QUAD>(sc, lo, hi, &lds_stack[lane], s);
    fill_write_out(list, dst, m, s.cnt, s.append);
}

}  // namespace ptd

// launch(quad, flt) with the two as compile-time constants
template <class LAUNCH>
static void box_dispatch(bool quad, bool flt, LAUNCH launch)
{
    if (quad) { if (flt) launch(std::true_type(), std::true_type()); else launch(std::true_type(), std::false_type()); }
    else { if (flt) launch(std::false_type(), std::true_type()); else launch(std::false_type(), std::false_type()); }
}

// What a call of any of the three hands every batch: the walk, the class bound, and whether the filter selects at all
struct BoxCall {
    bool quad, flt;
    float bound;
    hipStream_t stream;
};

// Each enqueues one batch of n <= 2^30 boxes
static hipError_t launch_box_count(const ptd::DevScene& sc, const float* d_boxes8, uint32_t n, const BoxCall& c, const ptd::QFilter& flt, int32_t* d_count)
{
    const dim3 blocks((n + 63u) / 64u);
    box_dispatch(c.quad, c.flt, [&](auto q, auto f) {
        hipLaunchKernelGGL((ptd::box_count<q.value, f.value>), blocks, dim3(64), 0, c.stream, sc, (const float4*)d_boxes8, n, c.bound, flt, d_count);
    });
    return hipGetLastError();
}

static hipError_t launch_box_any(const ptd::DevScene& sc, const float* d_boxes8, uint32_t n, const BoxCall& c, const ptd::QFilter& flt, PtBoxMember* d_out)
{
    const dim3 blocks((n + 63u) / 64u);
    box_dispatch(c.quad, c.flt, [&](auto q, auto f) {
        hipLaunchKernelGGL((ptd::box_any<q.value, f.value>), blocks, dim3(64), 0, c.stream, sc, (const float4*)d_boxes8, n, c.bound, flt, (float2*)d_out);
    });
    return hipGetLastError();
}

// The fill, then the sort of the segments longer than kListLds.  off: the batch's first offset; the records are addressed from d_out
// whatever the batch.
static hipError_t launch_box_list(const ptd::DevScene& sc, const float* d_boxes8, uint32_t n, const BoxCall& c, const ptd::QFilter& flt, const int64_t* off,
                                  int64_t cap, PtBoxMember* d_out)
{
    const dim3 blocks((n + 63u) / 64u);
    int2* out = (int2*)d_out;
    box_dispatch(c.quad, c.flt, [&](auto q, auto f) {
        hipLaunchKernelGGL((ptd::box_list<q.value, f.value>), blocks, dim3(64), 0, c.stream, sc, (const float4*)d_boxes8, n, c.bound, flt, off, cap, out);
    });
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return ptk_list_sort(off, n, cap, out, false, c.stream);
}

// ---- entry points (include/pt_api.h): every argument check comes before the first HIP call ----------------------------------------
// outName / outAlign: "count" (4 bytes) or the PtBoxMember records "out" (8)
static int box_args_ok(const char* who, const PtScene* s, const float* boxes, int64_t n, int32_t flags, const char* outName, int outAlign, const void* out,
                       bool list, const int64_t* offsets, int64_t cap, bool device, const PtQueryFilter* filter)
{
    const char* param = (flags != PT_BOX_TOUCHING && flags != PT_BOX_INSIDE) ? "unknown flags" : nullptr;
    return pt_query_args(who, s, n, device, {"boxes", boxes, outName, out, outName, outAlign, "detail", nullptr, param, list, offsets, cap, filter, false});
}

static BoxCall box_call(const PtScene* s, int32_t flags, const PtQueryFilter* filter, void* hip_stream)
{
    return BoxCall{pt_query_walks_quad(s), !pt_filter_neutral(filter), flags == PT_BOX_INSIDE ? 0.f : 1.f, (hipStream_t)hip_stream};
}

extern "C" {

int pt_box_count(PtScene* s, const float* d_boxes8, int64_t n, int32_t flags, const PtQueryFilter* filter, int32_t* d_count, void* hip_stream)
{
    int rc;
    if ((rc = box_args_ok("pt_box_count", s, d_boxes8, n, flags, "count", 4, d_count, false, nullptr, 0, true, filter)) != PT_OK) return rc;
    if (n == 0) return PT_OK;
    HIPCHK(hipSetDevice(s->device));
    const BoxCall c = box_call(s, flags, filter, hip_stream);
    HIPCHK(pt_query_batches(n, [&](int64_t off, uint32_t m) {
        return launch_box_count(s->dev, d_boxes8 + off * 8, m, c, pt_filter_dev(c.flt ? filter : nullptr, off), d_count + off);
    }));
    return PT_OK;
}

int pt_box_any(PtScene* s, const float* d_boxes8, int64_t n, int32_t flags, const PtQueryFilter* filter, PtBoxMember* d_out, void* hip_stream)
{
    int rc;
    if ((rc = box_args_ok("pt_box_any", s, d_boxes8, n, flags, "out", 8, d_out, false, nullptr, 0, true, filter)) != PT_OK) return rc;
    if (n == 0) return PT_OK;
    HIPCHK(hipSetDevice(s->device));
    const BoxCall c = box_call(s, flags, filter, hip_stream);
    HIPCHK(pt_query_batches(n, [&](int64_t off, uint32_t m) {
        return launch_box_any(s->dev, d_boxes8 + off * 8, m, c, pt_filter_dev(c.flt ? filter : nullptr, off), d_out + off);
    }));
    return PT_OK;
}

int pt_box_list(PtScene* s, const float* d_boxes8, int64_t n, int32_t flags, const int64_t* d_offsets, int64_t cap, const PtQueryFilter* filter,
                PtBoxMember* d_out, void* hip_stream)
{
    int rc;
    if ((rc = box_args_ok("pt_box_list", s, d_boxes8, n, flags, "out", 8, d_out, true, d_offsets, cap, true, filter)) != PT_OK) return rc;
    if (n == 0) return PT_OK;
    HIPCHK(hipSetDevice(s->device));
    const BoxCall c = box_call(s, flags, filter, hip_stream);
    HIPCHK(pt_query_batches(n, [&](int64_t off, uint32_t m) {
        return launch_box_list(s->dev, d_boxes8 + off * 8, m, c, pt_filter_dev(c.flt ? filter : nullptr, off), d_offsets + off, cap, d_out);
    }));
    return PT_OK;
}

int pt_box_count_host(PtScene* s, const float* h_boxes8, int64_t n, int32_t flags, int32_t* h_count)
{
    int rc;
    if ((rc = box_args_ok("pt_box_count_host", s, h_boxes8, n, flags, "count", 4, h_count, false, nullptr, 0, false, nullptr)) != PT_OK) return rc;
    if (n == 0) return PT_OK;
    HIPCHK(hipSetDevice(s->device));
    return pt_host_query(h_boxes8, (size_t)n * 32, h_count, (size_t)n * 4, nullptr, 0, [&](float* d_boxes, void* d_count, float*) {
        return pt_box_count(s, d_boxes, n, flags, nullptr, (int32_t*)d_count, nullptr);
    });
}

int pt_box_any_host(PtScene* s, const float* h_boxes8, int64_t n, int32_t flags, PtBoxMember* h_out)
{
    int rc;
    if ((rc = box_args_ok("pt_box_any_host", s, h_boxes8, n, flags, "out", 8, h_out, false, nullptr, 0, false, nullptr)) != PT_OK) return rc;
    if (n == 0) return PT_OK;
    HIPCHK(hipSetDevice(s->device));
    return pt_host_query(h_boxes8, (size_t)n * 32, h_out, (size_t)n * 8, nullptr, 0, [&](float* d_boxes, void* d_out, float*) {
        return pt_box_any(s, d_boxes, n, flags, nullptr, (PtBoxMember*)d_out, nullptr);
    });
}

int pt_box_list_host(PtScene* s, const float* h_boxes8, int64_t n, int32_t flags, int64_t* h_offsets, int64_t cap, PtBoxMember* h_out)
{
    int rc;
    if ((rc = box_args_ok("pt_box_list_host", s, h_boxes8, n, flags, "out", 8, h_out, true, h_offsets, cap, false, nullptr)) != PT_OK) return rc;
    if (n == 0) { h_offsets[0] = 0; return PT_OK; }
    HIPCHK(hipSetDevice(s->device));
    return pt_host_list("pt_box_list_host", h_boxes8, n, 32, h_offsets, cap, h_out, nullptr, 0,
                        [&](float* d_boxes, int32_t* d_count) { return pt_box_count(s, d_boxes, n, flags, nullptr, d_count, nullptr); },
                        [&](float* d_boxes, int64_t* d_off, int64_t total, void* d_out, float*) {
                            return pt_box_list(s, d_boxes, n, flags, d_off, total, nullptr, (PtBoxMember*)d_out, nullptr);
                        });
}

}  // extern "C"
