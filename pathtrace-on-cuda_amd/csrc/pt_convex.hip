// pt_convex.hip — which primitives lie inside or touch the caller's convex regions (frusta, oriented boxes, slabs: the intersection of up
// to 8 half-spaces), on an uploaded scene (include/pt_api.h: pt_convex_count, pt_convex_any, pt_convex_list, pt_camera_frustum).
// DESIGN.md section 42.
//
// All three are DEFINED without a tree, over C(Q) = { k : h(Q, k) <= bound } with the class key h of pt_convex.h (0 inside, 1 touching,
// +inf no member) and bound = 1 (PT_CONVEX_TOUCHING) or 0 (PT_CONVEX_INSIDE): |C|, some member, and C in the lists' one order (h
// ascending, among equal h the larger index first).  The walk only has to find the members, by the minimising corner of a node's box
// against every plane (pt_convex.h says why that never disagrees with h).
//
// Shape: pt_box.hip's — one region per lane, one-wave workgroups — over pt_convex.h's walks, whose per-lane LDS stack holds bare refs,
// entry e at stack[e * 64]: 10 KB a workgroup on the 4-wide tree, 8 KB on the binary one.  A lane's planes live in registers (at most
// 32 VGPRs, m 16-byte loads), not in LDS: the stack is what kQueryWaves is sized on.  The sinks are pt_lists.h's: KCount,
// SlotOne<true>, SlotSeg<false, KCount> with fill_write_out and ptk_list_sort, Filtered around each (FLT).
#include <hip/hip_runtime.h>
#include <cmath>
#include "pt_device.h"
#include "pt_math.h"
#include "pt_trace.h"
#include "pt_scene.h"
#include "pt_convex.h"
#include "pt_lists.h"

namespace ptd {

// Region i of the caller's PLANE4 records (n.xyz | d), m per region, as m 16-byte loads; the planes from m on are never read by a
// loop (every one is guarded by j < m) and hold the neutral plane
PT_DEV void load_planes(const float4* __restrict__ planes, size_t i, int m, float4 (&pl)[kConvexPlanes])
{
    const float4* p = planes + i * (size_t)m;
#pragma unroll
    for (int j = 0; j < kConvexPlanes; j++) {
        pl[j] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (j < m) pl[j] = p[j];
    }
}

// A sink of this file with or without the filter of query i around it
template <bool FLT, class SINK>
PT_DEV auto convex_sink(const SINK& s, const QFilter& flt, uint32_t i)
{
    if constexpr (FLT) return Filtered<SINK>{s, lane_filter(flt, i, 0.f)};
    else return s;
}

template <bool QUAD, bool FLT>
__global__ __launch_bounds__(64)
void convex_count(DevScene sc, const float4* __restrict__ planes, uint32_t n, int m, float bound, QFilter flt, int32_t* __restrict__ out)
{
    __shared__ int lds_stack[(QUAD ? kQueryStack : kStackDepth) * 64];
    const uint32_t i = blockIdx.x * 64u + threadIdx.x;
    if (i >= n) return;
    float4 pl[kConvexPlanes];
    load_planes(planes, i, m, pl);
    auto s = convex_sink<FLT>(KCount{0, bound}, flt, i);
    convex_query<QUAD>(sc, pl, m, &lds_stack[threadIdx.x], s);
    out[i] = s.cnt;
}

// Some member of C, with its own key: the walk ends at the first one the sink takes
template <bool QUAD, bool FLT>
__global__ __launch_bounds__(64)
void convex_any(DevScene sc, const float4* __restrict__ planes, uint32_t n, int m, float bound, QFilter flt, float2* __restrict__ out)
{
    __shared__ int lds_stack[(QUAD ? kQueryStack : kStackDepth) * 64];
    const uint32_t i = blockIdx.x * 64u + threadIdx.x;
    if (i >= n) return;
    float4 pl[kConvexPlanes];
    load_planes(planes, i, m, pl);
    auto s = convex_sink<FLT>(SlotOne<true>{bound, -1, 0.f, -1}, flt, i);
    convex_query<QUAD>(sc, pl, m, &lds_stack[threadIdx.x], s);
    out[i] = make_float2(s.key, __int_as_float(s.prim));      // a miss is (0, -1)
}

// The fill of pt_convex_list: box_list's shape.  A lane whose segment is empty walks nothing.  Nothing outside [0, cap) is written:
// list_segment clamps.
template <bool QUAD, bool FLT>
__global__ __launch_bounds__(64)
void convex_list(DevScene sc, const float4* __restrict__ planes, uint32_t n, int m, float bound, QFilter flt, const int64_t* __restrict__ off,
                 int64_t cap, int2* __restrict__ out)
{
    __shared__ int lds_stack[(QUAD ? kQueryStack : kStackDepth) * 64];
    __shared__ int2 lds_list[kListLds * kSlotRow];
    const uint32_t lane = threadIdx.x, i = blockIdx.x * 64u + lane;
    if (i >= n) return;
    int64_t b, e;
    list_segment(off, i, cap, b, e);
    const int64_t len = e - b;
    if (len == 0) return;
    float4 pl[kConvexPlanes];
    load_planes(planes, i, m, pl);
    int2* list = &lds_list[lane];
    int2* dst = out + b;
    auto s = convex_sink<FLT>(SlotSeg<false, KCount>(list, dst, len, bound), flt, i);
    convex_query<QUAD>(sc, pl, m, &lds_stack[lane], s);
    fill_write_out(list, dst, len, s.cnt, s.append);
}

}  // namespace ptd

// launch(quad, flt) with the two as compile-time constants
template <class LAUNCH>
static void convex_dispatch(bool quad, bool flt, LAUNCH launch)
{
    if (quad) { if (flt) launch(std::true_type(), std::true_type()); else launch(std::true_type(), std::false_type()); }
    else { if (flt) launch(std::false_type(), std::true_type()); else launch(std::false_type(), std::false_type()); }
}

// What a call of any of the three hands every batch: the walk, the planes per region, the class bound, and whether the filter selects
struct ConvexCall {
    bool quad, flt;
    int m;
    float bound;
    hipStream_t stream;
};

// Each enqueues one batch of n <= 2^30 regions
static hipError_t launch_convex_count(const ptd::DevScene& sc, const float* d_planes4, uint32_t n, const ConvexCall& c, const ptd::QFilter& flt, int32_t* d_count)
{
    const dim3 blocks((n + 63u) / 64u);
    convex_dispatch(c.quad, c.flt, [&](auto q, auto f) {
        hipLaunchKernelGGL((ptd::convex_count<q.value, f.value>), blocks, dim3(64), 0, c.stream, sc, (const float4*)d_planes4, n, c.m, c.bound, flt, d_count);
    });
    return hipGetLastError();
}

static hipError_t launch_convex_any(const ptd::DevScene& sc, const float* d_planes4, uint32_t n, const ConvexCall& c, const ptd::QFilter& flt, PtBoxMember* d_out)
{
    const dim3 blocks((n + 63u) / 64u);
    convex_dispatch(c.quad, c.flt, [&](auto q, auto f) {
        hipLaunchKernelGGL((ptd::convex_any<q.value, f.value>), blocks, dim3(64), 0, c.stream, sc, (const float4*)d_planes4, n, c.m, c.bound, flt, (float2*)d_out);
    });
    return hipGetLastError();
}

// The fill, then the sort of the segments longer than kListLds.  off: the batch's first offset; the records are addressed from d_out
// whatever the batch.
static hipError_t launch_convex_list(const ptd::DevScene& sc, const float* d_planes4, uint32_t n, const ConvexCall& c, const ptd::QFilter& flt,
                                     const int64_t* off, int64_t cap, PtBoxMember* d_out)
{
    const dim3 blocks((n + 63u) / 64u);
    int2* out = (int2*)d_out;
    convex_dispatch(c.quad, c.flt, [&](auto q, auto f) {
        hipLaunchKernelGGL((ptd::convex_list<q.value, f.value>), blocks, dim3(64), 0, c.stream, sc, (const float4*)d_planes4, n, c.m, c.bound, flt, off, cap, out);
    });
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return ptk_list_sort(off, n, cap, out, false, c.stream);
}

// ---- entry points (include/pt_api.h): every argument check comes before the first HIP call ----------------------------------------
// outName / outAlign: "count" (4 bytes) or the PtBoxMember records "out" (8)
static int convex_args_ok(const char* who, const PtScene* s, const float* planes, int64_t n, int32_t n_planes, int32_t flags, const char* outName, int outAlign,
                          const void* out, bool list, const int64_t* offsets, int64_t cap, bool device, const PtQueryFilter* filter)
{
    const char* param = (n_planes < 1 || n_planes > PT_CONVEX_MAX_PLANES) ? "n_planes outside 1 .. 8"
                        : (flags != PT_CONVEX_TOUCHING && flags != PT_CONVEX_INSIDE) ? "unknown flags" : nullptr;
    return pt_query_args(who, s, n, device, {"planes", planes, outName, out, outName, outAlign, "detail", nullptr, param, list, offsets, cap, filter, false});
}

static ConvexCall convex_call(const PtScene* s, int32_t n_planes, int32_t flags, const PtQueryFilter* filter, void* hip_stream)
{
    return ConvexCall{pt_query_walks_quad(s), !pt_filter_neutral(filter), n_planes, flags == PT_CONVEX_INSIDE ? 0.f : 1.f, (hipStream_t)hip_stream};
}

// d = n . pos and the plane (n | d) of a side of the frustum, rounded once to float32: n = cross(u, v) oriented so that `inside` is in
static void side_plane(const double* pos, const double* u, const double* v, const double* inside, float* out)
{
    double n[3] = {u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]};
    if (n[0] * inside[0] + n[1] * inside[1] + n[2] * inside[2] > 0.0) { n[0] = -n[0]; n[1] = -n[1]; n[2] = -n[2]; }
    for (int k = 0; k < 3; k++) out[k] = (float)(n[k] + 0.0);      // + 0.0: no -0 in a normal, so that a shared side is the same bits up to sign
    out[3] = (float)(n[0] * pos[0] + n[1] * pos[1] + n[2] * pos[2]);
}

extern "C" {

int pt_convex_count(PtScene* s, const float* d_planes4, int64_t n, int32_t n_planes, int32_t flags, const PtQueryFilter* filter, int32_t* d_count,
                    void* hip_stream)
{
    int rc;
    if ((rc = convex_args_ok("pt_convex_count", s, d_planes4, n, n_planes, flags, "count", 4, d_count, false, nullptr, 0, true, filter)) != PT_OK) return rc;
    if (n == 0) return PT_OK;
    HIPCHK(hipSetDevice(s->device));
    const ConvexCall c = convex_call(s, n_planes, flags, filter, hip_stream);
    HIPCHK(pt_query_batches(n, [&](int64_t off, uint32_t m) {
        return launch_convex_count(s->dev, d_planes4 + off * 4 * n_planes, m, c, pt_filter_dev(c.flt ? filter : nullptr, off), d_count + off);
    }));
    return PT_OK;
}

int pt_convex_any(PtScene* s, const float* d_planes4, int64_t n, int32_t n_planes, int32_t flags, const PtQueryFilter* filter, PtBoxMember* d_out,
                  void* hip_stream)
{
    int rc;
    if ((rc = convex_args_ok("pt_convex_any", s, d_planes4, n, n_planes, flags, "out", 8, d_out, false, nullptr, 0, true, filter)) != PT_OK) return rc;
    if (n == 0) return PT_OK;
    HIPCHK(hipSetDevice(s->device));
    const ConvexCall c = convex_call(s, n_planes, flags, filter, hip_stream);
    HIPCHK(pt_query_batches(n, [&](int64_t off, uint32_t m) {
        return launch_convex_any(s->dev, d_planes4 + off * 4 * n_planes, m, c, pt_filter_dev(c.flt ? filter : nullptr, off), d_out + off);
    }));
    return PT_OK;
}

int pt_convex_list(PtScene* s, const float* d_planes4, int64_t n, int32_t n_planes, int32_t flags, const int64_t* d_offsets, int64_t cap,
                   const PtQueryFilter* filter, PtBoxMember* d_out, void* hip_stream)
{
    int rc;
    if ((rc = convex_args_ok("pt_convex_list", s, d_planes4, n, n_planes, flags, "out", 8, d_out, true, d_offsets, cap, true, filter)) != PT_OK) return rc;
    if (n == 0) return PT_OK;
    HIPCHK(hipSetDevice(s->device));
    const ConvexCall c = convex_call(s, n_planes, flags, filter, hip_stream);
    HIPCHK(pt_query_batches(n, [&](int64_t off, uint32_t m) {
        return launch_convex_list(s->dev, d_planes4 + off * 4 * n_planes, m, c, pt_filter_dev(c.flt ? filter : nullptr, off), d_offsets + off, cap, d_out);
    }));
    return PT_OK;
}

int pt_convex_count_host(PtScene* s, const float* h_planes4, int64_t n, int32_t n_planes, int32_t flags, int32_t* h_count)
{
    int rc;
    if ((rc = convex_args_ok("pt_convex_count_host", s, h_planes4, n, n_planes, flags, "count", 4, h_count, false, nullptr, 0, false, nullptr)) != PT_OK) return rc;
    if (n == 0) return PT_OK;
    HIPCHK(hipSetDevice(s->device));
    return pt_host_query(h_planes4, (size_t)n * 16 * n_planes, h_count, (size_t)n * 4, nullptr, 0, [&](float* d_planes, void* d_count, float*) {
        return pt_convex_count(s, d_planes, n, n_planes, flags, nullptr, (int32_t*)d_count, nullptr);
    });
}

int pt_convex_any_host(PtScene* s, const float* h_planes4, int64_t n, int32_t n_planes, int32_t flags, PtBoxMember* h_out)
{
    int rc;
    if ((rc = convex_args_ok("pt_convex_any_host", s, h_planes4, n, n_planes, flags, "out", 8, h_out, false, nullptr, 0, false, nullptr)) != PT_OK) return rc;
    if (n == 0) return PT_OK;
    HIPCHK(hipSetDevice(s->device));
    return pt_host_query(h_planes4, (size_t)n * 16 * n_planes, h_out, (size_t)n * 8, nullptr, 0, [&](float* d_planes, void* d_out, float*) {
        return pt_convex_any(s, d_planes, n, n_planes, flags, nullptr, (PtBoxMember*)d_out, nullptr);
    });
}

int pt_convex_list_host(PtScene* s, const float* h_planes4, int64_t n, int32_t n_planes, int32_t flags, int64_t* h_offsets, int64_t cap, PtBoxMember* h_out)
{
    int rc;
    if ((rc = convex_args_ok("pt_convex_list_host", s, h_planes4, n, n_planes, flags, "out", 8, h_out, true, h_offsets, cap, false, nullptr)) != PT_OK) return rc;
    if (n == 0) { h_offsets[0] = 0; return PT_OK; }
    HIPCHK(hipSetDevice(s->device));
    return pt_host_list("pt_convex_list_host", h_planes4, n, (size_t)16 * n_planes, h_offsets, cap, h_out, nullptr, 0,
                        [&](float* d_planes, int32_t* d_count) { return pt_convex_count(s, d_planes, n, n_planes, flags, nullptr, d_count, nullptr); },
                        [&](float* d_planes, int64_t* d_off, int64_t total, void* d_out, float*) {
                            return pt_convex_list(s, d_planes, n, n_planes, flags, d_off, total, nullptr, (PtBoxMember*)d_out, nullptr);
                        });
}

// Host only, no HIP call.  float64 from the camera's float32 fields (tx, ty: the float32 tangents pt_fill_camera gives the device),
// rounded once.  A side with near < 0, or far = +inf, is the neutral plane (0, 0, 0, +inf).
int pt_camera_frustum(const PtCamera* cam, float x0, float y0, float x1, float y1, float near_dist, float far_dist, float* planes24)
{
    const auto fail = [](const char* what) { pt_set_error("pt_camera_frustum: %s", what); return PT_ERR_INVALID; };
    if (!cam) return fail("NULL camera");
    if (!planes24) return fail("NULL planes");
    if (cam->W < 2 || cam->H < 2) return fail("a frame smaller than 2 x 2");
    if (!(0.f <= x0 && x0 < x1 && x1 <= (float)cam->W && 0.f <= y0 && y0 < y1 && y1 <= (float)cam->H)) return fail("the window must have 0 <= x0 < x1 <= W and 0 <= y0 < y1 <= H");
    if (far_dist != far_dist || near_dist != near_dist || (near_dist >= 0.f && !(near_dist <= far_dist))) return fail("near and far must not be NaN, and near <= far");
    for (int k = 0; k < 3; k++)
        if (!std::isfinite(cam->pos[k]) || !std::isfinite(cam->forward[k]) || !std::isfinite(cam->up[k]) || !std::isfinite(cam->right[k]))
            return fail("a camera vector that is not finite");
    if (!std::isfinite(cam->fovy_deg) || !std::isfinite(cam->aspect)) return fail("a camera angle that is not finite");
    ptd::DevCamera c;
    pt_fill_camera(cam, c);
    const double tx = c.tan_half_fovx, ty = c.tan_half_fovy;
    if (!(std::isfinite(tx) && std::isfinite(ty) && tx > 0.0 && ty > 0.0)) return fail("a field of view without a positive finite tangent");
    const double pos[3] = {cam->pos[0], cam->pos[1], cam->pos[2]};
    const double F[3] = {cam->forward[0], cam->forward[1], cam->forward[2]};
    const double flen = std::sqrt(F[0] * F[0] + F[1] * F[1] + F[2] * F[2]);
    if (!(flen > 0.0)) return fail("a zero forward vector");
    // the direction at screen position (fx, fy), as pixel_direction forms it (csrc/pt_shade.h), unnormalised
    const auto dir = [&](double fx, double fy, double* o) {
        const double a = 2.0 * (fx / (double)(cam->W - 1) - 0.5) * tx, b = -2.0 * (fy / (double)(cam->H - 1) - 0.5) * ty;
        for (int k = 0; k < 3; k++) o[k] = F[k] + a * (double)cam->right[k] + b * (double)cam->up[k];
    };
    double c00[3], c10[3], c01[3], c11[3], mid[3];
    dir(x0, y0, c00);
    dir(x1, y0, c10);
    dir(x0, y1, c01);
    dir(x1, y1, c11);
    dir(0.5 * ((double)x0 + x1), 0.5 * ((double)y0 + y1), mid);
    side_plane(pos, c00, c01, mid, planes24 + 0);       // left:   x = x0
    side_plane(pos, c10, c11, mid, planes24 + 4);       // right:  x = x1
    side_plane(pos, c00, c10, mid, planes24 + 8);       // top:    y = y0
    side_plane(pos, c01, c11, mid, planes24 + 12);      // bottom: y = y1
    for (int k = 0; k < 4; k++) {
        const float* p = planes24 + 4 * k;
        if (!(p[0] != 0.f || p[1] != 0.f || p[2] != 0.f)) return fail("a degenerate camera: a side plane has no normal");
    }
    const double fp = (F[0] * pos[0] + F[1] * pos[1] + F[2] * pos[2]) / flen;
    const float kInf = __builtin_inff();
    float* nr = planes24 + 16;
    float* fr = planes24 + 20;
    if (near_dist < 0.f) { nr[0] = nr[1] = nr[2] = 0.f; nr[3] = kInf; }
    else { for (int k = 0; k < 3; k++) nr[k] = (float)(-F[k] / flen + 0.0); nr[3] = (float)(-(fp + (double)near_dist)); }
    if (far_dist == kInf) { fr[0] = fr[1] = fr[2] = 0.f; fr[3] = kInf; }
    else { for (int k = 0; k < 3; k++) fr[k] = (float)(F[k] / flen + 0.0); fr[3] = (float)(fp + (double)far_dist); }
    return PT_OK;
}

}  // extern "C"
