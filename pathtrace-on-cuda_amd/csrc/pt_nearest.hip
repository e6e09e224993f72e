// pt_nearest.hip — closest-point queries on an uploaded scene (include/pt_api.h: pt_closest_points): for the caller's points, the primitive
// nearest to each (or any primitive within the radius), on the caller's stream, nothing but (dist2, prim) per point written.
// DESIGN.md section 29.
//
// The result is DEFINED without a tree: the minimum over all primitives of the float32 function f of the header (tri_f, sphere_f in pt_nearest.h),
// largest index among equals.  The walk only has to find it, and what lets it prune is one inequality that holds exactly in float32:
// f(p, k) >= boxdist2(p, box of k) by construction (f's last operation is the max with it), and boxdist2 is monotone in the box
// under rounding, so a child whose (widened) box contains the boxes of the triangles below it and whose boxdist2 exceeds the best f
// so far holds nothing that could win or tie.  No slack factor on the distances; the slack is on the boxes (widen_*), where one rounded
// addition of the 4-wide decode and the record's a + ab against the V1 the boxes were built from can each cost an ulp.
//
// Shape: query_rays' (pt_query.hip) — one point per lane, one-wave workgroups, a per-lane LDS stack with entry k at stack[k * 64].
// An entry is (bound, ref): a popped entry whose bound exceeds the best by now is dropped without fetching its node, which is what a
// distance walk lives on (most entries are pushed before the first leaf has set `best`).  8 bytes x kQueryStack x 64 lanes = 20 KB per
// workgroup: 8 workgroups per CU, 2 waves per SIMD.
#include <hip/hip_runtime.h>
#include "pt_device.h"
#include "pt_math.h"
#include "pt_trace.h"
#include "pt_scene.h"
#include "pt_nearest.h"
#include "pt_lists.h"

namespace ptd {

constexpr int kNearestWaves = 2;      // waves per SIMD the 4-wide walk's LDS stacks allow: 160 KB / 20 KB = 8 one-wave workgroups per CU (the binary walk's 16 KB would allow 3; it shares the bound)

// The tie rule of the ray queries: a smaller f wins, among equal f the larger primitive index; best starts at r2 with prim = -1, so the
// first candidate needs f <= r2.  A NaN f never wins.
PT_DEV void near_take(float f, int prim, float& best, int& bestPrim)
{
    if ((f < best) | ((f == best) & (prim > bestPrim))) { best = f; bestPrim = prim; }
}

// The `cnt` triangles at tree position `first` (a leaf of either tree: ~ref = first << 3 | cnt)
PT_DEV void near_leaf(const DevScene& sc, int ref, const f3& p, float& best, int& bestPrim)
{
    const int code = ~ref, first = code >> 3, cnt = code & 7;
    for (int k = 0; k < cnt; k++) {
        const float4* rec = sc.tri + 3 * (size_t)(first + k);
        const float4 a = rec[0], b = rec[1], c = rec[2];
        near_take(tri_f(p, f3(a.x, a.y, a.z), f3(b.x, b.y, b.z), f3(c.x, c.y, c.z)), __float_as_int(a.w), best, bestPrim);
    }
}

// The walk over the 4-wide quantised tree.  A node pushes at most three of its children and descends into the fourth, a leaf pushes
// nothing: the stack never exceeds 3 entries per level (the caller has checked 3 * quad_depth + 2 <= kQueryStack), and the walk ends
// whatever the floats are, as quad_step's does.
template <bool ANY>
PT_DEV void near_walk_quad(const DevScene& sc, const f3& p, int2* stack, float& best, int& bestPrim)
{
    int cur = 0, sp = 0;
    for (;;) {
        if (cur >= 0) {
            const uint4* np = sc.quad + 4 * (size_t)cur;
            const uint4 n0 = np[0], n1 = np[1], n2 = np[2], n3 = np[3];
            const int ref[4] = {(int)n1.x, (int)n1.y, (int)n1.z, (int)n1.w};
            int key[4];
#pragma unroll
            for (int k = 0; k < 4; k++) {
                f3 lo, hi;
                near_quad_child_box(n0, n2, n3, k, lo, hi);
                const float lb = boxdist2(p, lo, hi);
                key[k] = ((ref[k] == -1) | (lb > best)) ? kQuadMiss : __float_as_int(lb);      // an empty slot's box is inverted, not far away
            }
            int k0 = key[0], k1 = key[1], k2 = key[2], k3 = key[3], r0 = ref[0], r1 = ref[1], r2 = ref[2], r3 = ref[3];
#define PT_CE(ka, ra, kb, rb) { const bool sw = ka > kb; const int tk = sw ? kb : ka, tr = sw ? rb : ra; kb = sw ? ka : kb; rb = sw ? ra : rb; ka = tk; ra = tr; }
            PT_CE(k0, r0, k1, r1) PT_CE(k2, r2, k3, r3) PT_CE(k0, r0, k2, r2) PT_CE(k1, r1, k3, r3) PT_CE(k1, r1, k2, r2)
#undef PT_CE
            if (k0 != kQuadMiss) {      // the nearest child is next, the others wait, farthest first
                if (k3 != kQuadMiss) { stack[sp * 64] = make_int2(k3, r3); sp++; }
                if (k2 != kQuadMiss) { stack[sp * 64] = make_int2(k2, r2); sp++; }
                if (k1 != kQuadMiss) { stack[sp * 64] = make_int2(k1, r1); sp++; }
                cur = r0;
                continue;
            }
        } else {
            near_leaf(sc, cur, p, best, bestPrim);
            if (ANY && bestPrim >= 0) return;
        }
        if (!near_pop(stack, sp, best, cur)) return;
    }
}

// The walk over the binary tree, for a scene whose 4-wide walk would not fit kQueryStack (or PTAMD_QUERY_QUAD=0).  As in trace_closest a
// leaf child is evaluated on the spot and an entry is pushed only where both children are interior: at most depth - 1 <= 31 entries.
template <bool ANY>
PT_DEV void near_walk_binary(const DevScene& sc, const f3& p, int2* stack, float& best, int& bestPrim)
{
    int cur = 0, sp = 0;
    for (;;) {
        const float4 q0 = sc.nodes[4 * (size_t)cur + 0], q1 = sc.nodes[4 * (size_t)cur + 1], q2 = sc.nodes[4 * (size_t)cur + 2], q3 = sc.nodes[4 * (size_t)cur + 3];
        f3 loL(q0.x, q0.y, q0.z), hiL(q0.w, q1.x, q1.y), loR(q1.z, q1.w, q2.x), hiR(q2.y, q2.z, q2.w);
        widen_binary(loL, hiL);
        widen_binary(loR, hiR);
        const float lbL = boxdist2(p, loL, hiL), lbR = boxdist2(p, loR, hiR);
        const int refL = __float_as_int(q3.x), refR = __float_as_int(q3.y);
        if (refL < 0 && !(lbL > best)) {
            near_leaf(sc, refL, p, best, bestPrim);
            if (ANY && bestPrim >= 0) return;
        }
        if (refR < 0 && !(lbR > best)) {
            near_leaf(sc, refR, p, best, bestPrim);
            if (ANY && bestPrim >= 0) return;
        }
        const bool okL = (refL >= 0) & !(lbL > best), okR = (refR >= 0) & !(lbR > best);      // against what the leaves left
        if (okL & okR) {
            const bool lNear = lbL <= lbR;
            stack[sp * 64] = lNear ? make_int2(__float_as_int(lbR), refR) : make_int2(__float_as_int(lbL), refL);
            sp++;
            cur = lNear ? refL : refR;
        } else if (okL) {
            cur = refL;
        } else if (okR) {
            cur = refR;
        } else if (!near_pop(stack, sp, best, cur)) {
            return;
        }
    }
}

template <bool ANY, bool QUAD>
__global__ __launch_bounds__(64, kNearestWaves)
void nearest_points(DevScene sc, const float4* __restrict__ points, uint32_t n, float2* __restrict__ out)
{
    __shared__ int2 lds_stack[(QUAD ? kQueryStack : kStackDepth) * 64];
    const uint32_t i = blockIdx.x * 64u + threadIdx.x;
    if (i >= n) return;
    int2* stack = &lds_stack[threadIdx.x];
    const float4 q = points[i];
    const f3 p(q.x, q.y, q.z);
    float best = q.w * q.w;
    int bestPrim = -1;
    if (QUAD) near_walk_quad<ANY>(sc, p, stack, best, bestPrim);
    else near_walk_binary<ANY>(sc, p, stack, best, bestPrim);
    if (!(ANY && bestPrim >= 0)) {
        for (int s = 0; s < sc.n_spheres; s++) {
            near_take(sphere_f(p, sc.spheres[4 * s]), sc.n_tris + s, best, bestPrim);
            if (ANY && bestPrim >= 0) break;
        }
    }
    out[i] = make_float2(bestPrim < 0 ? 0.f : best, __int_as_float(bestPrim));      // a miss is (0, -1)
}

// The 8-float detail record of the header for every finished closest-point result; zeros for a miss.  The winning triangle is read from
// its surface record (indexed by primitive in the reference's order), which starts with V0 E1 E2, the floats its tri record holds.
__global__ __launch_bounds__(256)
void nearest_detail(DevScene sc, const float4* __restrict__ points, uint32_t n, const float2* __restrict__ res, float* __restrict__ out8)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const int prim = __float_as_int(res[i].y);
    float* o = out8 + (size_t)i * 8;
    if (prim < 0) { for (int k = 0; k < 8; k++) o[k] = 0.f; return; }
    near_detail(sc, points[i], prim, o);
}

}  // namespace ptd

// Enqueues one batch of n <= 2^30 points on `stream`: (dist2, prim) per point, then the detail records if asked for
static hipError_t launch_nearest(const ptd::DevScene& sc, const float* d_points4, uint32_t n, int any, int quad, PtNearest* d_out, float* d_detail8, hipStream_t stream)
{
    using namespace ptd;
    const float4* pts = (const float4*)d_points4;
    float2* out = (float2*)d_out;
    const uint32_t blocks = (n + 63u) / 64u;
    if (quad) {
        if (any) hipLaunchKernelGGL((nearest_points<true, true>), dim3(blocks), dim3(64), 0, stream, sc, pts, n, out);
        else hipLaunchKernelGGL((nearest_points<false, true>), dim3(blocks), dim3(64), 0, stream, sc, pts, n, out);
    } else {
        if (any) hipLaunchKernelGGL((nearest_points<true, false>), dim3(blocks), dim3(64), 0, stream, sc, pts, n, out);
        else hipLaunchKernelGGL((nearest_points<false, false>), dim3(blocks), dim3(64), 0, stream, sc, pts, n, out);
    }
    if (d_detail8) hipLaunchKernelGGL(nearest_detail, dim3((n + 255u) / 256u), dim3(256), 0, stream, sc, pts, n, (const float2*)out, d_detail8);
    return hipGetLastError();
}

// ---- entry points (include/pt_api.h): every argument check comes before the first HIP call ----------------------------------------
static int nearest_args_ok(const char* who, const PtScene* s, const float* points, int64_t n, int32_t mode, const PtNearest* out, const float* detail,
                           bool device, const PtQueryFilter* filter = nullptr)
{
    const char* param = (mode != PT_NEAREST_CLOSEST && mode != PT_NEAREST_ANY) ? "mode must be PT_NEAREST_CLOSEST or PT_NEAREST_ANY" :
                        (mode == PT_NEAREST_ANY && detail) ? "an any-within query has no detail record (d_detail8 must be NULL)" : nullptr;
    return pt_query_args(who, s, n, device, {"points", points, "out", out, "out", 8, "detail", detail, param, false, nullptr, 0, filter, false});
}

extern "C" {

int pt_closest_points(PtScene* s, const float* d_points4, int64_t n, int32_t mode, PtNearest* d_out, float* d_detail8, void* hip_stream)
{
    int rc;
    if ((rc = nearest_args_ok("pt_closest_points", s, d_points4, n, mode, d_out, d_detail8, true)) != PT_OK) return rc;
    if (n == 0) return PT_OK;
    HIPCHK(hipSetDevice(s->device));
    const bool quad = pt_query_walks_quad(s);
    HIPCHK(pt_query_batches(n, [&](int64_t off, uint32_t m) {
        return launch_nearest(s->dev, d_points4 + off * 4, m, mode == PT_NEAREST_ANY, quad, d_out + off, d_detail8 ? d_detail8 + off * 8 : nullptr,
                              (hipStream_t)hip_stream);
    }));
    return PT_OK;
}

int pt_closest_points_host(PtScene* s, const float* h_points4, int64_t n, int32_t mode, PtNearest* h_out, float* h_detail8)
{
    int rc;
    if ((rc = nearest_args_ok("pt_closest_points_host", s, h_points4, n, mode, h_out, h_detail8, false)) != PT_OK) return rc;
    if (n == 0) return PT_OK;
    HIPCHK(hipSetDevice(s->device));
    return pt_host_query(h_points4, (size_t)n * 16, h_out, (size_t)n * 8, h_detail8, (size_t)n * 32, [&](float* d_pts, void* d_out, float* d_det) {
        return pt_closest_points(s, d_pts, n, mode, (PtNearest*)d_out, d_det, nullptr);
    });
}

// The filtered form (section "Query filters"): the twin's checks, then the filter's; a neutral filter enqueues the twin itself.  Else
// the shared point walk (pt_knearest.hip) over the one-slot sink writes the records, and the detail records come from nearest_detail.
int pt_closest_points_f(PtScene* s, const float* d_points4, int64_t n, int32_t mode, const PtQueryFilter* filter, PtNearest* d_out, float* d_detail8,
                        void* hip_stream)
{
    int rc;
    if ((rc = nearest_args_ok("pt_closest_points_f", s, d_points4, n, mode, d_out, d_detail8, true, filter)) != PT_OK) return rc;
    if (n == 0) return PT_OK;
    if (pt_filter_neutral(filter)) return pt_closest_points(s, d_points4, n, mode, d_out, d_detail8, hip_stream);
    HIPCHK(hipSetDevice(s->device));
    const bool quad = pt_query_walks_quad(s);
    hipStream_t stream = (hipStream_t)hip_stream;
    HIPCHK(pt_query_batches(n, [&](int64_t off, uint32_t m) {
        const float* pts = d_points4 + off * 4;
        const hipError_t e = ptk_near_one_f(s->dev, pts, m, mode == PT_NEAREST_ANY, quad, pt_filter_dev(filter, off), d_out + off, stream);
        if (e != hipSuccess || !d_detail8) return e;
        hipLaunchKernelGGL(ptd::nearest_detail, dim3((m + 255u) / 256u), dim3(256), 0, stream, s->dev, (const float4*)pts, m, (const float2*)(d_out + off),
                           d_detail8 + off * 8);
        return hipGetLastError();
    }));
    return PT_OK;
}

}  // extern "C"
