// pt_query.hip — ray queries on an uploaded scene (include/pt_api.h: pt_trace_rays): the caller's rays, closest hit or any hit, on the
// caller's stream, nothing but (t, prim) per ray written.  DESIGN.md section 14.
//
// One ray per lane.  The walk is wf_drain's: quad_step (pt_trace.h) over the 4-wide quantised tree with a per-lane stack in LDS, the
// pair-record triangle test, the reference's acceptance and tie rule, then the spheres in order — so (t, prim) of a closest-hit query
// are the bits trace_closest and the reference's RayCast give.  Workgroups are ONE wave (10 KB of stack each): a finished wave frees
// its slot at once, where a 256-thread workgroup would hold four until its slowest wave is done.
//
// Lane i of the grid traces ray i; a wave lasts as long as its longest ray.  A persistent variant whose waves refilled
// finished lanes from a global ray counter, as wf_trace does, was built and measured: 5-21 % faster on incoherent closest-hit sets,
// 2.3-4 x slower on camera rays, slower over all six cases — not kept.
// An any-hit query is the closest-hit walk with quad_step's early-out armed for every hit (stopBelow = +inf).
// The 29-float surface record, when asked for, is a second kernel over the finished hits (query_surface): make_surf's registers
// (12 float4 of surface record, three interpolated frames) never sit in the traversal loop.
#include <hip/hip_runtime.h>
#include "pt_device.h"
#include "pt_math.h"
#include "pt_bxdf.h"
#include "pt_trace.h"
#include "pt_shade.h"
#include "pt_scene.h"
#include "pt_lists.h"

namespace ptd {

// The spheres, in order, against the triangles' result (pt_trace.h: spheres_closest), and the 8-byte record.  An any-hit query that has its
// triangle needs no sphere; one that has none tests them against tmax exactly as the closest-hit query does, and stops at the first.
template <bool ANY>
PT_DEV void finish_ray(const DevScene& sc, const f3& org, const f3& dir, float bestT, int bestPrim, float2* __restrict__ hit)
{
    if (!(ANY && bestPrim >= 0)) spheres_closest<ANY>(sc, org, dir, bestT, bestPrim);
    *hit = make_float2(bestPrim < 0 ? 0.f : bestT, __int_as_float(bestPrim));      // a miss is (0, -1)
}

// QUAD = false: the binary tree with trace_closest, for a scene whose 4-wide walk would not fit kQueryStack (or PTAMD_QUERY_QUAD=0).
// Its closest hit is also a valid answer to an any-hit query.
template <bool ANY, bool QUAD>
__global__ __launch_bounds__(64, kQueryWaves)
void query_rays(DevScene sc, const float4* __restrict__ rays, uint32_t n, float2* __restrict__ hits)
{
    __shared__ int lds_stack[(QUAD ? kQueryStack : kStackDepth) * 64];
    const uint32_t i = blockIdx.x * 64u + threadIdx.x;
    if (i >= n) return;
    int* stack = &lds_stack[threadIdx.x];
    f3 org, dir; float bestT;
    load_ray(rays, i, org, dir, bestT);
    if (QUAD) {
        f3 inv; float cscale; bool degenerate;
        ray_setup(dir, inv, cscale, degenerate);
        const float stopBelow = ANY ? __builtin_inff() : -__builtin_inff();
        int bestPrim = -1, cur = 0, sp = 0;
        while (!quad_step(sc, org, dir, inv, cscale, degenerate, stopBelow, stack, cur, sp, bestT, bestPrim)) {}
        finish_ray<ANY>(sc, org, dir, bestT, bestPrim, &hits[i]);
    } else {
        TraceStats ts{0, 0, 0};
        float t;
        const int prim = trace_closest<false>(sc, org, dir, bestT, stack, t, ts);
        hits[i] = make_float2(prim < 0 ? 0.f : t, __int_as_float(prim));
    }
}

// The HIT record of pt_dbg_raycast (29 floats) for every finished closest hit; zeros for a miss.
__global__ __launch_bounds__(256)
void query_surface(DevScene sc, const float* __restrict__ uv, const float4* __restrict__ rays, uint32_t n, const float2* __restrict__ hits, float* __restrict__ out29)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const float2 h = hits[i];
    const int prim = __float_as_int(h.y);
    float* o = out29 + (size_t)i * 29;
    if (prim < 0) { for (int k = 0; k < 29; k++) o[k] = 0.f; return; }
    f3 org, dir; float tmax;
    load_ray(rays, i, org, dir, tmax);
    const float t = h.x;
    Surf s;
    make_surf(sc, prim, t, org, dir, s);
    o[0] = 1.f; o[1] = t; o[4] = s.fr.front ? 1.f : 0.f;
    hit_uv(sc, uv, prim, org, dir, o[2], o[3]);
    o[5] = s.p.x; o[6] = s.p.y; o[7] = s.p.z;
    o[8] = s.fr.n.x; o[9] = s.fr.n.y; o[10] = s.fr.n.z;
    o[11] = s.fr.t.x; o[12] = s.fr.t.y; o[13] = s.fr.t.z;
    o[14] = s.fr.b.x; o[15] = s.fr.b.y; o[16] = s.fr.b.z;
    o[17] = s.m.emittance.x; o[18] = s.m.emittance.y; o[19] = s.m.emittance.z;
    o[20] = s.m.albedo.x; o[21] = s.m.albedo.y; o[22] = s.m.albedo.z;
    o[23] = s.m.specular.x; o[24] = s.m.specular.y; o[25] = s.m.specular.z;
    o[26] = s.m.opacity; o[27] = s.m.roughness; o[28] = s.m.metallic;
}

}  // namespace ptd

// Enqueues one batch of n < 2^31 rays on `stream`: (t, prim) per ray, then the 29-float surface records if asked for.  quad: walk the
// 4-wide tree (the caller has checked that it fits kQueryStack), else the binary one.
static hipError_t launch_query(const ptd::DevScene& sc, const float* uv, const float* d_rays8, uint32_t n, int any, int quad, PtRayHit* d_hits, float* d_surface29,
                               hipStream_t stream)
{
    using namespace ptd;
    const float4* rays = (const float4*)d_rays8;
    float2* hits = (float2*)d_hits;
    const uint32_t blocks = (n + 63u) / 64u;
    if (quad) {
        if (any) hipLaunchKernelGGL((query_rays<true, true>), dim3(blocks), dim3(64), 0, stream, sc, rays, n, hits);
        else hipLaunchKernelGGL((query_rays<false, true>), dim3(blocks), dim3(64), 0, stream, sc, rays, n, hits);
    } else {
        if (any) hipLaunchKernelGGL((query_rays<true, false>), dim3(blocks), dim3(64), 0, stream, sc, rays, n, hits);
        else hipLaunchKernelGGL((query_rays<false, false>), dim3(blocks), dim3(64), 0, stream, sc, rays, n, hits);
    }
    if (d_surface29) hipLaunchKernelGGL(query_surface, dim3((n + 255u) / 256u), dim3(256), 0, stream, sc, uv, rays, n, (const float2*)hits, d_surface29);
    return hipGetLastError();
}

// ---- entry points (include/pt_api.h): every argument check comes before the first HIP call ----------------------------------------
static int query_args_ok(const char* who, const PtScene* s, const float* rays, int64_t n, int32_t mode, const PtRayHit* hits, const float* surface,
                         bool device, const PtQueryFilter* filter = nullptr)
{
    const char* param = (mode != PT_QUERY_CLOSEST && mode != PT_QUERY_ANY) ? "mode must be PT_QUERY_CLOSEST or PT_QUERY_ANY" :
                        (mode == PT_QUERY_ANY && surface) ? "an any-hit query has no surface record (d_surface29 must be NULL)" : nullptr;
    return pt_query_args(who, s, n, device, {"rays", rays, "hits", hits, "hits", 8, "surface", surface, param, false, nullptr, 0, filter, true});
}

extern "C" {

int pt_trace_rays(PtScene* s, const float* d_rays8, int64_t n, int32_t mode, PtRayHit* d_hits, float* d_surface29, void* hip_stream)
{
    int rc;
    if ((rc = query_args_ok("pt_trace_rays", s, d_rays8, n, mode, d_hits, d_surface29, true)) != PT_OK) return rc;
    if (n == 0) return PT_OK;
    HIPCHK(hipSetDevice(s->device));
    const bool quad = pt_query_walks_quad(s);
    HIPCHK(pt_query_batches(n, [&](int64_t off, uint32_t m) {
        return launch_query(s->dev, s->uv.as<float>(), d_rays8 + off * 8, m, mode == PT_QUERY_ANY, quad, d_hits + off,
                            d_surface29 ? d_surface29 + off * 29 : nullptr, (hipStream_t)hip_stream);
    }));
    return PT_OK;
}

int pt_trace_rays_host(PtScene* s, const float* h_rays8, int64_t n, int32_t mode, PtRayHit* h_hits, float* h_surface29)
{
    int rc;
    if ((rc = query_args_ok("pt_trace_rays_host", s, h_rays8, n, mode, h_hits, h_surface29, false)) != PT_OK) return rc;
    if (n == 0) return PT_OK;
    HIPCHK(hipSetDevice(s->device));
    return pt_host_query(h_rays8, (size_t)n * 32, h_hits, (size_t)n * 8, h_surface29, (size_t)n * 116, [&](float* d_rays, void* d_hits, float* d_surf) {
        return pt_trace_rays(s, d_rays, n, mode, (PtRayHit*)d_hits, d_surf, nullptr);
    });
}

// The filtered form (section "Query filters"): the twin's checks, then the filter's; a neutral filter enqueues the twin itself.  Else
// pt_rayhits.hip's walk over the one-slot sink writes the records, and the surface records come from query_surface as above.
int pt_trace_rays_f(PtScene* s, const float* d_rays8, int64_t n, int32_t mode, const PtQueryFilter* filter, PtRayHit* d_hits, float* d_surface29,
                    void* hip_stream)
{
    int rc;
    if ((rc = query_args_ok("pt_trace_rays_f", s, d_rays8, n, mode, d_hits, d_surface29, true, filter)) != PT_OK) return rc;
    if (n == 0) return PT_OK;
    if (pt_filter_neutral(filter)) return pt_trace_rays(s, d_rays8, n, mode, d_hits, d_surface29, hip_stream);
    HIPCHK(hipSetDevice(s->device));
    const bool quad = pt_query_walks_quad(s);
    hipStream_t stream = (hipStream_t)hip_stream;
    HIPCHK(pt_query_batches(n, [&](int64_t off, uint32_t m) {
        const float* rays = d_rays8 + off * 8;
        const hipError_t e = ptk_rays_one_f(s->dev, rays, m, mode == PT_QUERY_ANY, quad, pt_filter_dev(filter, off), d_hits + off, stream);
        if (e != hipSuccess || !d_surface29) return e;
        hipLaunchKernelGGL(ptd::query_surface, dim3((m + 255u) / 256u), dim3(256), 0, stream, s->dev, s->uv.as<float>(), (const float4*)rays, m,
                           (const float2*)(d_hits + off), d_surface29 + off * 29);
        return hipGetLastError();
    }));
    return PT_OK;
}

}  // extern "C"
