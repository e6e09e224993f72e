// pt_sweep.hip — sphere casts on an uploaded scene (include/pt_api.h: pt_sweep_spheres): how far a sphere of the caller's can travel along
// its segment before it touches the scene, and what it touches, on the caller's stream, nothing but (t, prim) per sweep written (and
// the contact's detail record if asked for).  DESIGN.md section 43.
//
// The result is DEFINED without a tree: the minimum over all primitives of the float32 first-contact parameter tau of the header
// (sweep_tri_key, sweep_sphere_key in pt_sweep.h), largest index among equals.  The walk only has to find it; pt_sweep.h says why its
// cull never disagrees with the definition.
//
// Shape: pt_nearest.hip's closest kernel — one sweep per lane, one-wave workgroups, a per-lane LDS stack of int2 (key bits, ref) with
// entry e at stack[e * 64], the nearest child first.  A lane keeps its record, inv = 1 / d and r2 in 12 registers.  8 bytes x
// kQueryStack x 64 lanes = 20 KB per workgroup on the 4-wide tree (16 KB on the binary one): 8 workgroups per CU, 2 waves per SIMD,
// which is what kSweepWaves lets the register allocation assume.  The sinks are pt_lists.h's one-slot sink, closest and any, with
// Filtered around each (FLT).
#include <hip/hip_runtime.h>
#include "pt_device.h"
#include "pt_math.h"
#include "pt_trace.h"
#include "pt_scene.h"
#include "pt_sweep.h"
#include "pt_lists.h"

namespace ptd {

constexpr int kSweepWaves = 2;      // waves per SIMD the 4-wide walk's LDS stacks allow: 160 KB / 20 KB = 8 one-wave workgroups per CU

// The one-slot sink of sweep i with or without its filter around it
template <bool ANY, bool FLT>
PT_DEV auto sweep_sink(float tmax, const QFilter& flt, uint32_t i)
{
    if constexpr (FLT) return Filtered<SlotOne<ANY>>{{tmax, -1, 0.f, -1}, lane_filter(flt, i, 0.f)};
    else return SlotOne<ANY>{tmax, -1, 0.f, -1};
}

template <bool ANY, bool QUAD, bool FLT>
__global__ __launch_bounds__(64, kSweepWaves)
void sweep_spheres(DevScene sc, const float4* __restrict__ sweeps, uint32_t n, QFilter flt, float2* __restrict__ out)
{
    __shared__ int2 lds_stack[(QUAD ? kQueryStack : kStackDepth) * 64];
    const uint32_t i = blockIdx.x * 64u + threadIdx.x;
    if (i >= n) return;
    const SweepLane q = sweep_lane(sweeps[2 * (size_t)i], sweeps[2 * (size_t)i + 1]);
    auto s = sweep_sink<ANY, FLT>(q.tmax, flt, i);
    sweep_query<QUAD>(sc, q, &lds_stack[threadIdx.x], s);
    out[i] = make_float2(s.key, __int_as_float(s.prim));      // a miss is (0, -1)
}

// The 8-float detail record of the closest-point section for every finished closest sweep, at the sphere's centre at contact,
// o + t * d (one multiply and one add per axis), for the winning primitive; zeros for a miss
__global__ __launch_bounds__(256)
void sweep_detail(DevScene sc, const float4* __restrict__ sweeps, uint32_t n, const float2* __restrict__ res, float* __restrict__ out8)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const float2 h = res[i];
    const int prim = __float_as_int(h.y);
    float* o = out8 + (size_t)i * 8;
    if (prim < 0) { for (int k = 0; k < 8; k++) o[k] = 0.f; return; }
    const float4 q0 = sweeps[2 * (size_t)i], q1 = sweeps[2 * (size_t)i + 1];
    near_detail(sc, make_float4(q0.x + h.x * q1.x, q0.y + h.x * q1.y, q0.z + h.x * q1.z, 0.f), prim, o);
}

}  // namespace ptd

// Enqueues one batch of n <= 2^30 sweeps on `stream`: (t, prim) per sweep, then the detail records if asked for
static hipError_t launch_sweep(const ptd::DevScene& sc, const float* d_sweeps8, uint32_t n, bool any, bool quad, bool filtered, const ptd::QFilter& flt,
                               PtRayHit* d_hits, float* d_detail8, hipStream_t stream)
{
    using namespace ptd;
    const float4* in = (const float4*)d_sweeps8;
    float2* out = (float2*)d_hits;
    const dim3 blocks((n + 63u) / 64u);
    const auto launch = [&](auto a, auto q, auto f) {
        hipLaunchKernelGGL((sweep_spheres<a.value, q.value, f.value>), blocks, dim3(64), 0, stream, sc, in, n, flt, out);
    };
    const auto by_filter = [&](auto a, auto q) { if (filtered) launch(a, q, std::true_type()); else launch(a, q, std::false_type()); };
    const auto by_walk = [&](auto a) { if (quad) by_filter(a, std::true_type()); else by_filter(a, std::false_type()); };
    if (any) by_walk(std::true_type()); else by_walk(std::false_type());
    if (d_detail8) hipLaunchKernelGGL(sweep_detail, dim3((n + 255u) / 256u), dim3(256), 0, stream, sc, in, n, (const float2*)out, d_detail8);
    return hipGetLastError();
}

// ---- entry points (include/pt_api.h): every argument check comes before the first HIP call ----------------------------------------
static int sweep_args_ok(const char* who, const PtScene* s, const float* sweeps, int64_t n, int32_t mode, const PtRayHit* hits, const float* detail, bool device,
                         const PtQueryFilter* filter)
{
    const char* param = (mode != PT_SWEEP_CLOSEST && mode != PT_SWEEP_ANY) ? "mode must be PT_SWEEP_CLOSEST or PT_SWEEP_ANY" :
                        (mode == PT_SWEEP_ANY && detail) ? "an any-contact sweep has no detail record (d_detail8 must be NULL)" : nullptr;
    return pt_query_args(who, s, n, device, {"sweeps", sweeps, "hits", hits, "hits", 8, "detail", detail, param, false, nullptr, 0, filter, false});
}

extern "C" {

int pt_sweep_spheres(PtScene* s, const float* d_sweeps8, int64_t n, int32_t mode, const PtQueryFilter* filter, PtRayHit* d_hits, float* d_detail8,
                     void* hip_stream)
{
    int rc;
    if ((rc = sweep_args_ok("pt_sweep_spheres", s, d_sweeps8, n, mode, d_hits, d_detail8, true, filter)) != PT_OK) return rc;
    if (n == 0) return PT_OK;
    HIPCHK(hipSetDevice(s->device));
    const bool quad = pt_query_walks_quad(s), filtered = !pt_filter_neutral(filter);
    HIPCHK(pt_query_batches(n, [&](int64_t off, uint32_t m) {
        return launch_sweep(s->dev, d_sweeps8 + off * 8, m, mode == PT_SWEEP_ANY, quad, filtered, pt_filter_dev(filtered ? filter : nullptr, off), d_hits + off,
                            d_detail8 ? d_detail8 + off * 8 : nullptr, (hipStream_t)hip_stream);
    }));
    return PT_OK;
}

int pt_sweep_spheres_host(PtScene* s, const float* h_sweeps8, int64_t n, int32_t mode, PtRayHit* h_hits, float* h_detail8)
{
    int rc;
    if ((rc = sweep_args_ok("pt_sweep_spheres_host", s, h_sweeps8, n, mode, h_hits, h_detail8, false, nullptr)) != PT_OK) return rc;
    if (n == 0) return PT_OK;
    HIPCHK(hipSetDevice(s->device));
    return pt_host_query(h_sweeps8, (size_t)n * 32, h_hits, (size_t)n * 8, h_detail8, (size_t)n * 32, [&](float* d_sweeps, void* d_hits, float* d_det) {
        return pt_sweep_spheres(s, d_sweeps, n, mode, nullptr, (PtRayHit*)d_hits, d_det, nullptr);
    });
}

}  // extern "C"
