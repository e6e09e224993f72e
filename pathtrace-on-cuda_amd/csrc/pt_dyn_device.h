// pt_dyn_device.h — the device expressions that the vertex update (pt_dynamic.hip), the material update (pt_material.hip) and the tree
// rebuild (pt_rebuild.hip) share: a triangle's nine position floats, its edges and its light record, and the selections and the area
// of a box.  They are the host's own expressions (host/bvh_build.cpp: flatten_tri; host/accel_build.cpp) and are stated once, so that a
// light record or an area comes out with the same bits whichever file computes it.
#pragma once
#include <hip/hip_runtime.h>

namespace ptd {

// Selections are written as comparisons, not fminf, so that the sign of a zero comes out as on the host.
__device__ __forceinline__ float min2(float x, float y) { return (y < x) ? y : x; }      // glm::min / std::min
__device__ __forceinline__ float max2(float x, float y) { return (x < y) ? y : x; }      // glm::max / std::max
// surface area of a box with sides d0 d1 d2 (host/accel_build.cpp: Builder::area)
__device__ __forceinline__ float box_area(float d0, float d1, float d2) { return 2.f * (d0 * d1 + d1 * d2 + d2 * d0); }

struct Tri9 { float v0[3], v1[3], v2[3]; };
struct Edges { float e1[3], e2[3]; };

__device__ __forceinline__ Tri9 load_tri(const float* __restrict__ pos, int prim)
{
    const float* p = pos + (size_t)prim * 9;
    Tri9 t;
    for (int k = 0; k < 3; k++) { t.v0[k] = p[k]; t.v1[k] = p[3 + k]; t.v2[k] = p[6 + k]; }
    return t;
}
__device__ __forceinline__ Edges edges_of(const Tri9& t)
{
    Edges e;
    for (int k = 0; k < 3; k++) { e.e1[k] = t.v1[k] - t.v0[k]; e.e2[k] = t.v2[k] - t.v0[k]; }
    return e;
}

// the 64-byte light record of triangle t: V0 V1 V2 normal area 0 0 0
__device__ __forceinline__ void write_light(float4* r, const Tri9& t)
{
    const Edges e = edges_of(t);
    // bvh_build.cpp: flatten_tri (the reference's component forms, CudaVector.cuh:109-113)
    const float cx = e.e1[1] * e.e2[2] - e.e1[2] * e.e2[1];
    const float cy = -(e.e1[0] * e.e2[2] - e.e1[2] * e.e2[0]);
    const float cz = e.e1[0] * e.e2[1] - e.e1[1] * e.e2[0];
    const float len = sqrtf(cx * cx + cy * cy + cz * cz);
    r[0] = make_float4(t.v0[0], t.v0[1], t.v0[2], t.v1[0]);
    r[1] = make_float4(t.v1[1], t.v1[2], t.v2[0], t.v2[1]);
    r[2] = make_float4(t.v2[2], cx / len, cy / len, cz / len);
    r[3] = make_float4(len * 0.5f, 0.f, 0.f, 0.f);
}

}  // namespace ptd
