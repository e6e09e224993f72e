// pt_dynamic.h — argument block of the vertex update (csrc/pt_dynamic.hip), shared with the host side (csrc/pt_api.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ptd {

constexpr int kCoreBlocks = 256;         // partial boxes of the core-box reduction (one per workgroup)

// Device pointers of one scene: the arrays a render reads (rewritten by an update), the maps of the build (host/accel_build.h,
// read only) and the update's scratch.  "Builder node" = node of the binary traversal tree in the builder's numbering, 0 = root.
struct DynScene {
    // rewritten
    float4* nodes; uint4* quad; float4* tri; float4* tripair; float4* leafbox; float4* surf; float4* lights; float* core;
    // maps
    const int4* bn;              // per builder node: l, r, first, count (count > 0: leaf over tree-order triangles first .. first + count)
    const int32_t* order;        // builder nodes sorted by height
    const int2* wide_bn;         // per `nodes` record: builder node of its L / R box
    const int4* quad_bn;         // per `quad` record: builder node of each child, -1 = none
    const int2* leaf_range;      // per reference leaf: first triangle (reference order), count
    const int2* tmap;            // per tree-order triangle: prim (reference order), reference leaf
    const int32_t* light_prim;   // per light: prim
    const uint8_t* small;        // per prim: 1 = classified small at upload (core box), nullptr when the scene has no core box
    // scratch
    float4* bbox;                // per builder node: unpadded box, mn.xyz 0 | mx.xyz 0
    float* maxabs;               // largest |coordinate| of the root box
    float* core_partial;         // kCoreBlocks x 8 floats
    double* area_partial;        // one block sum per kAreaBlock builder nodes
    int32_t n_bn, n_wide, n_quad, n_tris, n_leaves, n_lights;
};

}  // namespace ptd

extern "C" {
// Enqueues the whole update on `stream`.  level_start: host array of n_levels + 1 offsets into `order` (height h = one launch).
hipError_t ptk_dyn_update(const ptd::DynScene* sc, const float* d_pos, const float* d_frames, const int32_t* level_start, int n_levels,
                          hipStream_t stream);
// Enqueues the area reduction over bbox into area_partial ((n_bn + 1023) / 1024 doubles).
hipError_t ptk_dyn_area(const ptd::DynScene* sc, hipStream_t stream);
}
