// accel_build.h — device acceleration structure built at upload (see accel_build.cpp).
#pragma once
#include <cstdint>
#include <vector>
#include "../../include/pt_api.h"

constexpr int kQuadTopBfs = 1024;       // leading quad nodes numbered breadth-first (wf_trace stages a prefix of them in LDS)
constexpr int kAccelMaxDepth = 32;       // == ptd::kStackDepth; the builder never exceeds it
constexpr int kQuadDepthCap = 12;        // deepest 4-wide level the size-aware collapse aims for: wf_drain walks the 4-wide tree only while
                                         // 3 * quad_depth + 2 fits its 40-entry stack (csrc/pt_wavefront.hip: kDrainQuadStack)

struct PtAccel {
    std::vector<float> wide;             // n_wide x 16 floats (two child boxes + two refs)
    std::vector<float> tri;              // n_tris x 12 floats, tree order: (V0,prim) (E1,refLeaf) (E2,0)
    std::vector<float> tripair;          // n_tris x 32 floats: record q = triangles q and q+1 (the last: q twice) interleaved for wf_trace's 2-wide test + their two reference leaf boxes (csrc/pt_device.h)
    std::vector<float> leafbox;          // n_leaves x 8 floats: the reference's leaf boxes, verbatim
    std::vector<uint32_t> quad;          // n_quad x 16 dwords: the 4-wide quantised tree (layout: csrc/pt_device.h)
    int n_wide = 0, n_leaves = 0, depth = 0;
    int n_quad = 0, quad_depth = 0;
    // ---- maps of the build, for a refit of the arrays above from new vertex positions (csrc/pt_dynamic.hip) ----
    // The five arrays above do not depend on them.  A "builder node" is a node of the binary traversal tree in the builder's
    // depth-first numbering (0 = root, a child's index is above its parent's).  That order of the indices is used by host code only
    // (accel_build.cpp: the height passes; tests/dynamic_ref.py: refit_nodes on the REFERENCE tree): no dyn_* kernel relies on it — they go
    // through `order` / `level_start` (dyn_refit_level), or visit every node on its own (dyn_nodes, dyn_quad, dyn_area) — and the maps
    // a GPU rebuild writes (csrc/pt_rebuild.hip) number a node by its rank in the radix tree, the root at 0, children in no such order.
    std::vector<int32_t> bn;             // n_bn x 4: l, r, first, count — count > 0: a leaf over tri[first .. first + count), else its two children
    std::vector<int32_t> order;          // n_bn builder nodes sorted by height (0 = leaf), ascending index within a height
    std::vector<int32_t> level_start;    // heights + 2 offsets into `order`: height h is order[level_start[h] .. level_start[h + 1])
    std::vector<int32_t> wide_bn;        // n_wide x 2: builder node whose box is the L / the R box of each `wide` record
    std::vector<int32_t> quad_bn;        // n_quad x 4: builder node of each child of each `quad` record (after the renumbering), -1 = no child
    std::vector<int32_t> leaf_range;     // n_leaves x 2: first triangle (reference order) and triangle count of each reference leaf
    std::vector<int32_t> tmap;           // n_tris x 2, tree order: prim (index in the reference's order), reference leaf
    double area_sum = 0.0;               // pt_accel_area_sum over the builder's own boxes: the denominator of pt_scene_tree_inflation
};

// Sum of Builder::area (float32) of n boxes (8 floats each: mn.xyz _ mx.xyz _), in float64, in the fixed order the device reduction
// uses (csrc/pt_dynamic.hip: dyn_area): blocks of kAreaBlock boxes; in a block 256 partial sums of 4 consecutive boxes each, folded
// by halving (v[t] += v[t + s], s = 128 .. 1); the block sums added in index order.
constexpr int kAreaBlock = 1024;
double pt_accel_area_sum(const float* boxes8, int n);

void pt_build_accel(const PtBVHNode* ref_nodes, int n_ref_nodes, const PtTriangle* tris, int n_tris, PtAccel& out);
