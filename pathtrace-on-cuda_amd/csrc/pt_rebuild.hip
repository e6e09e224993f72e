// pt_rebuild.hip — both traversal trees of an uploaded scene built anew on the GPU from the scene's current positions
// (include/pt_api.h: "Tree rebuild").
//
// The RESULT of a render is defined by the triangles and the reference leaf boxes (host/accel_build.cpp); the traversal trees only
// steer the search, so any conservative tree gives the same frame.  The vertex update (pt_dynamic.hip) already writes every box
// and every triangle record from the positions through the maps of the build, so a rebuild only has to produce a new TOPOLOGY —
// the maps bn, order, level_start, wide_bn, quad_bn, tmap and the child refs of `nodes` and `quad` — and then runs that update.
//
// The topology is a linear BVH (Lauterbach 2009; Karras 2012): every step is a sort, a scan or an independent per-node
// computation, and it is a function of the positions and the triangle -> reference leaf assignment alone:
//   centroid box (two-stage reduction) -> 30-bit Morton code, key = morton << 32 | prim (unique) -> rocPRIM radix sort ->
//   Karras' radix tree over the sorted keys, one thread per internal node -> depth (walk up the parent links, read-only by then)
//   and height (integer atomicMax climbing from the leaves) -> numbering by exclusive scans and stable sorts -> the maps.
// "Raw" node v of the radix tree: v < n - 1 is Karras' internal node v (0 = root), v >= n - 1 is the leaf of sorted triangle
// v - (n - 1).  An internal node over exactly two triangles becomes a LEAF OF TWO and its two raw leaves are dead; every other raw
// leaf is a leaf of one.  Builder node = rank of a live raw node among the live ones, `nodes` record = rank of an interior node
// among the interior ones, `quad` record = rank of an interior node at even depth in the stable sort by depth / 2.  No atomic
// decides an index or an order; the two atomicMax (height, deepest level) are maxima of integers, read by the next kernel only.
//
// Everything is built in buffers of its own and checked against the kernels' stack limits on the host BEFORE the first write to an
// array a render reads: a topology that is too deep leaves the scene exactly as it was.
//
// pt_scene_rebuild_tree_ex is the same build with two opt-in steps: the triangles' size class as bit 62 of
// the key, each class quantised in a centroid box of its own, and a depth budget — every triangle rewrites its key below the
// topmost ancestor that would reach below the budget, and the radix tree is built a second time over the new keys.
// pt_scene_rebuild_tree_opt adds treelet restructuring passes by surface area between that tree and the numbering.
#include <hip/hip_runtime.h>
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <utility>
#include <vector>
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include "pt_scene.h"
#include "pt_dyn_device.h"
#include "../host/accel_build.h"

namespace {

using ptd::DynScene;
using ptd::Tri9;
using ptd::load_tri;

__device__ __forceinline__ float min2(float x, float y) { return (y < x) ? y : x; }      // as pt_dynamic.hip
__device__ __forceinline__ float max2(float x, float y) { return (x < y) ? y : x; }

constexpr int kDead = 127;           // sort key of a raw node that gets no number (heights and levels are below 64: unique keys with at most 63 significant bits)
constexpr int kLevelSlots = 129;     // first index with key >= h, h = 0 .. 128
// the words read back before the commit: level offsets of `order`, level offsets of the 4-wide numbering, deepest builder node
constexpr int kLvOrder = 0, kLvQuad = kLevelSlots, kLvDepth = 2 * kLevelSlots, kLvWords = 2 * kLevelSlots + 2;

// What the build works in (PtScene::rb_buf, in this order).  n = triangles, N = 2 n - 1 raw nodes, I = max(n - 1, 1) internal nodes.
struct RbDev {
    int32_t* prim_leaf;      // n: reference leaf of every prim
    float* box_partial;      // kCoreBlocks x 8
    float* cbox;             // 8: lo.xyz hi.xyz of the centroids
    uint64_t* keys;          // n, unsorted
    uint64_t* sorted;        // n
    int2* child;             // I: raw l, r
    int2* range;             // I: first, last sorted triangle
    int32_t* parent;         // N
    int32_t* depth;          // N
    int32_t* height;         // N
    int32_t* live;           // N: 1 = gets a builder node
    int32_t* newid;          // N: builder node
    int32_t* wflag;          // I: 1 = interior (more than two triangles)
    int32_t* widx;           // I: `nodes` record
    uint32_t* key_in;        // N: sort keys (height, then level)
    uint32_t* key_out;       // N
    int32_t* iota;           // I
    int32_t* qsorted;        // I: raw internal nodes by level
    int32_t* qidx;           // I: `quad` record
    int32_t* levels;         // kLvWords
    // the new maps and refs, staged
    int4* bn; int32_t* order; int2* wide_bn; int4* quad_bn; int2* tmap; int2* node_ref; int4* quad_ref;
    int32_t n;
};

// ---- prim -> reference leaf (once per scene) ------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void rb_prim_leaf(DynScene s, RbDev r)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= s.n_leaves) return;
    const int2 lr = s.leaf_range[i];
    for (int k = 0; k < lr.y; k++) r.prim_leaf[lr.x + k] = i;
}

// ---- centroid box: two stages in the shape of dyn_core_partial / dyn_core_final, no float atomics ------------------------------
__device__ __forceinline__ void centroid(const float* __restrict__ pos, int prim, float* c)
{
    const Tri9 t = load_tri(pos, prim);
    for (int a = 0; a < 3; a++) {
        const float mn = min2(t.v0[a], min2(t.v1[a], t.v2[a]));
        const float mx = max2(t.v0[a], max2(t.v1[a], t.v2[a]));
        c[a] = 0.5f * (mn + mx);
    }
}

__device__ __forceinline__ void block_box(float* v, float (*lds)[6])      // v[0..2] min, v[3..5] max over the block, in lds[0]
{
    for (int k = 0; k < 6; k++) lds[threadIdx.x][k] = v[k];
    __syncthreads();
    for (int st = 128; st > 0; st >>= 1) {
        if ((int)threadIdx.x < st)
            for (int k = 0; k < 6; k++) {
                const float a = lds[threadIdx.x][k], b = lds[threadIdx.x + st][k];
                lds[threadIdx.x][k] = k < 3 ? min2(a, b) : max2(a, b);
            }
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void rb_box_partial(RbDev r, const float* __restrict__ pos)
{
    __shared__ float lds[256][6];
    float v[6] = {FLT_MAX, FLT_MAX, FLT_MAX, -FLT_MAX, -FLT_MAX, -FLT_MAX};
    for (int i = blockIdx.x * 256 + threadIdx.x; i < r.n; i += ptd::kCoreBlocks * 256) {
        float c[3];
        centroid(pos, i, c);
        for (int a = 0; a < 3; a++) { v[a] = min2(v[a], c[a]); v[3 + a] = max2(v[3 + a], c[a]); }
    }
    block_box(v, lds);
    if (threadIdx.x == 0) for (int k = 0; k < 6; k++) r.box_partial[blockIdx.x * 8 + k] = lds[0][k];
}

__global__ __launch_bounds__(256) void rb_box_final(RbDev r)
{
    __shared__ float lds[256][6];
    float v[6];
    for (int k = 0; k < 6; k++) v[k] = r.box_partial[threadIdx.x * 8 + k];      // kCoreBlocks == the block size
    block_box(v, lds);
    if (threadIdx.x == 0) for (int k = 0; k < 6; k++) r.cbox[k] = lds[0][k];
}

// ---- keys: 10 bits per axis, x the most significant of every triple; the prim below makes the key unique -----------------------
__device__ __forceinline__ uint32_t spread3(uint32_t q)      // bit k of q -> bit 3 k
{
    q &= 1023u;
    q = (q | (q << 16)) & 0x030000ffu;
    q = (q | (q << 8)) & 0x0300f00fu;
    q = (q | (q << 4)) & 0x030c30c3u;
    q = (q | (q << 2)) & 0x09249249u;
    return q;
}

__global__ __launch_bounds__(256) void rb_keys(RbDev r, const float* __restrict__ pos)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= r.n) return;
    float c[3];
    centroid(pos, i, c);
    uint32_t q[3];
    for (int a = 0; a < 3; a++) {
        const float lo = r.cbox[a], ext = r.cbox[3 + a] - lo;
        int v = 0;
        if (ext > 0.f) { v = (int)(((c[a] - lo) / ext) * 1024.0f); if (v > 1023) v = 1023; }
        q[a] = (uint32_t)v;
    }
    const uint32_t morton = (spread3(q[0]) << 2) | (spread3(q[1]) << 1) | spread3(q[2]);
    r.keys[i] = ((uint64_t)morton << 32) | (uint32_t)i;
}

__global__ __launch_bounds__(256) void rb_tmap(RbDev r)
{
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= r.n) return;
    const int prim = (int)(uint32_t)r.sorted[q];
    r.tmap[q] = make_int2(prim, r.prim_leaf[prim]);
}

// ---- n <= 2: the single-leaf scene, the maps host/accel_build.cpp produces for it -------------------------------------------------
__global__ void rb_single(RbDev r)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const int leaf = ~r.n;      // ~((0 << 3) | n)
    r.bn[0] = make_int4(-1, -1, 0, r.n);
    r.order[0] = 0;
    r.wide_bn[0] = make_int2(0, 0);
    r.quad_bn[0] = make_int4(0, -1, -1, -1);
    r.node_ref[0] = make_int2(leaf, ~0);
    r.quad_ref[0] = make_int4(leaf, ~0, ~0, ~0);
    for (int h = 0; h < kLevelSlots; h++) { r.levels[kLvOrder + h] = h == 0 ? 0 : 1; r.levels[kLvQuad + h] = h == 0 ? 0 : 1; }
    r.levels[kLvDepth] = 0;
}

// ---- Karras 2012: the radix tree over n >= 3 sorted unique keys, one thread per internal node ------------------------------------
__device__ __forceinline__ int delta(const uint64_t* __restrict__ k, int n, uint64_t ki, int j)
{
    return (j < 0 || j >= n) ? -1 : __clzll((long long)(ki ^ k[j]));
}

__global__ __launch_bounds__(256) void rb_karras(RbDev r)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    const int n = r.n;
    if (i >= n - 1) return;
    const uint64_t* __restrict__ k = r.sorted;
    const uint64_t ki = k[i];
    const int d = delta(k, n, ki, i + 1) > delta(k, n, ki, i - 1) ? 1 : -1;
    const int dmin = delta(k, n, ki, i - d);
    int lmax = 2;
    while (delta(k, n, ki, i + lmax * d) > dmin) lmax <<= 1;
    int l = 0;
    for (int t = lmax >> 1; t >= 1; t >>= 1)
        if (delta(k, n, ki, i + (l + t) * d) > dmin) l += t;
    const int j = i + l * d;
    const int dnode = delta(k, n, ki, j);
    int s = 0, t = l;
    do {
        t = (t + 1) >> 1;
        if (delta(k, n, ki, i + (s + t) * d) > dnode) s += t;
    } while (t > 1);
    const int gamma = i + s * d + (d < 0 ? -1 : 0);
    const int first = i < j ? i : j, last = i < j ? j : i;
    const int left = first == gamma ? (n - 1) + gamma : gamma;
    const int right = last == gamma + 1 ? (n - 1) + gamma + 1 : gamma + 1;
    r.child[i] = make_int2(left, right);
    r.range[i] = make_int2(first, last);
    r.parent[left] = i;
    r.parent[right] = i;
    if (i == 0) r.parent[0] = -1;
}

// ---- depth, liveness, interior flag (the parent links are from the kernel before) ------------------------------------------------
__global__ __launch_bounds__(256) void rb_depth(RbDev r)
{
    const int v = blockIdx.x * 256 + threadIdx.x;
    const int n = r.n, N = 2 * n - 1;
    if (v >= N) return;
    int live = 1, interior = 0;
    if (v >= n - 1) {
        const int2 pr = r.range[r.parent[v]];
        live = pr.y - pr.x == 1 ? 0 : 1;      // under a leaf of two
    } else {
        const int2 rg = r.range[v];
        interior = rg.y - rg.x > 1 ? 1 : 0;
        r.wflag[v] = interior;
        r.iota[v] = v;
    }
    int dep = 0;
    for (int p = r.parent[v]; p >= 0; p = r.parent[p]) dep++;
    r.depth[v] = dep;
    r.height[v] = 0;
    r.live[v] = live;
    if (live && !interior) atomicMax(&r.levels[kLvDepth], dep);      // the deepest node is a leaf
}

// every leaf climbs; it stops where another leaf has already brought at least its own height
__global__ __launch_bounds__(256) void rb_height(RbDev r)
{
    const int v = blockIdx.x * 256 + threadIdx.x;
    const int n = r.n, N = 2 * n - 1;
    if (v >= N || !r.live[v]) return;
    if (v < n - 1 && r.wflag[v]) return;
    int h = 0;
    for (int p = r.parent[v]; p >= 0; p = r.parent[p]) {
        h++;
        if (atomicMax(&r.height[p], h) >= h) break;
    }
}

__global__ __launch_bounds__(256) void rb_height_keys(RbDev r)
{
    const int v = blockIdx.x * 256 + threadIdx.x;
    if (v >= 2 * r.n - 1) return;
    r.key_in[v] = r.live[v] ? (uint32_t)r.height[v] : (uint32_t)kDead;
}

__global__ __launch_bounds__(256) void rb_level_keys(RbDev r)
{
    const int v = blockIdx.x * 256 + threadIdx.x;
    if (v >= r.n - 1) return;
    const int dep = r.depth[v];
    r.key_in[v] = (r.wflag[v] && (dep & 1) == 0) ? (uint32_t)(dep >> 1) : (uint32_t)kDead;
}

// out[h] = first index of the sorted keys with key >= h, h = 0 .. 128 (every slot is written by exactly one thread)
__global__ __launch_bounds__(256) void rb_level_start(const uint32_t* __restrict__ keys, int count, int32_t* __restrict__ out)
{
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= count) return;
    const int k = (int)keys[t], prev = t > 0 ? (int)keys[t - 1] : -1;
    for (int h = prev + 1; h <= k; h++) out[h] = t;
    if (t == count - 1) for (int h = k + 1; h < kLevelSlots; h++) out[h] = count;
}

__global__ __launch_bounds__(256) void rb_qidx(RbDev r)
{
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= r.n - 1) return;
    if (r.key_out[p] != (uint32_t)kDead) r.qidx[r.qsorted[p]] = p;
}

// ---- the maps and the refs, one thread per raw node ---------------------------------------------------------------------------------
__device__ __forceinline__ bool rb_is_interior(const RbDev& r, int c) { return c < r.n - 1 && r.wflag[c]; }
__device__ __forceinline__ int rb_leaf_ref(const RbDev& r, int c)      // pt_device.h: ~((first << 3) | count)
{
    return c >= r.n - 1 ? ~(((c - (r.n - 1)) << 3) | 1) : ~((r.range[c].x << 3) | 2);
}

__global__ __launch_bounds__(256) void rb_emit(RbDev r)
{
    const int v = blockIdx.x * 256 + threadIdx.x;
    const int n = r.n, N = 2 * n - 1;
    if (v >= N || !r.live[v]) return;
    const int id = r.newid[v];
    if (v >= n - 1) { r.bn[id] = make_int4(-1, -1, v - (n - 1), 1); return; }
    if (!r.wflag[v]) { r.bn[id] = make_int4(-1, -1, r.range[v].x, 2); return; }
    const int2 c = r.child[v];
    const int nl = r.newid[c.x], nr = r.newid[c.y];
    r.bn[id] = make_int4(nl, nr, 0, 0);
    const int w = r.widx[v];
    r.wide_bn[w] = make_int2(nl, nr);
    r.node_ref[w] = make_int2(rb_is_interior(r, c.x) ? r.widx[c.x] : rb_leaf_ref(r, c.x), rb_is_interior(r, c.y) ? r.widx[c.y] : rb_leaf_ref(r, c.y));
    if (r.depth[v] & 1) return;
    // the 4-wide node of an interior node at even depth: its grandchildren, or a child itself where the child is a leaf
    int ch[4], nc = 0;
    const int side[2] = {c.x, c.y};
    for (int k = 0; k < 2; k++) {
        if (rb_is_interior(r, side[k])) { const int2 g = r.child[side[k]]; ch[nc++] = g.x; ch[nc++] = g.y; }
        else ch[nc++] = side[k];
    }
    int bnode[4] = {-1, -1, -1, -1}, ref[4] = {~0, ~0, ~0, ~0};
    for (int k = 0; k < nc; k++) {
        bnode[k] = r.newid[ch[k]];
        ref[k] = rb_is_interior(r, ch[k]) ? r.qidx[ch[k]] : rb_leaf_ref(r, ch[k]);
    }
    const int q = r.qidx[v];
    r.quad_bn[q] = make_int4(bnode[0], bnode[1], bnode[2], bnode[3]);
    r.quad_ref[q] = make_int4(ref[0], ref[1], ref[2], ref[3]);
}

// ---- commit: the refs go into the arrays a render reads (the boxes follow from the vertex update's kernels) ------------------------
__global__ __launch_bounds__(256) void rb_refs(DynScene s, RbDev r)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < s.n_wide) {
        const int2 f = r.node_ref[i];
        s.nodes[(size_t)i * 4 + 3] = make_float4(__int_as_float(f.x), __int_as_float(f.y), 0.f, 0.f);
    }
    if (i < s.n_quad) {
        const int4 f = r.quad_ref[i];
        s.quad[(size_t)i * 4 + 1] = make_uint4((uint32_t)f.x, (uint32_t)f.y, (uint32_t)f.z, (uint32_t)f.w);
    }
}

// ---- pt_scene_rebuild_tree_ex: two size classes and a depth budget (include/pt_api.h: "Tree rebuild with a depth budget")
// What only the extended call works in (PtScene::rbx_buf, one block): the partial and the final centroid boxes of the two classes, and
// its own copy of the read-back words with the report's two counts behind them (they travel with wait 1).
constexpr int kRxClassPartial = 0, kRxClassBox = ptd::kCoreBlocks * 16 * 4, kRxLevels = kRxClassBox + 16 * 4;
constexpr int kLvLarge = kLvWords, kLvFlattened = kLvWords + 1, kLvWordsEx = kLvWords + 2;
constexpr int kRxBytes = kRxLevels + kLvWordsEx * 4;

struct RbEx {
    float* class_partial;      // kCoreBlocks x 16: small lo.xyz hi.xyz, pad, large lo.xyz hi.xyz, pad
    float* class_box;          // 16, the same layout
    float large_fraction;
};

// the triangle's centroid and the longest side of its own box
__device__ __forceinline__ float centroid_extent(const float* __restrict__ pos, int prim, float* c)
{
    const Tri9 t = load_tri(pos, prim);
    float ext = 0.f;
    for (int a = 0; a < 3; a++) {
        const float mn = min2(t.v0[a], min2(t.v1[a], t.v2[a]));
        const float mx = max2(t.v0[a], max2(t.v1[a], t.v2[a]));
        c[a] = 0.5f * (mn + mx);
        ext = max2(ext, mx - mn);
    }
    return ext;
}

// f * E, E the longest side of the box of all centroids (rb_box_final has written it)
__device__ __forceinline__ float large_bound(const RbDev& r, float f)
{
    const float E = max2(r.cbox[3] - r.cbox[0], max2(r.cbox[4] - r.cbox[1], r.cbox[5] - r.cbox[2]));
    return f * E;
}

__global__ __launch_bounds__(256) void rb_class_partial(RbDev r, RbEx x, const float* __restrict__ pos)
{
    __shared__ float lds[256][6];
    __shared__ int n_large;
    float v[12] = {FLT_MAX, FLT_MAX, FLT_MAX, -FLT_MAX, -FLT_MAX, -FLT_MAX, FLT_MAX, FLT_MAX, FLT_MAX, -FLT_MAX, -FLT_MAX, -FLT_MAX};
    if (threadIdx.x == 0) n_large = 0;
    const float bound = large_bound(r, x.large_fraction);
    int mine = 0;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < r.n; i += ptd::kCoreBlocks * 256) {
        float c[3];
        const bool large = centroid_extent(pos, i, c) > bound;
        mine += large ? 1 : 0;
        for (int a = 0; a < 3; a++) {
            const float lo_s = large ? v[a] : min2(v[a], c[a]), hi_s = large ? v[3 + a] : max2(v[3 + a], c[a]);
            const float lo_l = large ? min2(v[6 + a], c[a]) : v[6 + a], hi_l = large ? max2(v[9 + a], c[a]) : v[9 + a];
            v[a] = lo_s; v[3 + a] = hi_s; v[6 + a] = lo_l; v[9 + a] = hi_l;
        }
    }
    for (int cls = 0; cls < 2; cls++) {      // after block_box only thread 0 reads lds, and only the row it alone writes
        block_box(v + 6 * cls, lds);
        if (threadIdx.x == 0) for (int k = 0; k < 6; k++) x.class_partial[blockIdx.x * 16 + cls * 8 + k] = lds[0][k];
    }
    if (mine) atomicAdd(&n_large, mine);
    __syncthreads();
    if (threadIdx.x == 0 && n_large) atomicAdd(&r.levels[kLvLarge], n_large);      // a count: it decides no index
}

__global__ __launch_bounds__(256) void rb_class_final(RbEx x)
{
    __shared__ float lds[256][6];
    for (int cls = 0; cls < 2; cls++) {
        float v[6];
        for (int k = 0; k < 6; k++) v[k] = x.class_partial[threadIdx.x * 16 + cls * 8 + k];      // kCoreBlocks == the block size
        block_box(v, lds);
        if (threadIdx.x == 0) for (int k = 0; k < 6; k++) x.class_box[cls * 8 + k] = lds[0][k];
    }
}

// rb_keys with the cell taken in the box of the triangle's own class, and the class above the Morton code
__global__ __launch_bounds__(256) void rb_keys_classes(RbDev r, RbEx x, const float* __restrict__ pos)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= r.n) return;
    float c[3];
    const bool large = centroid_extent(pos, i, c) > large_bound(r, x.large_fraction);
    const float* __restrict__ box = x.class_box + (large ? 8 : 0);
    uint32_t q[3];
    for (int a = 0; a < 3; a++) {
        const float lo = box[a], ext = box[3 + a] - lo;
        int v = 0;
        if (ext > 0.f) { v = (int)(((c[a] - lo) / ext) * 1024.0f); if (v > 1023) v = 1023; }
        q[a] = (uint32_t)v;
    }
    const uint32_t morton = (spread3(q[0]) << 2) | (spread3(q[1]) << 1) | spread3(q[2]);
    r.keys[i] = ((uint64_t)(large ? 1 : 0) << 62) | ((uint64_t)morton << 32) | (uint32_t)i;
}

__device__ __forceinline__ int clog2(int m) { return 32 - __clz(m - 1); }      // bit length of m - 1, m >= 1

// The depth budget: every sorted triangle finds the topmost ancestor v over more than two triangles with depth(v) + clog2(size(v))
// >= budget and, below the bits all of v's keys share, replaces its key by its rank in v.  Reads the first tree (child links are not
// needed: parent, range, depth) and `sorted`; writes `keys`, which nothing reads after the sort.
__global__ __launch_bounds__(256) void rb_rekey(RbDev r, int budget)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    const int n = r.n;
    int changed = 0;
    if (i < n) {
        int top = -1;
        for (int p = r.parent[(n - 1) + i]; p >= 0; p = r.parent[p]) {
            const int2 rg = r.range[p];
            const int size = rg.y - rg.x + 1;
            if (size > 2 && r.depth[p] + clog2(size) >= budget) top = p;
        }
        const uint64_t key = r.sorted[i];
        uint64_t out = key;
        if (top >= 0) {
            const int2 rg = r.range[top];
            const int low = 64 - __clzll((long long)(r.sorted[rg.x] ^ r.sorted[rg.y]));      // 1 .. 63: the keys differ and bit 63 is clear
            out = ((key >> low) << low) | (uint64_t)(i - rg.x);
        }
        r.keys[i] = out;
        changed = out != key ? 1 : 0;
    }
    const int total = __syncthreads_count(changed);
    if (threadIdx.x == 0 && total) atomicAdd(&r.levels[kLvFlattened], total);      // a count: it decides no index
}

// ---- pt_scene_rebuild_tree_opt: treelet restructuring passes over the radix tree (include/pt_api.h: "Tree rebuild with treelet
// restructuring"; Karras and Aila 2013).  A pass runs between the last rb_karras / rb_depth and the numbering and
// rewires `child` / `parent` of interior nodes only: leaves (singletons and internal nodes over two triangles) are never opened, so
// everything below — rb_depth, rb_height, the scans, rb_emit — runs as it is.  Interior nodes are taken in ascending start-of-pass height,
// one launch per height; the nodes of one height are roots of disjoint subtrees and a restructure stays inside its root's subtree, so no
// data passes between workgroups within a launch.
// What only this call works in (PtScene::rbo_buf, one block): its own copy of the read-back words with the report's four counts behind
// them, the level offsets of a pass (device only: they steer the per-height launches), a height and a box per raw node.
constexpr int kTreelet = 7, kOptMaxPasses = 8, kOptPassesDefault = 2;
constexpr int kOptBlock = 64;        // ro_solve: a workgroup is one wave64, two of the 128 subsets per lane
constexpr int kOptGrid = 4096;      // one wave per treelet, grid-stride over the level's slice (its size is known on the device only)
constexpr int kLvRoots = kLvWordsEx, kLvRestructured = kLvWordsEx + 1, kLvWordsOpt = kLvWordsEx + 2;
constexpr size_t kRoLevels = 0, kRoPassLevels = (size_t)kLvWordsOpt * 4, kRoHeights = (kRoPassLevels + (size_t)kLevelSlots * 4 + 15) / 16 * 16;

struct RbOpt {
    float* box;          // N x 6: lo.xyz hi.xyz
    int32_t* hcur;       // N: height now (leaf = 0)
    int32_t* lvl;        // kLevelSlots: first index of `qsorted` with start-of-pass height >= h
    int32_t h_lim;       // budget - 1, or -1: the depth of the tree the pass started from (levels[kLvDepth])
};

__device__ __forceinline__ float box_area(const float* b)      // dyn_area's expression
{
    const float d0 = b[3] - b[0], d1 = b[4] - b[1], d2 = b[5] - b[2];
    return 2.f * (d0 * d1 + d1 * d2 + d2 * d0);
}

__device__ __forceinline__ void tri_box(const float* __restrict__ pos, int prim, float* b)
{
    const Tri9 t = load_tri(pos, prim);
    for (int a = 0; a < 3; a++) {
        b[a] = min2(t.v0[a], min2(t.v1[a], t.v2[a]));
        b[3 + a] = max2(t.v0[a], max2(t.v1[a], t.v2[a]));
    }
}

// boxes and heights of the leaves: singletons, and internal nodes over two triangles (rb_depth has written wflag)
__global__ __launch_bounds__(256) void ro_init(RbDev r, RbOpt o, const float* __restrict__ pos)
{
    const int v = blockIdx.x * 256 + threadIdx.x;
    const int n = r.n, N = 2 * n - 1;
    if (v >= N) return;
    float b[6];
    if (v >= n - 1) {
        tri_box(pos, r.tmap[v - (n - 1)].x, b);
    } else {
        if (r.wflag[v]) return;
        const int2 c = r.child[v];
        float b1[6];
        tri_box(pos, r.tmap[c.x - (n - 1)].x, b);
        tri_box(pos, r.tmap[c.y - (n - 1)].x, b1);
        for (int a = 0; a < 3; a++) { b[a] = min2(b[a], b1[a]); b[3 + a] = max2(b[3 + a], b1[3 + a]); }
    }
    for (int k = 0; k < 6; k++) o.box[(size_t)v * 6 + k] = b[k];
    o.hcur[v] = 0;
}

__global__ __launch_bounds__(256) void ro_keys(RbDev r)
{
    const int v = blockIdx.x * 256 + threadIdx.x;
    if (v >= r.n - 1) return;
    r.key_in[v] = r.wflag[v] ? (uint32_t)r.height[v] : (uint32_t)kDead;
}

// One wave per interior node of start-of-pass height `level`: the treelet of up to 7 entries below it, the optimal topology over
// them by dynamic programming over the 127 subsets (two per lane, rounds by subset size), and the rewiring by lane 0.
__global__ __launch_bounds__(kOptBlock) void ro_solve(RbDev r, RbOpt o, int level)
{
    static_assert(kOptBlock == 64 && (1 << kTreelet) == 2 * kOptBlock, "the subsets of a treelet are dealt two per lane of one wave64");
    __shared__ float lbox[kTreelet][6];
    __shared__ float larea[kTreelet];
    __shared__ float sa[128], sc[128];
    __shared__ uint8_t spart[128], sh[128];
    __shared__ int sL[kTreelet], sI[kTreelet], stS[16], stP[16], stSide[16];
    __shared__ int sm;
    const int lane = threadIdx.x;
    const int first = o.lvl[level], last = o.lvl[level + 1];
    int roots = 0, done = 0;
    for (int idx = first + (int)blockIdx.x; idx < last; idx += (int)gridDim.x) {
        __syncthreads();      // the treelet before is done with the shared arrays
        const int v = r.qsorted[idx];
        int hv = 0;
        float was = 0.f;
        if (lane == 0) {
            // 1: box and height of v from its current children
            const int2 c = r.child[v];
            float bv[6];
            for (int k = 0; k < 6; k++) { lbox[0][k] = o.box[(size_t)c.x * 6 + k]; lbox[1][k] = o.box[(size_t)c.y * 6 + k]; }
            for (int a = 0; a < 3; a++) { bv[a] = min2(lbox[0][a], lbox[1][a]); bv[3 + a] = max2(lbox[0][3 + a], lbox[1][3 + a]); }
            for (int k = 0; k < 6; k++) o.box[(size_t)v * 6 + k] = bv[k];
            const int hl = o.hcur[c.x], hr = o.hcur[c.y];
            hv = 1 + (hl > hr ? hl : hr);
            o.hcur[v] = hv;
            // 2: the treelet
            sL[0] = c.x; sL[1] = c.y;
            larea[0] = box_area(lbox[0]); larea[1] = box_area(lbox[1]);
            int m = 2, ni = 0;
            while (m < kTreelet) {
                int pick = -1;
                for (int k = 0; k < m; k++)
                    if (rb_is_interior(r, sL[k]) && (pick < 0 || larea[k] > larea[pick])) pick = k;
                if (pick < 0) break;
                const int e = sL[pick];
                was = ni == 0 ? larea[pick] : was + larea[pick];
                sI[ni++] = e;
                const int2 ec = r.child[e];
                for (int k = 0; k < 6; k++) { lbox[pick][k] = o.box[(size_t)ec.x * 6 + k]; lbox[m][k] = o.box[(size_t)ec.y * 6 + k]; }
                sL[pick] = ec.x; sL[m] = ec.y;
                larea[pick] = box_area(lbox[pick]); larea[m] = box_area(lbox[m]);
                m++;
            }
            for (int k = 0; k < m; k++) sh[1 << k] = (uint8_t)o.hcur[sL[k]];
            sm = m;
        }
        __syncthreads();
        const int m = sm;
        if (m < 3) continue;
        const int full = (1 << m) - 1;
        // 3: areas of all subsets, then the cheapest partition of each by rounds of subset size
        for (int S = lane; S <= full; S += kOptBlock) {
            if (S == 0) continue;
            float b[6];
            bool any = false;
            for (int k = 0; k < m; k++) {
                if (!((S >> k) & 1)) continue;
                for (int a = 0; a < 3; a++) {
                    b[a] = any ? min2(b[a], lbox[k][a]) : lbox[k][a];
                    b[3 + a] = any ? max2(b[3 + a], lbox[k][3 + a]) : lbox[k][3 + a];
                }
                any = true;
            }
            sa[S] = box_area(b);
            if ((S & (S - 1)) == 0) sc[S] = 0.f;
        }
        __syncthreads();
        for (int size = 2; size <= m; size++) {
            for (int S = lane; S <= full; S += kOptBlock) {
                if (__popc(S) != size) continue;
                const int low = S & -S, rest = S ^ low;
                int bp = low, sub = (0 - rest) & rest;
                float best = sc[low] + sc[rest];
                while (sub != rest) {      // P = low | sub ascends with sub; a later P only where strictly cheaper
                    const int P = low | sub;
                    const float cand = sc[P] + sc[S ^ P];
                    if (cand < best) { best = cand; bp = P; }
                    sub = (sub - rest) & rest;
                }
                spart[S] = (uint8_t)bp;
                sc[S] = (S == full ? 0.f : sa[S]) + best;
                const int h0 = sh[bp], h1 = sh[S ^ bp];
                sh[S] = (uint8_t)(1 + (h0 > h1 ? h0 : h1));
            }
            __syncthreads();
        }
        if (lane == 0) {      // the other lanes go on to the barrier at the top of the loop: every barrier is reached by the whole workgroup
            // 4: cheaper, and no deeper than the budget (or than the tree was) allows
            roots++;
            const int room = (o.h_lim >= 0 ? o.h_lim : r.levels[kLvDepth]) - r.depth[v];
            if (sc[full] < was && (int)sh[full] <= (hv > room ? hv : room)) {
                done++;
                // 5: rewire in pre-order; the nodes of I are handed out as the subsets of two or more entries are met
                int sp = 0, nxt = 0;
                stS[0] = full; stP[0] = -1; stSide[0] = 0; sp = 1;
                while (sp > 0) {
                    sp--;
                    const int S = stS[sp], pid = stP[sp], side = stSide[sp];
                    const bool single = (S & (S - 1)) == 0;
                    const int node = single ? sL[31 - __clz(S)] : pid < 0 ? v : sI[nxt++];
                    if (pid >= 0) {
                        reinterpret_cast<int32_t*>(&r.child[pid])[side] = node;
                        r.parent[node] = pid;
                    }
                    if (single) continue;
                    o.hcur[node] = sh[S];
                    if (pid >= 0) {
                        float b[6];
                        bool any = false;
                        for (int k = 0; k < m; k++) {
                            if (!((S >> k) & 1)) continue;
                            for (int a = 0; a < 3; a++) {
                                b[a] = any ? min2(b[a], lbox[k][a]) : lbox[k][a];
                                b[3 + a] = any ? max2(b[3 + a], lbox[k][3 + a]) : lbox[k][3 + a];
                            }
                            any = true;
                        }
                        for (int k = 0; k < 6; k++) o.box[(size_t)node * 6 + k] = b[k];
                    }
                    const int P = spart[S];
                    stS[sp] = S ^ P; stP[sp] = node; stSide[sp] = 1; sp++;
                    stS[sp] = P; stP[sp] = node; stSide[sp] = 0; sp++;
                }
            }
        }
    }
    if (lane == 0) {      // counts: they decide no index
        if (roots) atomicAdd(&r.levels[kLvRoots], roots);
        if (done) atomicAdd(&r.levels[kLvRestructured], done);
    }
}

inline unsigned blocks_of(int n) { return (unsigned)((n + 255) / 256); }

// temporary storage of the largest of the rocPRIM calls below (sizes only: nothing is launched with a null storage pointer)
hipError_t rocprim_temp_bytes(int n, size_t& bytes)
{
    const int N = 2 * n - 1;
    size_t b = 0;
    bytes = 0;
    hipError_t e = rocprim::radix_sort_keys(nullptr, b, (uint64_t*)nullptr, (uint64_t*)nullptr, n, 0, 62);
    if (e != hipSuccess) return e;
    bytes = b > bytes ? b : bytes;
    e = rocprim::radix_sort_pairs(nullptr, b, (uint32_t*)nullptr, (uint32_t*)nullptr, (int32_t*)nullptr, (int32_t*)nullptr, N, 0, 8);
    if (e != hipSuccess) return e;
    bytes = b > bytes ? b : bytes;
    e = rocprim::exclusive_scan(nullptr, b, (int32_t*)nullptr, (int32_t*)nullptr, 0, N, rocprim::plus<int32_t>());
    if (e != hipSuccess) return e;
    bytes = b > bytes ? b : bytes;
    return hipSuccess;
}

}  // namespace

static_assert(ptd::kCoreBlocks == 256, "rb_box_final reads one partial per thread of a 256-thread block");

// The limits of the traversal kernels, as pt_scene_create enforces them.  Host only.
int pt_tree_limits(const char* who, int depth, int quad_depth)
{
    if (depth > ptd::kStackDepth) {
        pt_set_error("%s: traversal tree depth %d exceeds the traversal stack (%d)", who, depth, ptd::kStackDepth);
        return PT_ERR_UNSUPPORTED;
    }
    if (3 * quad_depth + 2 > ptk_wf_stack_capacity()) {
        pt_set_error("%s: 4-wide traversal tree depth %d needs more than the %d stack entries of the traversal kernel", who, quad_depth, ptk_wf_stack_capacity());
        return PT_ERR_UNSUPPORTED;
    }
    return PT_OK;
}

// First rebuild of a scene: the arrays and maps whose record count a rebuild may change move into buffers of worst-case size
// (2 n - 1 builder nodes, n - 1 `nodes` and `quad` records) with their contents, and the build's own buffers are allocated.  All
// of it is built beside the scene and moved in only once every allocation exists (as pt_dyn_prepare does).
static int rb_prepare(PtScene* s, hipStream_t st)
{
    if (s->rb_ready) return PT_OK;
    const size_t n = (size_t)s->dyn.n_tris, N = 2 * n - 1, I = n > 1 ? n - 1 : 1;
    size_t temp = 0;
    HIPCHK(rocprim_temp_bytes((int)n, temp));
    struct { DevBuf* live; size_t bytes; } grow[] = {
        {&s->arr[kArrNodes], I * 64}, {&s->arr[kArrQuad], I * 64}, {&s->dyn_buf[kDynBn], N * 16}, {&s->dyn_buf[kDynOrder], N * 4},
        {&s->dyn_buf[kDynWideBn], I * 8}, {&s->dyn_buf[kDynQuadBn], I * 16}, {&s->dyn_buf[kDynBbox], N * 32},
        {&s->dyn_buf[kDynAreaPartial], ((N + kAreaBlock - 1) / kAreaBlock) * 8}};
    constexpr int kGrow = (int)(sizeof(grow) / sizeof(grow[0]));
    const size_t plan[kRbAllocs] = {n * 4, (size_t)ptd::kCoreBlocks * 32, 32, n * 8, n * 8, I * 8, I * 8, N * 4, N * 4, N * 4, N * 4, N * 4, I * 4, I * 4,
                                    N * 4, N * 4, I * 4, I * 4, I * 4, (size_t)kLvWords * 4, temp,
                                    N * 16, N * 4, I * 8, I * 16, n * 8, I * 8, I * 16};
    DevBuf fresh[kGrow], mine[kRbAllocs];
    int64_t bytes = 0;
    for (int k = 0; k < kGrow; k++) {
        HIPCHK(fresh[k].alloc(grow[k].bytes));
        bytes += (int64_t)fresh[k].held() - (int64_t)grow[k].live->held();
        if (grow[k].live->bytes()) HIPCHK(hipMemcpyAsync(fresh[k].as<>(), grow[k].live->as<>(), grow[k].live->bytes(), hipMemcpyDeviceToDevice, st));
    }
    for (int k = 0; k < kRbAllocs; k++) { HIPCHK(mine[k].alloc(plan[k])); bytes += (int64_t)mine[k].held(); }
    HIPCHK(hipStreamSynchronize(st));      // the copies are done, and so is whatever the stream still read from the old blocks
    for (int k = 0; k < kGrow; k++) *grow[k].live = std::move(fresh[k]);      // the old blocks are freed with `fresh`
    for (int k = 0; k < kRbAllocs; k++) s->rb_buf[k] = std::move(mine[k]);
    s->bytes += bytes;
    s->rb_temp_bytes = temp;
    ptd::DynScene& d = s->dyn;
    s->dev.nodes = d.nodes = s->arr[kArrNodes].as<float4>(); s->dev.quad = d.quad = s->arr[kArrQuad].as<uint4>();
    d.bn = s->dyn_buf[kDynBn].as<const int4>(); d.order = s->dyn_buf[kDynOrder].as<const int32_t>(); d.wide_bn = s->dyn_buf[kDynWideBn].as<const int2>();
    d.quad_bn = s->dyn_buf[kDynQuadBn].as<const int4>(); d.bbox = s->dyn_buf[kDynBbox].as<float4>(); d.area_partial = s->dyn_buf[kDynAreaPartial].as<double>();
    // prim -> reference leaf: the assignment defines the result and never changes
    RbDev r{};
    r.prim_leaf = s->rb_buf[kRbPrimLeaf].as<int32_t>();
    hipLaunchKernelGGL(rb_prim_leaf, dim3(blocks_of(d.n_leaves)), dim3(256), 0, st, d, r);
    HIPCHK(hipGetLastError());
    s->rb_ready = true;
    return PT_OK;
}

// First extended rebuild of a scene: the block only pt_scene_rebuild_tree_ex works in, and temporary storage of its own where the
// sort over all 64 key bits asks for more than the build's has.  pt_scene_rebuild_tree never allocates either.
static int rbx_prepare(PtScene* s)
{
    if (s->rbx_buf) return PT_OK;
    size_t b64 = 0;
    HIPCHK(rocprim::radix_sort_keys(nullptr, b64, (uint64_t*)nullptr, (uint64_t*)nullptr, s->dyn.n_tris, 0, 64));
    DevBuf block, temp;
    HIPCHK(block.alloc(kRxBytes));
    if (b64 > s->rb_temp_bytes) HIPCHK(temp.alloc(b64));
    s->bytes += (int64_t)block.held() + (int64_t)temp.held();
    s->rbx_buf = std::move(block);
    s->rbx_temp = std::move(temp);
    return PT_OK;
}

// First optimised rebuild of a scene: the block only pt_scene_rebuild_tree_opt works in (28 bytes per raw node and 1.6 KB).  The two
// older calls never allocate it.
static size_t rbo_bytes(size_t n) { return kRoHeights + (2 * n - 1) * 4 + (2 * n - 1) * 24; }

static int rbo_prepare(PtScene* s)
{
    if (s->rbo_buf) return PT_OK;
    DevBuf block;
    HIPCHK(block.alloc(rbo_bytes((size_t)s->dyn.n_tris)));
    s->bytes += (int64_t)block.held();
    s->rbo_buf = std::move(block);
    return PT_OK;
}

static RbDev rb_args(PtScene* s)
{
    DevBuf* b = s->rb_buf;
    RbDev r;
    r.prim_leaf = b[kRbPrimLeaf].as<int32_t>(); r.box_partial = b[kRbBoxPartial].as<float>(); r.cbox = b[kRbCbox].as<float>();
    r.keys = b[kRbKeys].as<uint64_t>(); r.sorted = b[kRbSorted].as<uint64_t>(); r.child = b[kRbChild].as<int2>(); r.range = b[kRbRange].as<int2>();
    r.parent = b[kRbParent].as<int32_t>(); r.depth = b[kRbDepth].as<int32_t>(); r.height = b[kRbHeight].as<int32_t>(); r.live = b[kRbLive].as<int32_t>();
    r.newid = b[kRbNewId].as<int32_t>(); r.wflag = b[kRbWFlag].as<int32_t>(); r.widx = b[kRbWidx].as<int32_t>();
    r.key_in = b[kRbKeyIn].as<uint32_t>(); r.key_out = b[kRbKeyOut].as<uint32_t>(); r.iota = b[kRbIota].as<int32_t>(); r.qsorted = b[kRbQSorted].as<int32_t>();
    r.qidx = b[kRbQidx].as<int32_t>(); r.levels = b[kRbLevels].as<int32_t>();
    r.bn = b[kRbBn].as<int4>(); r.order = b[kRbOrder].as<int32_t>(); r.wide_bn = b[kRbWideBn].as<int2>(); r.quad_bn = b[kRbQuadBn].as<int4>();
    r.tmap = b[kRbTmap].as<int2>(); r.node_ref = b[kRbNodeRef].as<int2>(); r.quad_ref = b[kRbQuadRef].as<int4>();
    r.n = s->dyn.n_tris;
    return r;
}

// Enqueues the whole build of the topology into the staging buffers.  Nothing a render reads is written.  x: the extended call
// (pt_scene_rebuild_tree_ex) with its depth budget, NULL for pt_scene_rebuild_tree.  o: the optimised call
// (pt_scene_rebuild_tree_opt) with its number of restructuring passes, NULL for the other two.
static int rb_build(PtScene* s, const RbDev& r, hipStream_t st, const RbEx* x = nullptr, int budget = 0, const RbOpt* o = nullptr, int passes = 0)
{
    const int n = r.n, N = 2 * n - 1;
    const float* pos = s->dyn_buf[kDynPos].as<const float>();
    void* temp = s->rb_buf[kRbTemp].as<>();
    size_t tb = s->rb_temp_bytes;
    if (x) HIPCHK(hipMemsetAsync(r.levels, 0, (size_t)(o ? kLvWordsOpt : kLvWordsEx) * 4, st));      // the report's counts are summed from here on
    hipLaunchKernelGGL(rb_box_partial, dim3(ptd::kCoreBlocks), dim3(256), 0, st, r, pos);
    hipLaunchKernelGGL(rb_box_final, dim3(1), dim3(256), 0, st, r);
    if (x && x->large_fraction > 0.f) {      // a centroid box per size class; the class is bit 62 of the key
        hipLaunchKernelGGL(rb_class_partial, dim3(ptd::kCoreBlocks), dim3(256), 0, st, r, *x, pos);
        hipLaunchKernelGGL(rb_class_final, dim3(1), dim3(256), 0, st, *x);
        hipLaunchKernelGGL(rb_keys_classes, dim3(blocks_of(n)), dim3(256), 0, st, r, *x, pos);
        HIPCHK(hipGetLastError());
        void* temp64 = s->rbx_temp ? s->rbx_temp.as<>() : temp;
        tb = s->rbx_temp ? s->rbx_temp.bytes() : s->rb_temp_bytes;
        HIPCHK(rocprim::radix_sort_keys(temp64, tb, r.keys, r.sorted, n, 0, 64, st));
    } else {
        hipLaunchKernelGGL(rb_keys, dim3(blocks_of(n)), dim3(256), 0, st, r, pos);
        HIPCHK(hipGetLastError());
        HIPCHK(rocprim::radix_sort_keys(temp, tb, r.keys, r.sorted, n, 0, 62, st));
    }
    hipLaunchKernelGGL(rb_tmap, dim3(blocks_of(n)), dim3(256), 0, st, r);
    if (n <= 2) {
        hipLaunchKernelGGL(rb_single, dim3(1), dim3(64), 0, st, r);
        HIPCHK(hipGetLastError());
        return PT_OK;
    }
    if (!x) HIPCHK(hipMemsetAsync(r.levels, 0, (size_t)kLvWords * 4, st));
    hipLaunchKernelGGL(rb_karras, dim3(blocks_of(n - 1)), dim3(256), 0, st, r);
    hipLaunchKernelGGL(rb_depth, dim3(blocks_of(N)), dim3(256), 0, st, r);
    if (budget > 0) {      // flatten what would be deeper than the budget, then the tree over the new keys (they are in `keys`)
        RbDev again = r;
        again.sorted = r.keys;
        hipLaunchKernelGGL(rb_rekey, dim3(blocks_of(n)), dim3(256), 0, st, r, budget);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemsetAsync(r.levels + kLvDepth, 0, 4, st));
        hipLaunchKernelGGL(rb_karras, dim3(blocks_of(n - 1)), dim3(256), 0, st, again);
        hipLaunchKernelGGL(rb_depth, dim3(blocks_of(N)), dim3(256), 0, st, again);
    }
    if (o && passes > 0) {      // treelet restructuring: per pass the heights, the interior nodes by height, one launch per height, the depths anew
        const int top = budget > 0 ? budget - 1 : 63;      // no interior node is higher: the tree keeps the budget, and a radix tree over unique keys of at most 63 significant bits is at most 63 deep
        hipLaunchKernelGGL(ro_init, dim3(blocks_of(N)), dim3(256), 0, st, r, *o, pos);
        for (int pass = 0; pass < passes; pass++) {
            hipLaunchKernelGGL(rb_height, dim3(blocks_of(N)), dim3(256), 0, st, r);
            hipLaunchKernelGGL(ro_keys, dim3(blocks_of(n - 1)), dim3(256), 0, st, r);
            HIPCHK(hipGetLastError());
            tb = s->rb_temp_bytes;
            HIPCHK(rocprim::radix_sort_pairs(temp, tb, r.key_in, r.key_out, r.iota, r.qsorted, n - 1, 0, 8, st));
            hipLaunchKernelGGL(rb_level_start, dim3(blocks_of(n - 1)), dim3(256), 0, st, r.key_out, n - 1, o->lvl);
            for (int h = 1; h <= top; h++) hipLaunchKernelGGL(ro_solve, dim3(kOptGrid), dim3(kOptBlock), 0, st, r, *o, h);
            HIPCHK(hipGetLastError());
            HIPCHK(hipMemsetAsync(r.levels + kLvDepth, 0, 4, st));
            hipLaunchKernelGGL(rb_depth, dim3(blocks_of(N)), dim3(256), 0, st, r);
        }
    }
    hipLaunchKernelGGL(rb_height, dim3(blocks_of(N)), dim3(256), 0, st, r);
    HIPCHK(hipGetLastError());
    // numbering: builder nodes and `nodes` records by rank, `order` by height, `quad` records by level
    tb = s->rb_temp_bytes;
    HIPCHK(rocprim::exclusive_scan(temp, tb, r.live, r.newid, 0, N, rocprim::plus<int32_t>(), st));
    tb = s->rb_temp_bytes;
    HIPCHK(rocprim::exclusive_scan(temp, tb, r.wflag, r.widx, 0, n - 1, rocprim::plus<int32_t>(), st));
    hipLaunchKernelGGL(rb_height_keys, dim3(blocks_of(N)), dim3(256), 0, st, r);
    tb = s->rb_temp_bytes;
    HIPCHK(rocprim::radix_sort_pairs(temp, tb, r.key_in, r.key_out, r.newid, r.order, N, 0, 8, st));
    hipLaunchKernelGGL(rb_level_start, dim3(blocks_of(N)), dim3(256), 0, st, r.key_out, N, r.levels + kLvOrder);
    hipLaunchKernelGGL(rb_level_keys, dim3(blocks_of(n - 1)), dim3(256), 0, st, r);
    tb = s->rb_temp_bytes;
    HIPCHK(rocprim::radix_sort_pairs(temp, tb, r.key_in, r.key_out, r.iota, r.qsorted, n - 1, 0, 8, st));
    hipLaunchKernelGGL(rb_level_start, dim3(blocks_of(n - 1)), dim3(256), 0, st, r.key_out, n - 1, r.levels + kLvQuad);
    hipLaunchKernelGGL(rb_qidx, dim3(blocks_of(n - 1)), dim3(256), 0, st, r);
    hipLaunchKernelGGL(rb_emit, dim3(blocks_of(N)), dim3(256), 0, st, r);
    HIPCHK(hipGetLastError());
    return PT_OK;
}

// The rebuild behind the three entry points.  p: the parameters of pt_scene_rebuild_tree_ex (checked by the caller), NULL for
// pt_scene_rebuild_tree, whose launches, waits and allocations are exactly what they were before the extended call existed.
// passes >= 0: pt_scene_rebuild_tree_opt (p is not NULL), with its own report; -1 for the other two, which are what they were too.
static int rb_run(PtScene* s, const char* who, const PtRebuildParams* p, PtRebuildReport* report, hipStream_t st, int passes = -1,
                  PtRebuildOptReport* opt_report = nullptr)
{
    HIPCHK(hipSetDevice(s->device));
    int rc;
    if ((rc = pt_dyn_prepare(s)) != PT_OK) return rc;
    if ((rc = rb_prepare(s, st)) != PT_OK) return rc;
    if (p && (rc = rbx_prepare(s)) != PT_OK) return rc;
    const bool opt = passes >= 0;
    if (opt && (rc = rbo_prepare(s)) != PT_OK) return rc;
    RbDev r = rb_args(s);
    RbEx x{};
    RbOpt o{};
    if (p) {
        char* base = s->rbx_buf.as<char>();
        x.class_partial = (float*)(base + kRxClassPartial); x.class_box = (float*)(base + kRxClassBox); x.large_fraction = p->large_fraction;
        r.levels = (int32_t*)(base + kRxLevels);
    }
    if (opt) {
        char* base = s->rbo_buf.as<char>();
        r.levels = (int32_t*)(base + kRoLevels);
        o.lvl = (int32_t*)(base + kRoPassLevels); o.hcur = (int32_t*)(base + kRoHeights); o.box = (float*)(base + kRoHeights + (2 * (size_t)r.n - 1) * 4);
        o.h_lim = p->depth_budget > 0 ? p->depth_budget - 1 : -1;
    }
    if ((rc = rb_build(s, r, st, p ? &x : nullptr, p ? p->depth_budget : 0, opt ? &o : nullptr, opt ? passes : 0)) != PT_OK) return rc;
    // wait 1: the level offsets, the counts and the depths (and, behind them, the two counts of the extended call's report)
    int32_t lv[kLvWordsOpt] = {};
    HIPCHK(hipMemcpyAsync(lv, r.levels, (size_t)(opt ? kLvWordsOpt : p ? kLvWordsEx : kLvWords) * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (report) { report->n_large = lv[kLvLarge]; report->n_flattened_tris = lv[kLvFlattened]; }
    if (opt_report) { opt_report->n_large = lv[kLvLarge]; opt_report->n_flattened_tris = lv[kLvFlattened]; opt_report->n_roots = lv[kLvRoots]; opt_report->n_restructured = lv[kLvRestructured]; }
    const int n_bn = lv[kLvOrder + kDead], n_quad = lv[kLvQuad + kDead], n_wide = n_bn > 1 ? (n_bn - 1) / 2 : 1;
    int top = 0, quad_depth = 0;
    while (lv[kLvOrder + top + 1] < n_bn) top++;                 // heights 0 .. top
    while (lv[kLvQuad + quad_depth + 1] < n_quad) quad_depth++;      // levels 0 .. quad_depth
    const int depth = lv[kLvDepth];
    if ((rc = pt_tree_limits(who, depth, quad_depth)) != PT_OK) return rc;      // nothing a render, a query or an update reads has been written
    // ---- commit ----
    ptd::DynScene& d = s->dyn;
    const struct { int dst, src; size_t bytes; } maps[] = {{kDynBn, kRbBn, (size_t)n_bn * 16}, {kDynOrder, kRbOrder, (size_t)n_bn * 4}, {kDynWideBn, kRbWideBn, (size_t)n_wide * 8},
                                                           {kDynQuadBn, kRbQuadBn, (size_t)n_quad * 16}, {kDynTmap, kRbTmap, (size_t)d.n_tris * 8}};
    for (const auto& m : maps) HIPCHK(hipMemcpyAsync(s->dyn_buf[m.dst].as<>(), s->rb_buf[m.src].as<>(), m.bytes, hipMemcpyDeviceToDevice, st));
    d.n_bn = n_bn; d.n_wide = n_wide; d.n_quad = n_quad;
    s->dev.n_nodes = n_wide; s->dev.n_quad = n_quad; s->dev.quad_depth = quad_depth;
    s->max_depth = depth;
    s->dyn_host.level_start.assign(lv + kLvOrder, lv + kLvOrder + top + 2);
    hipLaunchKernelGGL(rb_refs, dim3(blocks_of(n_wide > n_quad ? n_wide : n_quad)), dim3(256), 0, st, d, r);
    HIPCHK(hipGetLastError());
    // tri, tripair, every box of `nodes`, origin / scales / quantised boxes of `quad`, from the scene's own positions
    HIPCHK(pt_dyn_launch_update(d, s->dyn_buf[kDynPos].as<const float>(), nullptr, nullptr, s->dyn_host.level_start.data(), top + 1, /*trees_only=*/true, st));
    // wait 2: the new denominator of pt_scene_tree_inflation, by the same reduction in the same order
    s->h_area.assign(((size_t)n_bn + kAreaBlock - 1) / kAreaBlock, 0.0);
    HIPCHK(pt_dyn_launch_area(d, st));
    HIPCHK(hipMemcpyAsync(s->h_area.data(), d.area_partial, s->h_area.size() * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    double sum = 0.0;
    for (double v : s->h_area) sum += v;
    s->dyn_host.area_sum = sum;
    s->rebuilds++;
    return PT_OK;
}

extern "C" {

int pt_scene_rebuild_tree(PtScene* s, void* hip_stream)
{
    if (!s) { pt_set_error("pt_scene_rebuild_tree: NULL scene"); return PT_ERR_INVALID; }
    return rb_run(s, "pt_scene_rebuild_tree", nullptr, nullptr, (hipStream_t)hip_stream);
}

void pt_rebuild_params_default(PtRebuildParams* p)
{
    if (p) { p->depth_budget = 26; p->large_fraction = 0.0625f; }
}

// The parameter checks of pt_scene_rebuild_tree_ex, under the name of the entry point that applies them.  No HIP call.
static int rb_check_params(const char* who, const PtScene* s, const PtRebuildParams* p)
{
    if (!s || !p) { pt_set_error("%s: NULL %s", who, !s ? "scene" : "params"); return PT_ERR_INVALID; }
    if (p->depth_budget < 0 || p->depth_budget > ptd::kStackDepth) {
        pt_set_error("%s: depth_budget %d is not in 0 .. %d", who, p->depth_budget, ptd::kStackDepth);
        return PT_ERR_INVALID;
    }
    if (!(p->large_fraction >= 0.f) || std::isinf(p->large_fraction)) {
        pt_set_error("%s: large_fraction %g is not a finite number >= 0", who, (double)p->large_fraction);
        return PT_ERR_INVALID;
    }
    return PT_OK;
}

static int rb_check_budget(const char* who, const PtScene* s, const PtRebuildParams* p)
{
    const int n = s->dyn.n_tris;
    int need = 0;
    while (n >= 3 && need < 32 && ((int64_t)1 << need) < n) need++;      // clog2(n): a tree over n triangles is at least that deep
    if (p->depth_budget > 0 && p->depth_budget < need) {
        pt_set_error("%s: depth_budget %d is below %d, the depth of a balanced tree over %d triangles", who, p->depth_budget, need, n);
        return PT_ERR_INVALID;
    }
    return PT_OK;
}

int pt_scene_rebuild_tree_ex(PtScene* s, const PtRebuildParams* p, PtRebuildReport* report, void* hip_stream)
{
    const char* who = "pt_scene_rebuild_tree_ex";
    int rc;
    if ((rc = rb_check_params(who, s, p)) != PT_OK || (rc = rb_check_budget(who, s, p)) != PT_OK) return rc;
    return rb_run(s, who, p, report, (hipStream_t)hip_stream);
}

int32_t pt_rebuild_opt_passes_default(void) { return kOptPassesDefault; }

int pt_scene_rebuild_tree_opt(PtScene* s, const PtRebuildParams* p, int32_t passes, PtRebuildOptReport* report, void* hip_stream)
{
    const char* who = "pt_scene_rebuild_tree_opt";
    int rc;
    if ((rc = rb_check_params(who, s, p)) != PT_OK) return rc;
    if (passes < 0 || passes > kOptMaxPasses) {      // before the scene is read: the checks above and this one need no scene
        pt_set_error("%s: passes %d is not in 0 .. %d", who, passes, kOptMaxPasses);
        return PT_ERR_INVALID;
    }
    if ((rc = rb_check_budget(who, s, p)) != PT_OK) return rc;
    return rb_run(s, who, p, nullptr, (hipStream_t)hip_stream, passes, report);
}

int pt_scene_tree_info(const PtScene* s, PtTreeInfo* out)
{
    if (!s || !out) { pt_set_error("pt_scene_tree_info: NULL %s", !s ? "scene" : "out"); return PT_ERR_INVALID; }
    out->n_wide = s->dev.n_nodes; out->n_quad = s->dev.n_quad; out->depth = s->max_depth; out->quad_depth = s->dev.quad_depth; out->rebuilds = s->rebuilds;
    return PT_OK;
}

int pt_dbg_tree_limits(int32_t depth, int32_t quad_depth, int32_t* max_depth, int32_t* max_quad_depth)
{
    if (max_depth) *max_depth = ptd::kStackDepth;
    if (max_quad_depth) *max_quad_depth = (ptk_wf_stack_capacity() - 2) / 3;
    return pt_tree_limits("pt_dbg_tree_limits", depth, quad_depth);
}

}  // extern "C"
