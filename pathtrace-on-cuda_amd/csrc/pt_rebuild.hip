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
// One build serves the three entry points; it is a function of (depth_budget, large_fraction, passes).  large_fraction > 0 (DESIGN.md
// section 24): the triangles' size class is bit 62 of the key, each class quantised in a centroid box of its own.  depth_budget > 0:
// every triangle rewrites its key below the topmost ancestor that would reach below the budget, and the radix tree is built a second
// time over the new keys.  passes > 0: treelet restructuring passes by surface area between that tree and the
// numbering.  {0, 0, 0} is the plain rebuild.  What a scene holds follows the same three numbers (the workspace table below; DESIGN.md
// section 26).
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
using ptd::min2;
using ptd::max2;

constexpr int kDead = 127;           // sort key of a raw node that gets no number (heights and levels are below 64: unique keys with at most 63 significant bits)
constexpr int kLevelSlots = 129;     // first index with key >= h, h = 0 .. 128
// The words read back before the commit, one block: level offsets of `order`, level offsets of the 4-wide numbering, deepest builder
// node, the report's four counts.  Cleared once at the start of every build, always read back whole.
constexpr int kLvOrder = 0, kLvQuad = kLevelSlots, kLvDepth = 2 * kLevelSlots, kLvLarge = kLvDepth + 2, kLvFlattened = kLvLarge + 1, kLvRoots = kLvLarge + 2,
              kLvRestructured = kLvLarge + 3, kLvWords = kLvLarge + 4;
constexpr int kTreelet = 7, kOptMaxPasses = 8, kOptPassesDefault = 2;
constexpr int kOptBlock = 64;        // ro_solve: a workgroup is one wave64, two of the 128 subsets per lane
constexpr int kOptGrid = 4096;      // one wave per treelet, grid-stride over the level's slice (its size is known on the device only)

// What a build is a function of, beside the positions (the entry points check the ranges), and the four counts it reports.
struct RbParams { int depth_budget; float large_fraction; int passes; };
struct RbReport { int n_large, n_flattened_tris, n_roots, n_restructured; bool known; };      // known: wait 1 came back (a refused build reports too)

// ---- the workspace: every buffer of a build stated once — element type, name, elements, when it is needed ------------------------------
// RbDev's pointers, the slots of PtScene::rb_buf and rb_prepare's allocations all follow from this list, whatever its order.
// The counts are evaluated in rb_prepare: n = triangles, N = 2 n - 1 raw nodes, I = max(n - 1, 1) internal nodes, temp_bytes and
// temp64_bytes from rocprim_temp_bytes.  A buffer of no elements is not allocated.
enum RbNeed { kAlways = 1, kClasses = 2 /* large_fraction > 0 */, kPasses = 4 /* passes > 0 */ };
#define RB_WORKSPACE(X)                                                                                                                          \
    X(int32_t,  prim_leaf,     n,                     kAlways)  /* reference leaf of every prim (written once per scene) */                      \
    X(float,    box_partial,   ptd::kCoreBlocks * 8,  kAlways)                                                                                   \
    X(float,    cbox,          8,                     kAlways)  /* lo.xyz hi.xyz of the centroids */                                             \
    X(uint64_t, keys,          n,                     kAlways)  /* unsorted */                                                                   \
    X(uint64_t, sorted,        n,                     kAlways)                                                                                   \
    X(int2,     child,         I,                     kAlways)  /* raw l, r */                                                                   \
    X(int2,     range,         I,                     kAlways)  /* first, last sorted triangle */                                                \
    X(int32_t,  parent,        N,                     kAlways)                                                                                   \
    X(int32_t,  depth,         N,                     kAlways)                                                                                   \
    X(int32_t,  height,        N,                     kAlways)                                                                                   \
    X(int32_t,  live,          N,                     kAlways)  /* 1 = gets a builder node */                                                    \
    X(int32_t,  newid,         N,                     kAlways)  /* builder node */                                                               \
    X(int32_t,  wflag,         I,                     kAlways)  /* 1 = interior (more than two triangles) */                                     \
    X(int32_t,  widx,          I,                     kAlways)  /* `nodes` record */                                                             \
    X(uint32_t, key_in,        N,                     kAlways)  /* sort keys (height, then level) */                                             \
    X(uint32_t, key_out,       N,                     kAlways)                                                                                   \
    X(int32_t,  iota,          I,                     kAlways)                                                                                   \
    X(int32_t,  qsorted,       I,                     kAlways)  /* raw internal nodes by level (in a pass: by height) */                         \
    X(int32_t,  qidx,          I,                     kAlways)  /* `quad` record */                                                              \
    X(int32_t,  levels,        kLvWords,              kAlways)  /* the words read back */                                                        \
    X(char,     temp,          temp_bytes,            kAlways)  /* rocPRIM temporary storage */                                                  \
    X(int4,     bn,            N,                     kAlways)  /* the new maps and refs, staged: this line and the six below */                 \
    X(int32_t,  order,         N,                     kAlways)                                                                                   \
    X(int2,     wide_bn,       I,                     kAlways)                                                                                   \
    X(int4,     quad_bn,       I,                     kAlways)                                                                                   \
    X(int2,     tmap,          n,                     kAlways)                                                                                   \
    X(int2,     node_ref,      I,                     kAlways)                                                                                   \
    X(int4,     quad_ref,      I,                     kAlways)                                                                                   \
    X(float,    class_partial, ptd::kCoreBlocks * 16, kClasses) /* per block: small lo.xyz hi.xyz, pad, large lo.xyz hi.xyz, pad */              \
    X(float,    class_box,     16,                    kClasses) /* the same layout */                                                            \
    X(char,     temp64,        temp64_bytes,          kClasses) /* only where the sort over all 64 key bits asks for more than `temp` has */     \
    X(int32_t,  lvl,           kLevelSlots,           kPasses)  /* first index of `qsorted` with start-of-pass height >= h (device only) */      \
    X(int32_t,  hcur,          N,                     kPasses)  /* height now (leaf = 0) */                                                      \
    X(float,    box,           N * 6,                 kPasses)  /* lo.xyz hi.xyz */

#define X(T, name, count, need) kRb_##name,
enum RbSlot { RB_WORKSPACE(X) kRbSlots };
#undef X

struct RbDev {
#define X(T, name, count, need) T* name;
    RB_WORKSPACE(X)
#undef X
    int32_t n;
    float large_fraction;      // > 0 where the kernels of the size classes run
    int32_t h_lim;             // a pass: budget - 1, or -1: the depth of the tree the pass started from (levels[kLvDepth])
};

// ---- prim -> reference leaf (once per scene) ------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void rb_prim_leaf(DynScene s, RbDev r)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= s.n_leaves) return;
    const int2 lr = s.leaf_range[i];
    for (int k = 0; k < lr.y; k++) r.prim_leaf[lr.x + k] = i;
}

// ---- a triangle's own box; its centroid and its longest side follow from it --------------------------------------------------------
__device__ __forceinline__ void tri_box(const float* __restrict__ pos, int prim, float* b)
{
    const Tri9 t = load_tri(pos, prim);
    for (int a = 0; a < 3; a++) {
        b[a] = min2(t.v0[a], min2(t.v1[a], t.v2[a]));
        b[3 + a] = max2(t.v0[a], max2(t.v1[a], t.v2[a]));
    }
}
__device__ __forceinline__ void centroid(const float* b, float* c) { for (int a = 0; a < 3; a++) c[a] = 0.5f * (b[a] + b[3 + a]); }
__device__ __forceinline__ float longest_side(const float* b) { return max2(max2(max2(0.f, b[3] - b[0]), b[4] - b[1]), b[5] - b[2]); }
__device__ __forceinline__ float box_area(const float* b) { return ptd::box_area(b[3] - b[0], b[4] - b[1], b[5] - b[2]); }

// ---- centroid box: two stages in the shape of dyn_core_partial / dyn_core_final, no float atomics ------------------------------
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

// the 256 partial boxes of the first stage (one per thread, `stride` floats apart) into one box
__device__ __forceinline__ void reduce_partials(const float* __restrict__ partial, int stride, float* __restrict__ box, float (*lds)[6])
{
    float v[6];
    for (int k = 0; k < 6; k++) v[k] = partial[threadIdx.x * stride + k];      // kCoreBlocks == the block size
    block_box(v, lds);
    if (threadIdx.x == 0) for (int k = 0; k < 6; k++) box[k] = lds[0][k];
}

__global__ __launch_bounds__(256) void rb_box_partial(RbDev r, const float* __restrict__ pos)
{
    __shared__ float lds[256][6];
    float v[6] = {FLT_MAX, FLT_MAX, FLT_MAX, -FLT_MAX, -FLT_MAX, -FLT_MAX};
    for (int i = blockIdx.x * 256 + threadIdx.x; i < r.n; i += ptd::kCoreBlocks * 256) {
        float b[6], c[3];
        tri_box(pos, i, b);
        centroid(b, c);
        for (int a = 0; a < 3; a++) { v[a] = min2(v[a], c[a]); v[3 + a] = max2(v[3 + a], c[a]); }
    }
    block_box(v, lds);
    if (threadIdx.x == 0) for (int k = 0; k < 6; k++) r.box_partial[blockIdx.x * 8 + k] = lds[0][k];
}

__global__ __launch_bounds__(256) void rb_box_final(RbDev r)
{
    __shared__ float lds[256][6];
    reduce_partials(r.box_partial, 8, r.cbox, lds);
}

// the same per size class.  A triangle is large where its longest side exceeds f * E, E the longest side of the box of all centroids
// (rb_box_final has written it)
__device__ __forceinline__ float large_bound(const RbDev& r)
{
    const float E = max2(r.cbox[3] - r.cbox[0], max2(r.cbox[4] - r.cbox[1], r.cbox[5] - r.cbox[2]));
    return r.large_fraction * E;
}

__global__ __launch_bounds__(256) void rb_class_partial(RbDev r, const float* __restrict__ pos)
{
    __shared__ float lds[256][6];
    __shared__ int n_large;
    float v[12] = {FLT_MAX, FLT_MAX, FLT_MAX, -FLT_MAX, -FLT_MAX, -FLT_MAX, FLT_MAX, FLT_MAX, FLT_MAX, -FLT_MAX, -FLT_MAX, -FLT_MAX};
    if (threadIdx.x == 0) n_large = 0;
    const float bound = large_bound(r);
    int mine = 0;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < r.n; i += ptd::kCoreBlocks * 256) {
        float b[6], c[3];
        tri_box(pos, i, b);
        centroid(b, c);
        const bool large = longest_side(b) > bound;
        mine += large ? 1 : 0;
        for (int a = 0; a < 3; a++) {
            const float lo_s = large ? v[a] : min2(v[a], c[a]), hi_s = large ? v[3 + a] : max2(v[3 + a], c[a]);
            const float lo_l = large ? min2(v[6 + a], c[a]) : v[6 + a], hi_l = large ? max2(v[9 + a], c[a]) : v[9 + a];
            v[a] = lo_s; v[3 + a] = hi_s; v[6 + a] = lo_l; v[9 + a] = hi_l;
        }
    }
    for (int cls = 0; cls < 2; cls++) {      // after block_box only thread 0 reads lds, and only the row it alone writes
        block_box(v + 6 * cls, lds);
        if (threadIdx.x == 0) for (int k = 0; k < 6; k++) r.class_partial[blockIdx.x * 16 + cls * 8 + k] = lds[0][k];
    }
    if (mine) atomicAdd(&n_large, mine);
    __syncthreads();
    if (threadIdx.x == 0 && n_large) atomicAdd(&r.levels[kLvLarge], n_large);      // a count: it decides no index
}

__global__ __launch_bounds__(256) void rb_class_final(RbDev r)
{
    __shared__ float lds[256][6];
    for (int cls = 0; cls < 2; cls++) reduce_partials(r.class_partial + cls * 8, 16, r.class_box + cls * 8, lds);
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

// the Morton code of the cell of centroid c in `box` (lo.xyz hi.xyz)
__device__ __forceinline__ uint32_t morton_cell(const float* __restrict__ box, const float* c)
{
    uint32_t q[3];
    for (int a = 0; a < 3; a++) {
        const float lo = box[a], ext = box[3 + a] - lo;
        int v = 0;
        if (ext > 0.f) { v = (int)(((c[a] - lo) / ext) * 1024.0f); if (v > 1023) v = 1023; }
        q[a] = (uint32_t)v;
    }
    return (spread3(q[0]) << 2) | (spread3(q[1]) << 1) | spread3(q[2]);
}

// kClasses: the cell is taken in the box of the triangle's own class, and the class goes above the Morton code.  Without classes the
// size test is not evaluated at all: with a fraction of 0 it would call every non-degenerate triangle large.
template <bool kClasses>
__global__ __launch_bounds__(256) void rb_keys(RbDev r, const float* __restrict__ pos)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= r.n) return;
    float b[6], c[3];
    tri_box(pos, i, b);
    centroid(b, c);
    const bool large = kClasses && longest_side(b) > large_bound(r);
    const float* __restrict__ box = kClasses ? r.class_box + (large ? 8 : 0) : r.cbox;
    r.keys[i] = ((uint64_t)(large ? 1 : 0) << 62) | ((uint64_t)morton_cell(box, c) << 32) | (uint32_t)i;
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

// ---- treelet restructuring passes over the radix tree (include/pt_api.h: "Tree rebuild with treelet restructuring"; DESIGN.md section
// 25; Karras and Aila 2013).  A pass runs between the last rb_karras / rb_depth and the numbering and
// rewires `child` / `parent` of interior nodes only: leaves (singletons and internal nodes over two triangles) are never opened, so
// everything below — rb_depth, rb_height, the scans, rb_emit — runs as it is.  Interior nodes are taken in ascending start-of-pass height,
// one launch per height; the nodes of one height are roots of disjoint subtrees and a restructure stays inside its root's subtree, so no
// data passes between workgroups within a launch.

// boxes and heights of the leaves: singletons, and internal nodes over two triangles (rb_depth has written wflag)
__global__ __launch_bounds__(256) void ro_init(RbDev r, const float* __restrict__ pos)
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
    for (int k = 0; k < 6; k++) r.box[(size_t)v * 6 + k] = b[k];
    r.hcur[v] = 0;
}

__global__ __launch_bounds__(256) void ro_keys(RbDev r)
{
    const int v = blockIdx.x * 256 + threadIdx.x;
    if (v >= r.n - 1) return;
    r.key_in[v] = r.wflag[v] ? (uint32_t)r.height[v] : (uint32_t)kDead;
}

// One wave per interior node of start-of-pass height `level`: the treelet of up to 7 entries below it (lane 0), the optimal topology
// over them by dynamic programming over the 127 subsets (two per lane, rounds by subset size), and the rewiring (lane 0).
struct Treelet {      // the shared arrays of one workgroup
    float lbox[kTreelet][6], larea[kTreelet];      // box and area of every entry
    float sa[128], sc[128];                        // per subset: area of its box, cost of its cheapest topology
    uint8_t spart[128], sh[128];                   // per subset: one side of its cheapest partition, height of that topology
    int sL[kTreelet], sI[kTreelet];                // raw nodes: the entries, the interior nodes opened
    int stS[16], stP[16], stSide[16];              // the rewiring's stack: subset, parent, side
    int sm;                                        // entries
};

// box of the entries in S: the lowest first, then ascending (include/pt_api.h fixes the order)
__device__ __forceinline__ void subset_box(int S, int m, const float (*lbox)[6], float* b)
{
    int k = __ffs(S) - 1;
    for (int j = 0; j < 6; j++) b[j] = lbox[k][j];
    for (k++; k < m; k++) {
        if (!((S >> k) & 1)) continue;
        for (int a = 0; a < 3; a++) { b[a] = min2(b[a], lbox[k][a]); b[3 + a] = max2(b[3 + a], lbox[k][3 + a]); }
    }
}

// Lane 0.  Box and height of v from its current children, then the treelet: the interior entry of the largest area is opened until
// there are 7 entries or none is interior.  Returns v's height; was = the summed area of the opened nodes.
__device__ __forceinline__ int ro_form(const RbDev& r, Treelet& t, int v, float& was)
{
    const int2 c = r.child[v];
    float bv[6];
    for (int k = 0; k < 6; k++) { t.lbox[0][k] = r.box[(size_t)c.x * 6 + k]; t.lbox[1][k] = r.box[(size_t)c.y * 6 + k]; }
    for (int a = 0; a < 3; a++) { bv[a] = min2(t.lbox[0][a], t.lbox[1][a]); bv[3 + a] = max2(t.lbox[0][3 + a], t.lbox[1][3 + a]); }
    for (int k = 0; k < 6; k++) r.box[(size_t)v * 6 + k] = bv[k];
    const int hl = r.hcur[c.x], hr = r.hcur[c.y];
    const int hv = 1 + (hl > hr ? hl : hr);
    r.hcur[v] = hv;
    t.sL[0] = c.x; t.sL[1] = c.y;
    t.larea[0] = box_area(t.lbox[0]); t.larea[1] = box_area(t.lbox[1]);
    int m = 2, ni = 0;
    while (m < kTreelet) {
        int pick = -1;
        for (int k = 0; k < m; k++)
            if (rb_is_interior(r, t.sL[k]) && (pick < 0 || t.larea[k] > t.larea[pick])) pick = k;
        if (pick < 0) break;
        const int e = t.sL[pick];
        was = ni == 0 ? t.larea[pick] : was + t.larea[pick];
        t.sI[ni++] = e;
        const int2 ec = r.child[e];
        for (int k = 0; k < 6; k++) { t.lbox[pick][k] = r.box[(size_t)ec.x * 6 + k]; t.lbox[m][k] = r.box[(size_t)ec.y * 6 + k]; }
        t.sL[pick] = ec.x; t.sL[m] = ec.y;
        t.larea[pick] = box_area(t.lbox[pick]); t.larea[m] = box_area(t.lbox[m]);
        m++;
    }
    for (int k = 0; k < m; k++) t.sh[1 << k] = (uint8_t)r.hcur[t.sL[k]];
    t.sm = m;
    return hv;
}

// The wave.  Areas of all subsets, then the cheapest partition of each by rounds of subset size.
__device__ __forceinline__ void ro_cheapest(Treelet& t, int m, int lane)
{
    const int full = (1 << m) - 1;
    for (int S = lane; S <= full; S += kOptBlock) {
        if (S == 0) continue;
        float b[6];
        subset_box(S, m, t.lbox, b);
        t.sa[S] = box_area(b);
        if ((S & (S - 1)) == 0) t.sc[S] = 0.f;
    }
    __syncthreads();
    for (int size = 2; size <= m; size++) {
        for (int S = lane; S <= full; S += kOptBlock) {
            if (__popc(S) != size) continue;
            const int low = S & -S, rest = S ^ low;
            int bp = low, sub = (0 - rest) & rest;
            float best = t.sc[low] + t.sc[rest];
            while (sub != rest) {      // P = low | sub ascends with sub; a later P only where strictly cheaper
                const int P = low | sub;
                const float cand = t.sc[P] + t.sc[S ^ P];
                if (cand < best) { best = cand; bp = P; }
                sub = (sub - rest) & rest;
            }
            t.spart[S] = (uint8_t)bp;
            t.sc[S] = (S == full ? 0.f : t.sa[S]) + best;
            const int h0 = t.sh[bp], h1 = t.sh[S ^ bp];
            t.sh[S] = (uint8_t)(1 + (h0 > h1 ? h0 : h1));
        }
        __syncthreads();
    }
}

// Lane 0.  Accepted where cheaper, and no deeper than the budget (or than the tree was) allows; then rewired in pre-order, the nodes of
// I handed out as the subsets of two or more entries are met.  Returns whether v's treelet was restructured.
__device__ __forceinline__ bool ro_rewire(const RbDev& r, Treelet& t, int v, int m, int hv, float was)
{
    const int full = (1 << m) - 1;
    const int room = (r.h_lim >= 0 ? r.h_lim : r.levels[kLvDepth]) - r.depth[v];
    if (!(t.sc[full] < was && (int)t.sh[full] <= (hv > room ? hv : room))) return false;
    int sp = 0, nxt = 0;
    t.stS[0] = full; t.stP[0] = -1; t.stSide[0] = 0; sp = 1;
    while (sp > 0) {
        sp--;
        const int S = t.stS[sp], pid = t.stP[sp], side = t.stSide[sp];
        const bool single = (S & (S - 1)) == 0;
        const int node = single ? t.sL[31 - __clz(S)] : pid < 0 ? v : t.sI[nxt++];
        if (pid >= 0) {
            reinterpret_cast<int32_t*>(&r.child[pid])[side] = node;
            r.parent[node] = pid;
        }
        if (single) continue;
        r.hcur[node] = t.sh[S];
        if (pid >= 0) {
            float b[6];
            subset_box(S, m, t.lbox, b);
            for (int k = 0; k < 6; k++) r.box[(size_t)node * 6 + k] = b[k];
        }
        const int P = t.spart[S];
        t.stS[sp] = S ^ P; t.stP[sp] = node; t.stSide[sp] = 1; sp++;
        t.stS[sp] = P; t.stP[sp] = node; t.stSide[sp] = 0; sp++;
    }
    return true;
}

__global__ __launch_bounds__(kOptBlock) void ro_solve(RbDev r, int level)
{
    static_assert(kOptBlock == 64 && (1 << kTreelet) == 2 * kOptBlock, "the subsets of a treelet are dealt two per lane of one wave64");
    __shared__ Treelet t;
    const int lane = threadIdx.x;
    const int first = r.lvl[level], last = r.lvl[level + 1];
    int roots = 0, done = 0;
    for (int idx = first + (int)blockIdx.x; idx < last; idx += (int)gridDim.x) {
        __syncthreads();      // the treelet before is done with the shared arrays
        const int v = r.qsorted[idx];
        int hv = 0;
        float was = 0.f;
        if (lane == 0) hv = ro_form(r, t, v, was);
        __syncthreads();
        const int m = t.sm;
        if (m < 3) continue;
        ro_cheapest(t, m, lane);
        if (lane == 0) {      // the other lanes go on to the barrier at the top of the loop: every barrier is reached by the whole workgroup
            roots++;
            done += ro_rewire(r, t, v, m, hv, was) ? 1 : 0;
        }
    }
    if (lane == 0) {      // counts: they decide no index
        if (roots) atomicAdd(&r.levels[kLvRoots], roots);
        if (done) atomicAdd(&r.levels[kLvRestructured], done);
    }
}

inline unsigned blocks_of(int n) { return (unsigned)((n + 255) / 256); }

// ---- rocPRIM: the temporary storage of the largest call of a build, and of the sort over all 64 key bits where that asks for more
// (sizes only: nothing is launched with a null storage pointer).  temp64 = 0: `temp` serves that sort too.
hipError_t rocprim_temp_bytes(int n, size_t& temp, size_t& temp64)
{
    const int N = 2 * n - 1;
    size_t b[4] = {};
    hipError_t e = rocprim::radix_sort_keys(nullptr, b[0], (uint64_t*)nullptr, (uint64_t*)nullptr, n, 0, 62);
    if (e == hipSuccess) e = rocprim::radix_sort_pairs(nullptr, b[1], (uint32_t*)nullptr, (uint32_t*)nullptr, (int32_t*)nullptr, (int32_t*)nullptr, N, 0, 8);
    if (e == hipSuccess) e = rocprim::exclusive_scan(nullptr, b[2], (int32_t*)nullptr, (int32_t*)nullptr, 0, N, rocprim::plus<int32_t>());
    if (e == hipSuccess) e = rocprim::radix_sort_keys(nullptr, b[3], (uint64_t*)nullptr, (uint64_t*)nullptr, n, 0, 64);
    temp = b[0] > b[1] ? (b[0] > b[2] ? b[0] : b[2]) : (b[1] > b[2] ? b[1] : b[2]);
    temp64 = b[3] > temp ? b[3] : 0;
    return e;
}

// A rocPRIM call with its temporary storage: the size is an in/out argument, so every call gets a copy of it.
struct RbTemp { void* p; size_t bytes; };
template <class Call> hipError_t with_temp(RbTemp t, Call call) { return call(t.p, t.bytes); }

// key_in (written by `keys`, one thread per item) sorted with a payload, and the level offsets of the sorted keys into `levels`
hipError_t rb_sort_levels(void (*keys)(RbDev), const RbDev& r, RbTemp temp, int count, int32_t* payload, int32_t* sorted_payload, int32_t* levels, hipStream_t st)
{
    hipLaunchKernelGGL(keys, dim3(blocks_of(count)), dim3(256), 0, st, r);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess)
        e = with_temp(temp, [&](void* p, size_t& b) { return rocprim::radix_sort_pairs(p, b, r.key_in, r.key_out, payload, sorted_payload, count, 0, 8, st); });
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(rb_level_start, dim3(blocks_of(count)), dim3(256), 0, st, r.key_out, count, levels);
    return hipGetLastError();
}

// The depth of every raw node, after the radix tree over `sorted_keys` where that is not NULL.  Every call of a build but its first
// counts the deepest level anew (the first finds the words as the build's memset left them).
hipError_t rb_depths(RbDev r, uint64_t* sorted_keys, bool first, hipStream_t st)
{
    const int n = r.n;
    if (!first) {
        const hipError_t e = hipMemsetAsync(r.levels + kLvDepth, 0, 4, st);
        if (e != hipSuccess) return e;
    }
    if (sorted_keys) {
        r.sorted = sorted_keys;
        hipLaunchKernelGGL(rb_karras, dim3(blocks_of(n - 1)), dim3(256), 0, st, r);
    }
    hipLaunchKernelGGL(rb_depth, dim3(blocks_of(2 * n - 1)), dim3(256), 0, st, r);
    return hipGetLastError();
}

}  // namespace

static_assert(ptd::kCoreBlocks == 256, "reduce_partials reads one partial per thread of a 256-thread block");

// What this call needs and no earlier one allocated (the table's third kind of column).  On a scene's first rebuild also: the arrays
// and maps whose record count a rebuild may change move into buffers of worst-case size (2 n - 1 builder nodes, n - 1 `nodes` and
// `quad` records) with their contents.  All of it is built beside the scene and moved in only once every allocation exists (as
// pt_dyn_prepare does); only the first rebuild waits, for its copies.
static int rb_prepare(PtScene* s, int needs, hipStream_t st)
{
    const bool first = !s->rb_ready;
    const size_t n = (size_t)s->dyn.n_tris, N = 2 * n - 1, I = n > 1 ? n - 1 : 1;
    size_t temp_bytes = s->rb_temp_bytes, temp64_bytes = s->rb_temp64_bytes;
    if (first) HIPCHK(rocprim_temp_bytes((int)n, temp_bytes, temp64_bytes));
#define X(T, name, count, need) {(size_t)(count) * sizeof(T), need},
    const struct { size_t bytes; int need; } plan[kRbSlots] = {RB_WORKSPACE(X)};
#undef X
    struct { DevBuf* live; size_t bytes; } grow[] = {
        {&s->arr[kArrNodes], I * 64}, {&s->arr[kArrQuad], I * 64}, {&s->dyn_buf[kDynBn], N * 16}, {&s->dyn_buf[kDynOrder], N * 4},
        {&s->dyn_buf[kDynWideBn], I * 8}, {&s->dyn_buf[kDynQuadBn], I * 16}, {&s->dyn_buf[kDynBbox], N * 32},
        {&s->dyn_buf[kDynAreaPartial], ((N + kAreaBlock - 1) / kAreaBlock) * 8}};
    constexpr int kGrow = (int)(sizeof(grow) / sizeof(grow[0]));
    DevBuf fresh[kGrow], mine[kRbSlots];
    int64_t bytes = 0;
    for (int k = 0; first && k < kGrow; k++) {
        HIPCHK(fresh[k].alloc(grow[k].bytes));
        bytes += (int64_t)fresh[k].held() - (int64_t)grow[k].live->held();
        if (grow[k].live->bytes()) HIPCHK(hipMemcpyAsync(fresh[k].as<>(), grow[k].live->as<>(), grow[k].live->bytes(), hipMemcpyDeviceToDevice, st));
    }
    for (int k = 0; k < kRbSlots; k++) {
        if (!(plan[k].need & needs) || !plan[k].bytes || (!first && s->rb_buf[k])) continue;
        HIPCHK(mine[k].alloc(plan[k].bytes));
        bytes += (int64_t)mine[k].held();
    }
    if (first) {
        HIPCHK(hipStreamSynchronize(st));      // the copies are done, and so is whatever the stream still read from the old blocks
        for (int k = 0; k < kGrow; k++) *grow[k].live = std::move(fresh[k]);      // the old blocks are freed with `fresh`
        s->rb_buf.resize(kRbSlots);
    }
    for (int k = 0; k < kRbSlots; k++) if (mine[k]) s->rb_buf[k] = std::move(mine[k]);
    s->bytes += bytes;
    if (!first) return PT_OK;
    s->rb_temp_bytes = temp_bytes; s->rb_temp64_bytes = temp64_bytes;
    ptd::DynScene& d = s->dyn;
    s->dev.nodes = d.nodes = s->arr[kArrNodes].as<float4>(); s->dev.quad = d.quad = s->arr[kArrQuad].as<uint4>();
    d.bn = s->dyn_buf[kDynBn].as<const int4>(); d.order = s->dyn_buf[kDynOrder].as<const int32_t>(); d.wide_bn = s->dyn_buf[kDynWideBn].as<const int2>();
    d.quad_bn = s->dyn_buf[kDynQuadBn].as<const int4>(); d.bbox = s->dyn_buf[kDynBbox].as<float4>(); d.area_partial = s->dyn_buf[kDynAreaPartial].as<double>();
    // prim -> reference leaf: the assignment defines the result and never changes
    RbDev r{};
    r.prim_leaf = s->rb_buf[kRb_prim_leaf].as<int32_t>();
    hipLaunchKernelGGL(rb_prim_leaf, dim3(blocks_of(d.n_leaves)), dim3(256), 0, st, d, r);
    HIPCHK(hipGetLastError());
    s->rb_ready = true;
    return PT_OK;
}

static RbDev rb_args(const PtScene* s, const RbParams& p)
{
    RbDev r;
#define X(T, name, count, need) r.name = s->rb_buf[kRb_##name].as<T>();
    RB_WORKSPACE(X)
#undef X
    r.n = s->dyn.n_tris;
    r.large_fraction = p.large_fraction;
    r.h_lim = p.depth_budget > 0 ? p.depth_budget - 1 : -1;
    return r;
}

// Enqueues the whole build of the topology into the staging buffers.  Nothing a render reads is written.
static int rb_build(const PtScene* s, const RbDev& r, const RbParams& p, hipStream_t st)
{
    const int n = r.n, N = 2 * n - 1;
    const float* pos = s->dyn_buf[kDynPos].as<const float>();
    const RbTemp temp{r.temp, s->rb_temp_bytes};
    const bool classes = p.large_fraction > 0.f;
    HIPCHK(hipMemsetAsync(r.levels, 0, (size_t)kLvWords * 4, st));      // the counts are summed, and the deepest level is raised, from here on
    hipLaunchKernelGGL(rb_box_partial, dim3(ptd::kCoreBlocks), dim3(256), 0, st, r, pos);
    hipLaunchKernelGGL(rb_box_final, dim3(1), dim3(256), 0, st, r);
    if (classes) {      // a centroid box per size class; the class is bit 62 of the key
        hipLaunchKernelGGL(rb_class_partial, dim3(ptd::kCoreBlocks), dim3(256), 0, st, r, pos);
        hipLaunchKernelGGL(rb_class_final, dim3(1), dim3(256), 0, st, r);
    }
    void (*const keys)(RbDev, const float*) = classes ? rb_keys<true> : rb_keys<false>;
    hipLaunchKernelGGL(keys, dim3(blocks_of(n)), dim3(256), 0, st, r, pos);
    HIPCHK(hipGetLastError());
    HIPCHK(with_temp(classes && r.temp64 ? RbTemp{r.temp64, s->rb_temp64_bytes} : temp,
                     [&](void* t, size_t& b) { return rocprim::radix_sort_keys(t, b, r.keys, r.sorted, n, 0, classes ? 64 : 62, st); }));
    hipLaunchKernelGGL(rb_tmap, dim3(blocks_of(n)), dim3(256), 0, st, r);
    if (n <= 2) {
        hipLaunchKernelGGL(rb_single, dim3(1), dim3(64), 0, st, r);
        HIPCHK(hipGetLastError());
        return PT_OK;
    }
    HIPCHK(rb_depths(r, r.sorted, /*first=*/true, st));
    if (p.depth_budget > 0) {      // flatten what would be deeper than the budget, then the tree over the new keys (they are in `keys`)
        hipLaunchKernelGGL(rb_rekey, dim3(blocks_of(n)), dim3(256), 0, st, r, p.depth_budget);
        HIPCHK(hipGetLastError());
        HIPCHK(rb_depths(r, r.keys, false, st));
    }
    if (p.passes > 0) {      // treelet restructuring: per pass the heights, the interior nodes by height, one launch per height, the depths anew
        const int top = p.depth_budget > 0 ? p.depth_budget - 1 : 63;      // no interior node is higher: the tree keeps the budget, and a radix tree over unique keys of at most 63 significant bits is at most 63 deep
        hipLaunchKernelGGL(ro_init, dim3(blocks_of(N)), dim3(256), 0, st, r, pos);
        for (int pass = 0; pass < p.passes; pass++) {
            hipLaunchKernelGGL(rb_height, dim3(blocks_of(N)), dim3(256), 0, st, r);
            HIPCHK(rb_sort_levels(ro_keys, r, temp, n - 1, r.iota, r.qsorted, r.lvl, st));
            for (int h = 1; h <= top; h++) hipLaunchKernelGGL(ro_solve, dim3(kOptGrid), dim3(kOptBlock), 0, st, r, h);
            HIPCHK(hipGetLastError());
            HIPCHK(rb_depths(r, nullptr, false, st));
        }
    }
    hipLaunchKernelGGL(rb_height, dim3(blocks_of(N)), dim3(256), 0, st, r);
    HIPCHK(hipGetLastError());
    // numbering: builder nodes and `nodes` records by rank, `order` by height, `quad` records by level
    HIPCHK(with_temp(temp, [&](void* t, size_t& b) { return rocprim::exclusive_scan(t, b, r.live, r.newid, 0, N, rocprim::plus<int32_t>(), st); }));
    HIPCHK(with_temp(temp, [&](void* t, size_t& b) { return rocprim::exclusive_scan(t, b, r.wflag, r.widx, 0, n - 1, rocprim::plus<int32_t>(), st); }));
    HIPCHK(rb_sort_levels(rb_height_keys, r, temp, N, r.newid, r.order, r.levels + kLvOrder, st));
    HIPCHK(rb_sort_levels(rb_level_keys, r, temp, n - 1, r.iota, r.qsorted, r.levels + kLvQuad, st));
    hipLaunchKernelGGL(rb_qidx, dim3(blocks_of(n - 1)), dim3(256), 0, st, r);
    hipLaunchKernelGGL(rb_emit, dim3(blocks_of(N)), dim3(256), 0, st, r);
    HIPCHK(hipGetLastError());
    return PT_OK;
}

// The numbers of a built topology, from the words.
struct RbTree { int32_t lv[kLvWords]; int n_bn, n_wide, n_quad, top, depth, quad_depth; };

// Wait 1: the words come back, the report is filled, and the tree is checked against the kernels' stack limits.  Nothing a render, a
// query or an update reads has been written when this refuses.
static int rb_read_back(const char* who, const RbDev& r, hipStream_t st, RbReport& report, RbTree& t)
{
    HIPCHK(hipMemcpyAsync(t.lv, r.levels, sizeof(t.lv), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    report = {t.lv[kLvLarge], t.lv[kLvFlattened], t.lv[kLvRoots], t.lv[kLvRestructured], true};
    t.n_bn = t.lv[kLvOrder + kDead]; t.n_quad = t.lv[kLvQuad + kDead]; t.n_wide = t.n_bn > 1 ? (t.n_bn - 1) / 2 : 1;
    t.top = t.quad_depth = 0;
    while (t.lv[kLvOrder + t.top + 1] < t.n_bn) t.top++;                    // heights 0 .. top
    while (t.lv[kLvQuad + t.quad_depth + 1] < t.n_quad) t.quad_depth++;      // levels 0 .. quad_depth
    t.depth = t.lv[kLvDepth];
    return pt_tree_limits(who, t.depth, t.quad_depth);
}

// The commit: the staged maps and refs go into the scene, the vertex update's kernels write the boxes, and wait 2 brings the new
// denominator of pt_scene_tree_inflation.
static int rb_commit(PtScene* s, const RbDev& r, const RbTree& t, hipStream_t st)
{
    ptd::DynScene& d = s->dyn;
    const struct { int dst; const void* src; size_t bytes; } maps[] = {{kDynBn, r.bn, (size_t)t.n_bn * 16}, {kDynOrder, r.order, (size_t)t.n_bn * 4}, {kDynWideBn, r.wide_bn, (size_t)t.n_wide * 8},
                                                                        {kDynQuadBn, r.quad_bn, (size_t)t.n_quad * 16}, {kDynTmap, r.tmap, (size_t)d.n_tris * 8}};
    for (const auto& m : maps) HIPCHK(hipMemcpyAsync(s->dyn_buf[m.dst].as<>(), m.src, m.bytes, hipMemcpyDeviceToDevice, st));
    d.n_bn = t.n_bn; d.n_wide = t.n_wide; d.n_quad = t.n_quad;
    s->dev.n_nodes = t.n_wide; s->dev.n_quad = t.n_quad; s->dev.quad_depth = t.quad_depth;
    s->max_depth = t.depth;
    s->dyn_host.level_start.assign(t.lv + kLvOrder, t.lv + kLvOrder + t.top + 2);
    hipLaunchKernelGGL(rb_refs, dim3(blocks_of(t.n_wide > t.n_quad ? t.n_wide : t.n_quad)), dim3(256), 0, st, d, r);
    HIPCHK(hipGetLastError());
    // tri, tripair, every box of `nodes`, origin / scales / quantised boxes of `quad`, from the scene's own positions
    HIPCHK(pt_dyn_launch_update(d, s->dyn_buf[kDynPos].as<const float>(), nullptr, nullptr, s->dyn_host.level_start.data(), t.top + 1, /*trees_only=*/true, st));
    // wait 2: by the same reduction in the same order as at upload
    s->h_area.assign(((size_t)t.n_bn + kAreaBlock - 1) / kAreaBlock, 0.0);
    HIPCHK(pt_dyn_launch_area(d, st));
    HIPCHK(hipMemcpyAsync(s->h_area.data(), d.area_partial, s->h_area.size() * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    double sum = 0.0;
    for (double v : s->h_area) sum += v;
    s->dyn_host.area_sum = sum;
    s->rebuilds++;
    return PT_OK;
}

// The rebuild behind the three entry points, which have checked p.
static int rb_run(PtScene* s, const char* who, const RbParams& p, RbReport& report, hipStream_t st)
{
    HIPCHK(hipSetDevice(s->device));
    int rc;
    if ((rc = pt_dyn_prepare(s)) != PT_OK) return rc;
    if ((rc = rb_prepare(s, kAlways | (p.large_fraction > 0.f ? kClasses : 0) | (p.passes > 0 ? kPasses : 0), st)) != PT_OK) return rc;
    const RbDev r = rb_args(s, p);
    RbTree t;
    if ((rc = rb_build(s, r, p, st)) != PT_OK || (rc = rb_read_back(who, r, st, report, t)) != PT_OK) return rc;
    return rb_commit(s, r, t, st);
}

extern "C" {

int pt_scene_rebuild_tree(PtScene* s, void* hip_stream)
{
    if (!s) { pt_set_error("pt_scene_rebuild_tree: NULL scene"); return PT_ERR_INVALID; }
    RbReport rep{};
    return rb_run(s, "pt_scene_rebuild_tree", RbParams{0, 0.f, 0}, rep, (hipStream_t)hip_stream);
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
    RbReport rep{};
    rc = rb_run(s, who, RbParams{p->depth_budget, p->large_fraction, 0}, rep, (hipStream_t)hip_stream);
    if (report && rep.known) { report->n_large = rep.n_large; report->n_flattened_tris = rep.n_flattened_tris; }
    return rc;
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
    RbReport rep{};
    rc = rb_run(s, who, RbParams{p->depth_budget, p->large_fraction, passes}, rep, (hipStream_t)hip_stream);
    if (report && rep.known) { report->n_large = rep.n_large; report->n_flattened_tris = rep.n_flattened_tris; report->n_roots = rep.n_roots; report->n_restructured = rep.n_restructured; }
    return rc;
}

}  // extern "C"
