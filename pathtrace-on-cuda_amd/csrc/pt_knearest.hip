// pt_knearest.hip — the K nearest primitives within a radius, sorted, and the number of primitives within a radius, for the caller's points
// on an uploaded scene (include/pt_api.h: pt_nearest_k, pt_count_within).  DESIGN.md section 30.
//
// Both are DEFINED without a tree, over C(p) = { k : f(p, k) <= r2 } with the f of pt_nearest.h: the first K members of C in the order
// (f ascending, among equal f the larger index first), and |C|.  The walks only have to find them, by the inequality of section 29,
// f(p, k) >= boxdist2(p, box of k) >= boxdist2(p, any box that contains it), exact in float32: a child whose boxdist2 exceeds the bound
// holds no member that could enter.  The bound is r2 while the list holds fewer than K, then the f of its last slot (it only ever
// decreases); for the count it is r2 throughout.  What the closest query did not need: every triangle sits below exactly ONE leaf of
// the tree walked — a list would hold a triangle met twice in two slots, a count would count it twice.
//
// Shape: nearest_points' (pt_nearest.hip) — one point per lane, one-wave workgroups, the per-lane LDS stack of (bound, ref) entries with
// entry e at stack[e * 64].  Beside it the per-lane candidate list, sorted, slot j at list[j * kListRow + lane] as int2 (f's bits, prim):
// squared distances are >= 0, so their bits order as ints.  The count and the bound live in registers.
#include <hip/hip_runtime.h>
#include "pt_device.h"
#include "pt_math.h"
#include "pt_trace.h"
#include "pt_scene.h"
#include "pt_nearest.h"
#include "pt_lists.h"

namespace ptd {

// int2 entries from one slot of the list to the next: 64 lanes and one of padding.  The walk reads and writes a slot with consecutive
// lanes on consecutive entries either way; the padding is for the copy-out, which reads the list transposed (consecutive lanes read
// consecutive SLOTS of one point): at 64 those fall on one bank, k ways; at 65 slot j of point t sits in bank pair (j + t) mod 32.
constexpr int kListRow = 65;

// What a walk hands its candidates to.  `bound`: a child box farther than this holds nothing the sink would take.
// The list of the K nearest.  (bound, boundPrim) is (r2, -1) while cnt < k and slot k - 1 from then on, so that ONE rule accepts:
// f < bound, or f == bound and a larger index — with fewer than k that is f <= r2, with k it is "precedes the last slot".  A NaN f
// passes neither comparison.  Every slot index is at most min(cnt, k - 1) <= k - 1, and the kernel has checked k <= KC.
struct KList {
    static constexpr bool kOrdered = true;      // visit the nearer child first: the bound falls sooner
    int2* list;                                 // this lane's slot 0
    int k, cnt;
    float bound;
    int boundPrim;
    PT_DEV void take(float f, int prim)
    {
        if (!((f < bound) | ((f == bound) & (prim > boundPrim)))) return;
        const int fb = __float_as_int(f);
        int j = (cnt < k) ? cnt : k - 1;        // the slot that opens: the next free one, or the last, whose candidate drops out
        while (j > 0) {                         // shift from the tail until the slot before precedes the candidate
            const int2 e = list[(j - 1) * kListRow];
            if ((e.x < fb) | ((e.x == fb) & (e.y > prim))) break;
            list[j * kListRow] = e;
            j--;
        }
        list[j * kListRow] = make_int2(fb, prim);
        cnt += (cnt < k) ? 1 : 0;
        if (cnt == k) {
            const int2 last = list[(k - 1) * kListRow];
            bound = __int_as_float(last.x);
            boundPrim = last.y;
        }
    }
};

// The count of C(p): the bound stays r2
struct KCount {
    static constexpr bool kOrdered = false;     // every child within r2 is visited whatever the order
    int cnt;
    float bound;
    PT_DEV void take(float f, int) { cnt += (f <= bound) ? 1 : 0; }
};

// The `cnt` triangles at tree position `first` (a leaf of either tree: ~ref = first << 3 | cnt)
template <class SINK>
PT_DEV void knear_leaf(const DevScene& sc, int ref, const f3& p, SINK& s)
{
    const int code = ~ref, first = code >> 3, cnt = code & 7;
    for (int k = 0; k < cnt; k++) {
        const float4* rec = sc.tri + 3 * (size_t)(first + k);
        const float4 a = rec[0], b = rec[1], c = rec[2];
        s.take(tri_f(p, f3(a.x, a.y, a.z), f3(b.x, b.y, b.z), f3(c.x, c.y, c.z)), __float_as_int(a.w));
    }
}

// The walk over the 4-wide quantised tree: near_walk_quad's (pt_nearest.hip) against the sink's bound.  A node pushes at most three of
// its children and descends into the fourth, a leaf pushes nothing: at most 3 entries per level (the caller has checked
// 3 * quad_depth + 2 <= kQueryStack), and the walk ends whatever the floats are.  An ordered sink takes the nearest child next and
// pushes the others farthest first; an unordered one takes them as they come.
template <class SINK>
PT_DEV void knear_walk_quad(const DevScene& sc, const f3& p, int2* stack, SINK& s)
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
                key[k] = ((ref[k] == -1) | (lb > s.bound)) ? kQuadMiss : __float_as_int(lb);      // strictly: an equal bound may hide a tie that enters
            }
            if constexpr (SINK::kOrdered) {
                int k0 = key[0], k1 = key[1], k2 = key[2], k3 = key[3], r0 = ref[0], r1 = ref[1], r2 = ref[2], r3 = ref[3];
#define PT_CE(ka, ra, kb, rb) { const bool sw = ka > kb; const int tk = sw ? kb : ka, tr = sw ? rb : ra; kb = sw ? ka : kb; rb = sw ? ra : rb; ka = tk; ra = tr; }
                PT_CE(k0, r0, k1, r1) PT_CE(k2, r2, k3, r3) PT_CE(k0, r0, k2, r2) PT_CE(k1, r1, k3, r3) PT_CE(k1, r1, k2, r2)
#undef PT_CE
                if (k0 != kQuadMiss) {
                    if (k3 != kQuadMiss) { stack[sp * 64] = make_int2(k3, r3); sp++; }
                    if (k2 != kQuadMiss) { stack[sp * 64] = make_int2(k2, r2); sp++; }
                    if (k1 != kQuadMiss) { stack[sp * 64] = make_int2(k1, r1); sp++; }
                    cur = r0;
                    continue;
                }
            } else {
                bool have = false;
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    if (key[k] == kQuadMiss) continue;
                    if (have) { stack[sp * 64] = make_int2(key[k], ref[k]); sp++; }
                    else { cur = ref[k]; have = true; }
                }
                if (have) continue;
            }
        } else {
            knear_leaf(sc, cur, p, s);
        }
        if (!near_pop(stack, sp, s.bound, cur)) return;
    }
}

// The walk over the binary tree, for a scene whose 4-wide walk would not fit kQueryStack (or PTAMD_QUERY_QUAD=0): near_walk_binary's.
// A leaf child is evaluated on the spot and an entry is pushed only where both children are interior: at most depth - 1 <= 31 entries.
template <class SINK>
PT_DEV void knear_walk_binary(const DevScene& sc, const f3& p, int2* stack, SINK& s)
{
    int cur = 0, sp = 0;
    for (;;) {
        const float4 q0 = sc.nodes[4 * (size_t)cur + 0], q1 = sc.nodes[4 * (size_t)cur + 1], q2 = sc.nodes[4 * (size_t)cur + 2], q3 = sc.nodes[4 * (size_t)cur + 3];
        f3 loL(q0.x, q0.y, q0.z), hiL(q0.w, q1.x, q1.y), loR(q1.z, q1.w, q2.x), hiR(q2.y, q2.z, q2.w);
        widen_binary(loL, hiL);
        widen_binary(loR, hiR);
        const float lbL = boxdist2(p, loL, hiL), lbR = boxdist2(p, loR, hiR);
        const int refL = __float_as_int(q3.x), refR = __float_as_int(q3.y);
        if (refL < 0 && !(lbL > s.bound)) knear_leaf(sc, refL, p, s);
        if (refR < 0 && !(lbR > s.bound)) knear_leaf(sc, refR, p, s);
        const bool okL = (refL >= 0) & !(lbL > s.bound), okR = (refR >= 0) & !(lbR > s.bound);      // against what the leaves left
        if (okL & okR) {
            const bool lNear = !SINK::kOrdered || lbL <= lbR;
            stack[sp * 64] = lNear ? make_int2(__float_as_int(lbR), refR) : make_int2(__float_as_int(lbL), refL);
            sp++;
            cur = lNear ? refL : refR;
        } else if (okL) {
            cur = refL;
        } else if (okR) {
            cur = refR;
        } else if (!near_pop(stack, sp, s.bound, cur)) {
            return;
        }
    }
}

template <bool QUAD, class SINK>
PT_DEV void knear_point(const DevScene& sc, const float4& q, int2* stack, SINK& s)
{
    const f3 p(q.x, q.y, q.z);
    if (QUAD) knear_walk_quad(sc, p, stack, s);
    else knear_walk_binary(sc, p, stack, s);
    for (int j = 0; j < sc.n_spheres; j++) s.take(sphere_f(p, sc.spheres[4 * j]), sc.n_tris + j);
}

// KC: the capacity class of the list, the smallest of 4, 8, 16, 32 that holds k (launch_nearest_k), so that k = 2 does not pay the LDS
// of k = 32.  The wave's 64 points own the 64 * k consecutive records from out[blockIdx.x * 64 * k]; every lane pads its list with miss
// records and the wave copies the block out of LDS in record order, 64 consecutive records (512 bytes) per store.
template <int KC, bool QUAD>
__global__ __launch_bounds__(64)
void nearest_k(DevScene sc, const float4* __restrict__ points, uint32_t n, int k, int2* __restrict__ out)
{
    __shared__ int2 lds_stack[(QUAD ? kQueryStack : kStackDepth) * 64];
    __shared__ int2 lds_list[KC * kListRow];
    if (k < 1 || k > KC) return;      // the launcher's choice of KC, restated where the list is indexed
    const uint32_t lane = threadIdx.x, base = blockIdx.x * 64u, i = base + lane;
    int2* list = &lds_list[lane];
    int cnt = 0;
    if (i < n) {
        const float4 q = points[i];
        KList s{list, k, 0, q.w * q.w, -1};
        knear_point<QUAD>(sc, q, &lds_stack[lane], s);
        cnt = s.cnt;
    }
    for (int j = cnt; j < k; j++) list[j * kListRow] = make_int2(0, -1);      // a miss is (0, -1)
    __syncthreads();
    const uint32_t live = (n - base < 64u) ? n - base : 64u, total = live * (uint32_t)k;
    int2* dst = out + (size_t)base * (size_t)k;
    const int q64 = 64 / k, m64 = 64 % k;
    int t = (int)lane / k, j = (int)lane % k;      // record r is slot j of point t: r = t * k + j, t < live <= 64
    for (uint32_t r = lane; r < total; r += 64u) {
        dst[r] = lds_list[j * kListRow + t];
        j += m64;
        t += q64;
        if (j >= k) { j -= k; t++; }
    }
}

template <bool QUAD>
__global__ __launch_bounds__(64)
void count_within(DevScene sc, const float4* __restrict__ points, uint32_t n, int32_t* __restrict__ out)
{
    __shared__ int2 lds_stack[(QUAD ? kQueryStack : kStackDepth) * 64];
    const uint32_t i = blockIdx.x * 64u + threadIdx.x;
    if (i >= n) return;
    const float4 q = points[i];
    KCount s{0, q.w * q.w};
    knear_point<QUAD>(sc, q, &lds_stack[threadIdx.x], s);
    out[i] = s.cnt;
}

// The 8-float detail record of the header for every finished slot, one thread per slot; zeros for a miss slot.  Slot t belongs to point t / k.
// A launch covers the slots from `first` on (launch_nearest_k: at most kDetailSlots of them, so that no grid exceeds 2^31 threads).
__global__ __launch_bounds__(256)
void nearest_k_detail(DevScene sc, const float4* __restrict__ points, uint64_t first, uint64_t slots, uint32_t k, const int2* __restrict__ res, float* __restrict__ out8)
{
    const uint64_t t = first + (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (t >= slots) return;
    const int prim = res[t].y;
    float* o = out8 + t * 8;
    if (prim < 0) { for (int c = 0; c < 8; c++) o[c] = 0.f; return; }
    near_detail(sc, points[t / k], prim, o);
}

// ---- every primitive within the radius: the fill of pt_within_radius_list (pt_lists.h says which code sorts
// which segment) ----
// The sink of the fill.  A lane owns the segment [b, b + m) of the records.  m <= kListLds: KList itself, over the lane's LDS list with
// k = m; the list goes out sorted after the walk.  m > kListLds: every member of C is appended to the segment in the order the walk
// meets it, while fewer than m are stored, with KCount's bound (r2) and acceptance — so the members appended are the members
// pt_count_within counts —, and ptk_list_sort sorts the segment afterwards.  Ordered: the nearer child first, for the list's sake.
struct KSeg : KList {
    int2* seg;
    int64_t m;
    bool append;
    PT_DEV void take(float f, int prim)
    {
        if (!append) { KList::take(f, prim); return; }
        if ((f <= bound) & (cnt < m)) { seg[cnt] = make_int2(__float_as_int(f), prim); cnt++; }
    }
};

// One point per lane, nearest_k's shape with the list of class kListLds.  A lane whose segment is empty walks nothing.  Every record of
// the segment is written once, by its lane: the members, then the miss record (0, -1) up to m.  Nothing outside [0, cap) is written.
template <bool QUAD>
__global__ __launch_bounds__(64)
void near_list(DevScene sc, const float4* __restrict__ points, uint32_t n, const int64_t* __restrict__ off, int64_t cap, int2* __restrict__ out)
{
    __shared__ int2 lds_stack[(QUAD ? kQueryStack : kStackDepth) * 64];
    __shared__ int2 lds_list[kListLds * kListRow];
    const uint32_t lane = threadIdx.x, i = blockIdx.x * 64u + lane;
    if (i >= n) return;
    int64_t b, e;
    list_segment(off, i, cap, b, e);
    const int64_t m = e - b;
    if (m == 0) return;
    const float4 q = points[i];
    int2* list = &lds_list[lane];
    int2* dst = out + b;
    KSeg s;
    s.list = list; s.k = m > kListLds ? 0 : (int)m; s.cnt = 0; s.bound = q.w * q.w; s.boundPrim = -1;
    s.seg = dst; s.m = m; s.append = m > kListLds;
    knear_point<QUAD>(sc, q, &lds_stack[lane], s);
    int64_t j = 0;
    if (!s.append)
        for (; j < s.cnt; j++) dst[j] = list[j * kListRow];
    else
        j = s.cnt;
    for (; j < m; j++) dst[j] = make_int2(0, -1);
}

// The detail records of every segment, after the sort: near_detail per member slot, zeros per miss slot.  A short segment by its query's
// thread, a long one by the whole workgroup (pt_lists.h: for_each_segment).
__global__ __launch_bounds__(kSegThreads)
void near_list_detail(DevScene sc, const float4* __restrict__ points, uint32_t n, uint32_t per, const int64_t* __restrict__ off, int64_t cap,
                      const int2* __restrict__ res, float* __restrict__ out8)
{
    auto slot = [&](const float4& q, int64_t t) {
        const int prim = res[t].y;
        float* o = out8 + t * 8;
        if (prim < 0) { for (int c = 0; c < 8; c++) o[c] = 0.f; return; }
        near_detail(sc, q, prim, o);
    };
    for_each_segment(off, n, per, cap,
                     [&](uint32_t i, int64_t b, int64_t e) {
                         const float4 q = points[i];
                         for (int64_t t = b; t < e; t++) slot(q, t);
                     },
                     [&](uint32_t i, int64_t b, int64_t e) {
                         const float4 q = points[i];
                         for (int64_t t = b + threadIdx.x; t < e; t += kSegThreads) slot(q, t);
                     });
}

}  // namespace ptd

template <int KC>
static void launch_nearest_kc(const ptd::DevScene& sc, const float4* pts, uint32_t n, int k, bool quad, int2* out, hipStream_t stream)
{
    const dim3 blocks((n + 63u) / 64u);
    if (quad) hipLaunchKernelGGL((ptd::nearest_k<KC, true>), blocks, dim3(64), 0, stream, sc, pts, n, k, out);
    else hipLaunchKernelGGL((ptd::nearest_k<KC, false>), blocks, dim3(64), 0, stream, sc, pts, n, k, out);
}

static const uint64_t kDetailSlots = (uint64_t)1 << 31;      // slots per launch of nearest_k_detail (a multiple of its 256 threads)

// Enqueues one batch of n <= 2^30 points on `stream`: k records per point, then the detail records if asked for
static hipError_t launch_nearest_k(const ptd::DevScene& sc, const float* d_points4, uint32_t n, int k, bool quad, PtNearest* d_out, float* d_detail8, hipStream_t stream)
{
    const float4* pts = (const float4*)d_points4;
    int2* out = (int2*)d_out;
    if (k <= 4) launch_nearest_kc<4>(sc, pts, n, k, quad, out, stream);
    else if (k <= 8) launch_nearest_kc<8>(sc, pts, n, k, quad, out, stream);
    else if (k <= 16) launch_nearest_kc<16>(sc, pts, n, k, quad, out, stream);
    else launch_nearest_kc<32>(sc, pts, n, k, quad, out, stream);
    if (d_detail8) {      // 2^30 points are up to 2^35 slots: several launches, each of at most 2^31 threads
        const uint64_t slots = (uint64_t)n * (uint64_t)k;
        for (uint64_t first = 0; first < slots; first += kDetailSlots) {
            const uint64_t m = slots - first < kDetailSlots ? slots - first : kDetailSlots;
            hipLaunchKernelGGL(ptd::nearest_k_detail, dim3((uint32_t)((m + 255u) / 256u)), dim3(256), 0, stream, sc, pts, first, slots, (uint32_t)k, (const int2*)out, d_detail8);
        }
    }
    return hipGetLastError();
}

static hipError_t launch_count_within(const ptd::DevScene& sc, const float* d_points4, uint32_t n, bool quad, int32_t* d_count, hipStream_t stream)
{
    const dim3 blocks((n + 63u) / 64u);
    if (quad) hipLaunchKernelGGL((ptd::count_within<true>), blocks, dim3(64), 0, stream, sc, (const float4*)d_points4, n, d_count);
    else hipLaunchKernelGGL((ptd::count_within<false>), blocks, dim3(64), 0, stream, sc, (const float4*)d_points4, n, d_count);
    return hipGetLastError();
}

// Enqueues one batch of n <= 2^30 points of pt_within_radius_list on `stream`: the fill, the sort of the segments longer than kListLds,
// then the detail records if asked for.  off: the batch's first offset; the records are addressed from d_out whatever the batch.
static hipError_t launch_near_list(const ptd::DevScene& sc, const float* d_points4, uint32_t n, bool quad, const int64_t* off, int64_t cap,
                                   PtNearest* d_out, float* d_detail8, hipStream_t stream)
{
    const dim3 blocks((n + 63u) / 64u);
    const float4* pts = (const float4*)d_points4;
    int2* out = (int2*)d_out;
    if (quad) hipLaunchKernelGGL((ptd::near_list<true>), blocks, dim3(64), 0, stream, sc, pts, n, off, cap, out);
    else hipLaunchKernelGGL((ptd::near_list<false>), blocks, dim3(64), 0, stream, sc, pts, n, off, cap, out);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    if ((e = ptk_list_sort(off, n, cap, out, false, stream)) != hipSuccess) return e;
    if (d_detail8) {
        uint32_t per, grid;
        pt_list_grid(n, per, grid);
        hipLaunchKernelGGL(ptd::near_list_detail, dim3(grid), dim3(ptd::kSegThreads), 0, stream, sc, pts, n, per, off, cap, (const int2*)out, d_detail8);
    }
    return hipGetLastError();
}

// ---- entry points (include/pt_api.h): every argument check comes before the first HIP call ----------------------------------------
// out_align: 8 for PtNearest records, 4 for counts.  has_k: pt_nearest_k and its host variant.
static int knear_args_ok(const char* who, const PtScene* s, const float* points, int64_t n, bool has_k, int32_t k, const void* out, int out_align,
                         const float* detail, bool device)
{
    const char* bad = !s ? "NULL scene" : !points ? "NULL points" : !out ? "NULL out" : n < 0 ? "n < 0" :
                      (has_k && (k < 1 || k > PT_NEAREST_KMAX)) ? "k must be in 1 .. PT_NEAREST_KMAX" :
                      (device && ((uintptr_t)points & 15)) ? "points must be 16-byte aligned" :
                      (device && ((uintptr_t)out & (uintptr_t)(out_align - 1))) ? (out_align == 8 ? "out must be 8-byte aligned" : "count must be 4-byte aligned") :
                      (device && ((uintptr_t)detail & 3)) ? "detail must be 4-byte aligned" : nullptr;
    if (bad) { pt_set_error("%s: %s", who, bad); return PT_ERR_INVALID; }
    return PT_OK;
}

// pt_within_radius_list and its host variant.  device: the pointers are device pointers (alignment checked, out required); on the host
// variant out may be NULL (the sizing call).
static int near_list_args_ok(const char* who, const PtScene* s, const float* points, int64_t n, const int64_t* offsets, int64_t cap,
                             const void* out, const float* detail, bool device)
{
    const char* bad = !s ? "NULL scene" : !points ? "NULL points" : !offsets ? "NULL offsets" : (device && !out) ? "NULL out" : n < 0 ? "n < 0" :
                      cap < 0 ? "cap < 0" :
                      (device && ((uintptr_t)points & 15)) ? "points must be 16-byte aligned" :
                      (device && ((uintptr_t)offsets & 7)) ? "offsets must be 8-byte aligned" :
                      (device && ((uintptr_t)out & 7)) ? "out must be 8-byte aligned" :
                      (device && ((uintptr_t)detail & 3)) ? "detail must be 4-byte aligned" : nullptr;
    if (bad) { pt_set_error("%s: %s", who, bad); return PT_ERR_INVALID; }
    return PT_OK;
}

static const int64_t kKnearBatch = (int64_t)1 << 30;      // points per launch: point numbers are 32-bit

extern "C" {

int pt_nearest_k(PtScene* s, const float* d_points4, int64_t n, int32_t k, PtNearest* d_out, float* d_detail8, void* hip_stream)
{
    int rc;
    if ((rc = knear_args_ok("pt_nearest_k", s, d_points4, n, true, k, d_out, 8, d_detail8, true)) != PT_OK) return rc;
    if (n == 0) return PT_OK;
    HIPCHK(hipSetDevice(s->device));
    const bool quad = pt_query_walks_quad(s);
    for (int64_t off = 0; off < n; off += kKnearBatch) {
        const uint32_t m = (uint32_t)(n - off < kKnearBatch ? n - off : kKnearBatch);
        HIPCHK(launch_nearest_k(s->dev, d_points4 + off * 4, m, k, quad, d_out + off * k, d_detail8 ? d_detail8 + off * k * 8 : nullptr, (hipStream_t)hip_stream));
    }
    return PT_OK;
}

int pt_nearest_k_host(PtScene* s, const float* h_points4, int64_t n, int32_t k, PtNearest* h_out, float* h_detail8)
{
    int rc;
    if ((rc = knear_args_ok("pt_nearest_k_host", s, h_points4, n, true, k, h_out, 8, h_detail8, false)) != PT_OK) return rc;
    if (n == 0) return PT_OK;
    HIPCHK(hipSetDevice(s->device));
    const size_t slots = (size_t)n * (size_t)k;
    DevBuf d_pts, d_out, d_det;      // d_det stays null when the caller asked for no detail records
    HIPCHK(d_pts.alloc((size_t)n * 16));
    HIPCHK(d_out.alloc(slots * 8));
    if (h_detail8) HIPCHK(d_det.alloc(slots * 32));
    HIPCHK(hipMemcpy(d_pts.as<>(), h_points4, (size_t)n * 16, hipMemcpyHostToDevice));
    if ((rc = pt_nearest_k(s, d_pts.as<float>(), n, k, d_out.as<PtNearest>(), d_det.as<float>(), nullptr)) != PT_OK) return rc;
    HIPCHK(hipStreamSynchronize(nullptr));
    HIPCHK(hipMemcpy(h_out, d_out.as<>(), slots * 8, hipMemcpyDeviceToHost));
    if (h_detail8) HIPCHK(hipMemcpy(h_detail8, d_det.as<>(), slots * 32, hipMemcpyDeviceToHost));
    return PT_OK;
}

int pt_count_within(PtScene* s, const float* d_points4, int64_t n, int32_t* d_count, void* hip_stream)
{
    int rc;
    if ((rc = knear_args_ok("pt_count_within", s, d_points4, n, false, 0, d_count, 4, nullptr, true)) != PT_OK) return rc;
    if (n == 0) return PT_OK;
    HIPCHK(hipSetDevice(s->device));
    const bool quad = pt_query_walks_quad(s);
    for (int64_t off = 0; off < n; off += kKnearBatch) {
        const uint32_t m = (uint32_t)(n - off < kKnearBatch ? n - off : kKnearBatch);
        HIPCHK(launch_count_within(s->dev, d_points4 + off * 4, m, quad, d_count + off, (hipStream_t)hip_stream));
    }
    return PT_OK;
}

int pt_count_within_host(PtScene* s, const float* h_points4, int64_t n, int32_t* h_count)
{
    int rc;
    if ((rc = knear_args_ok("pt_count_within_host", s, h_points4, n, false, 0, h_count, 4, nullptr, false)) != PT_OK) return rc;
    if (n == 0) return PT_OK;
    HIPCHK(hipSetDevice(s->device));
    DevBuf d_pts, d_count;
    HIPCHK(d_pts.alloc((size_t)n * 16));
    HIPCHK(d_count.alloc((size_t)n * 4));
    HIPCHK(hipMemcpy(d_pts.as<>(), h_points4, (size_t)n * 16, hipMemcpyHostToDevice));
    if ((rc = pt_count_within(s, d_pts.as<float>(), n, d_count.as<int32_t>(), nullptr)) != PT_OK) return rc;
    HIPCHK(hipStreamSynchronize(nullptr));
    HIPCHK(hipMemcpy(h_count, d_count.as<>(), (size_t)n * 4, hipMemcpyDeviceToHost));
    return PT_OK;
}

int pt_within_radius_list(PtScene* s, const float* d_points4, int64_t n, const int64_t* d_offsets, int64_t cap, PtNearest* d_out, float* d_detail8,
                          void* hip_stream)
{
    int rc;
    if ((rc = near_list_args_ok("pt_within_radius_list", s, d_points4, n, d_offsets, cap, d_out, d_detail8, true)) != PT_OK) return rc;
    if (n == 0) return PT_OK;
    HIPCHK(hipSetDevice(s->device));
    const bool quad = pt_query_walks_quad(s);
    for (int64_t off = 0; off < n; off += kKnearBatch) {
        const uint32_t m = (uint32_t)(n - off < kKnearBatch ? n - off : kKnearBatch);
        HIPCHK(launch_near_list(s->dev, d_points4 + off * 4, m, quad, d_offsets + off, cap, d_out, d_detail8, (hipStream_t)hip_stream));
    }
    return PT_OK;
}

int pt_within_radius_list_host(PtScene* s, const float* h_points4, int64_t n, int64_t* h_offsets, int64_t cap, PtNearest* h_out, float* h_detail8)
{
    int rc;
    if ((rc = near_list_args_ok("pt_within_radius_list_host", s, h_points4, n, h_offsets, cap, h_out, h_detail8, false)) != PT_OK) return rc;
    if (n == 0) { h_offsets[0] = 0; return PT_OK; }
    HIPCHK(hipSetDevice(s->device));
    DevBuf d_pts, d_count, d_off, d_scratch, d_out, d_det;      // d_det stays null when the caller asked for no detail records
    HIPCHK(d_pts.alloc((size_t)n * 16));
    HIPCHK(d_count.alloc((size_t)n * 4));
    HIPCHK(d_off.alloc((size_t)(n + 1) * 8));
    HIPCHK(d_scratch.alloc((size_t)pt_list_offsets_scratch_bytes(n)));
    HIPCHK(hipMemcpy(d_pts.as<>(), h_points4, (size_t)n * 16, hipMemcpyHostToDevice));
    if ((rc = pt_count_within(s, d_pts.as<float>(), n, d_count.as<int32_t>(), nullptr)) != PT_OK) return rc;
    if ((rc = pt_list_offsets(d_count.as<int32_t>(), n, d_off.as<int64_t>(), d_scratch.as<>(), nullptr)) != PT_OK) return rc;
    HIPCHK(hipStreamSynchronize(nullptr));
    HIPCHK(hipMemcpy(h_offsets, d_off.as<>(), (size_t)(n + 1) * 8, hipMemcpyDeviceToHost));
    if (!h_out) return PT_OK;      // the sizing call
    const int64_t total = h_offsets[n];
    if (cap < total) { pt_set_error("pt_within_radius_list_host: cap %lld < %lld records", (long long)cap, (long long)total); return PT_ERR_INVALID; }
    HIPCHK(d_out.alloc((size_t)total * 8));
    if (h_detail8) HIPCHK(d_det.alloc((size_t)total * 32));
    if ((rc = pt_within_radius_list(s, d_pts.as<float>(), n, d_off.as<int64_t>(), total, d_out.as<PtNearest>(), d_det.as<float>(), nullptr)) != PT_OK)
        return rc;
    HIPCHK(hipStreamSynchronize(nullptr));
    HIPCHK(hipMemcpy(h_out, d_out.as<>(), (size_t)total * 8, hipMemcpyDeviceToHost));
    if (h_detail8) HIPCHK(hipMemcpy(h_detail8, d_det.as<>(), (size_t)total * 32, hipMemcpyDeviceToHost));
    return PT_OK;
}

}  // extern "C"
