// pt_lists.h — what the sorted query results share (include/pt_api.h: pt_trace_rays_k, pt_nearest_k, pt_list_offsets, pt_trace_rays_list,
// pt_within_radius_list; DESIGN.md sections 30, 34 and 37): the order of the records, the per-lane LDS list of the K kernels and of the
// fill, the fill's sink and its write-out, the clamped segment of a query, the pass over the segments that hands a short one to one
// thread and a long one to the whole workgroup, the detail kernels' body over it, and the launcher of the sort (pt_lists.hip).
//
// Which code sorts a segment of m slots:
//   m <= kListLds          the fill keeps it sorted in the K kernels' per-lane LDS list, with that lane's k = m
//   kListLds < m <= kListShort   the fill appends, list_sort's thread of that query sorts it in place (insertion)
//   m > kListShort         the fill appends, list_sort's whole workgroup sorts it (bitonic: LDS tiles, global steps between them)
#pragma once
#include <hip/hip_runtime.h>
#include "pt_device.h"
#include "pt_math.h"

namespace ptd {

constexpr int kListLds = 8;             // slots of the fill's per-lane LDS list (the K kernels' capacity class 8: 4,160 B a wave)
constexpr int kListShort = 32;          // the longest segment one thread handles after the fill (PT_RAY_HITS_KMAX)
constexpr int kSegThreads = 256;        // threads of a workgroup that walks the segments (list_sort, the detail kernels)
constexpr uint32_t kSegGrid = 4096;     // at most this many of those workgroups

// The segment [b, e) of query i: b = clamp(off[i], 0, cap), e = clamp(off[i + 1], b, cap).  Whatever the offsets hold, 0 <= b <= e <= cap.
PT_DEV void list_segment(const int64_t* __restrict__ off, uint64_t i, int64_t cap, int64_t& b, int64_t& e)
{
    int64_t lo = off[i], hi = off[i + 1];
    lo = lo < 0 ? 0 : (lo > cap ? cap : lo);
    hi = hi < lo ? lo : (hi > cap ? cap : hi);
    b = lo;
    e = hi;
}

// The order of the records (key's bits, prim) of a list, the one statement of it: does member a strictly precede member b?  Key
// ascending, among equal keys the larger prim first.  FKEY: the key is t, compared as a float (-0 equals +0); else f >= 0, whose bits
// order as ints.  The list's insertion shift, list_before and list_sort's comparators all compare with it.
template <bool FKEY>
PT_DEV bool slot_before(int2 a, int2 b)
{
    if (FKEY) {
        const float x = __int_as_float(a.x), y = __int_as_float(b.x);
        return (x < y) | ((x == y) & (a.y > b.y));
    }
    return (a.x < b.x) | ((a.x == b.x) & (a.y > b.y));
}

// slot_before over every record: a miss record (prim < 0) precedes nothing and every member precedes it, so misses go last.  No two
// members compare equal (the header's order is total), and two misses are the same bits: every correct sort gives the same array.
template <bool FKEY>
PT_DEV bool list_before(int2 a, int2 b)
{
    if (a.y < 0) return false;
    if (b.y < 0) return true;
    return slot_before<FKEY>(a, b);
}

// int2 entries from one slot of a per-lane LDS list to the next: 64 lanes and one of padding.  A walk reads and writes a slot with
// consecutive lanes on consecutive entries either way; the padding is for the K kernels' copy-out, which reads the list transposed (consecutive
// lanes read consecutive SLOTS of one query): at 64 those fall on one bank, k ways; at 65 slot j of query t sits in bank pair (j + t) mod 32.
constexpr int kSlotRow = 65;

// What a walk hands its candidates to.  A ray walk (pt_rayhits.hip) asks wants(key, prim), the sink's acceptance, and calls
// // take(key, prim) only after a wants() on the sink as it is now; a point walk (pt_nearest.h) calls offer(key, prim), which is both.
// `bound`: a box or child beyond this holds nothing the sink would take.
// The list of the first K of a query, sorted, slot j at list[j * kSlotRow].  (bound, boundPrim) is (tmax or r2, -1) while cnt < k and
// slot k - 1 from then on, so that ONE rule accepts: key < bound, or key == bound and a larger prim — with fewer than k that is
// key <= bound, with k it is "precedes the last slot".  A NaN key passes neither comparison.  Every slot index is at most
// min(cnt, k - 1) <= k - 1, and the kernel has checked k <= its capacity class.
template <bool FKEY>
struct SlotList {
    static constexpr bool kOrdered = true;      // a point walk visits the nearer child first: the bound falls sooner
    int2* list;                                 // this lane's slot 0
    int k, cnt;
    float bound;
    int boundPrim;
    PT_DEV bool wants(float key, int prim) const { return (key < bound) | ((key == bound) & (prim > boundPrim)); }
    PT_DEV void take(float key, int prim)
    {
        const int2 r = make_int2(__float_as_int(key), prim);
        int j = (cnt < k) ? cnt : k - 1;        // the slot that opens: the next free one, or the last, whose record drops out
        while (j > 0) {                         // shift from the tail until the slot before precedes the record
            const int2 e = list[(j - 1) * kSlotRow];
            if (slot_before<FKEY>(e, r)) break;
            list[j * kSlotRow] = e;
            j--;
        }
        list[j * kSlotRow] = r;
        cnt += (cnt < k) ? 1 : 0;
        if (cnt == k) {
            const int2 last = list[(k - 1) * kSlotRow];
            bound = __int_as_float(last.x);
            boundPrim = last.y;
        }
    }
    PT_DEV void offer(float key, int prim)
    {
        if (!wants(key, prim)) return;
        take(key, prim);
    }
};

// The sink of a list fill.  A lane owns the segment [b, b + m) of the records, seg = &out[b].  m <= kListLds:
// SlotList itself, over the lane's LDS list with k = m; the list goes out sorted.  m > kListLds: every member is appended to the segment
// in the order the walk meets it, while fewer than m are stored, with COUNT's acceptance (COUNT::counts(key, bound), the bound staying
// tmax or r2) — so the members appended are the members the matching count counts —, and ptk_list_sort sorts the segment afterwards.
template <bool FKEY, class COUNT>
struct SlotSeg : SlotList<FKEY> {
    int2* seg;
    int64_t m;
    bool append;
    PT_DEV SlotSeg(int2* lane_list, int2* dst, int64_t m_, float bound_)
        : SlotList<FKEY>{lane_list, m_ > kListLds ? 0 : (int)m_, 0, bound_, -1}, seg(dst), m(m_), append(m_ > kListLds) {}
    PT_DEV bool wants(float key, int prim) const { return append ? COUNT::counts(key, this->bound) : SlotList<FKEY>::wants(key, prim); }
    PT_DEV void take(float key, int prim)
    {
        if (!append) { SlotList<FKEY>::take(key, prim); return; }
        if (this->cnt < m) { seg[this->cnt] = make_int2(__float_as_int(key), prim); this->cnt++; }
    }
    PT_DEV void offer(float key, int prim)
    {
        if (!append) { SlotList<FKEY>::offer(key, prim); return; }
        if (COUNT::counts(key, this->bound) & (this->cnt < m)) { seg[this->cnt] = make_int2(__float_as_int(key), prim); this->cnt++; }
    }
};

// The end of a list fill, in the lane that owns the segment dst = &out[b] of m records: every record written once — the lane's list of
// cnt sorted members (slot 0 at list), or the cnt members appended, then the miss record (0, -1) up to m
PT_DEV void fill_write_out(const int2* list, int2* dst, int64_t m, int cnt, bool append)
{
    int64_t j = 0;
    if (!append)
        for (; j < cnt; j++) dst[j] = list[j * kSlotRow];
    else
        j = cnt;
    for (; j < m; j++) dst[j] = make_int2(0, -1);
}

// Every segment of n queries, in a grid of kSegThreads-thread workgroups: workgroup g takes the chunks of `per` consecutive queries
// c = g, g + gridDim.x, ...  In a chunk a query whose segment has 1 .. kListShort slots goes to its own thread, shortf(i, b, e); then the
// longer ones go one after the other to the whole workgroup, longf(i, b, e), called by every thread with the same arguments (it may
// hold barriers).  Which queries are long is exchanged through LDS as one ballot per wave: no atomics.
template <class SHORT, class LONG>
PT_DEV void for_each_segment(const int64_t* __restrict__ off, uint32_t n, uint32_t per, int64_t cap, SHORT shortf, LONG longf)
{
    __shared__ unsigned long long longMask[kSegThreads / 64];
    const uint32_t tid = threadIdx.x, nChunks = (n + per - 1) / per;
    for (uint32_t c = blockIdx.x; c < nChunks; c += gridDim.x) {
        const uint32_t i = c * per + tid;      // c * per < n + per <= 2^30 + 256
        bool isLong = false;
        if (tid < per && i < n) {
            int64_t b, e;
            list_segment(off, i, cap, b, e);
            if (e - b > kListShort) isLong = true;
            else if (e > b) shortf(i, b, e);
        }
        const unsigned long long ballot = __ballot(isLong);
        if ((tid & 63) == 0) longMask[tid >> 6] = ballot;
        __syncthreads();
        for (int w = 0; w < kSegThreads / 64; w++) {
            unsigned long long mask = longMask[w];      // the same value in every thread
            while (mask) {
                const uint32_t j = c * per + (uint32_t)(w * 64 + __builtin_ctzll(mask));
                mask &= mask - 1;
                int64_t b, e;
                list_segment(off, j, cap, b, e);
                longf(j, b, e);
            }
        }
        __syncthreads();      // longMask is rewritten by the next chunk
    }
}

// The body of a list's detail kernel, after the sort: the W-float detail record of every slot of every segment — detail(q, record, o)
// for a member, zeros for a miss —, with q = load(i) the query of the segment.  A short segment by its query's thread, a long one by the
// whole workgroup.
template <int W, class LOAD, class DETAIL>
PT_DEV void segments_detail(const int64_t* __restrict__ off, uint32_t n, uint32_t per, int64_t cap, const int2* __restrict__ res,
                            float* __restrict__ out, LOAD load, DETAIL detail)
{
    auto slot = [&](const auto& q, int64_t t) {
        const int2 h = res[t];
        float* o = out + t * W;
        if (h.y < 0) { for (int c = 0; c < W; c++) o[c] = 0.f; return; }
        detail(q, h, o);
    };
    for_each_segment(off, n, per, cap,
                     [&](uint32_t i, int64_t b, int64_t e) {
                         const auto q = load(i);
                         for (int64_t t = b; t < e; t++) slot(q, t);
                     },
                     [&](uint32_t i, int64_t b, int64_t e) {
                         const auto q = load(i);
                         for (int64_t t = b + threadIdx.x; t < e; t += kSegThreads) slot(q, t);
                     });
}

}  // namespace ptd

// The grid of for_each_segment over n queries: `per` queries per chunk (1 .. kSegThreads), at most kSegGrid workgroups, so that a
// batch of a few thousand long segments still spreads over the whole GPU and 2 M short ones cost 8,192 chunks.
inline void pt_list_grid(uint32_t n, uint32_t& per, uint32_t& blocks)
{
    uint32_t p = (n + ptd::kSegGrid - 1) / ptd::kSegGrid;
    p = p < 1 ? 1 : (p > (uint32_t)ptd::kSegThreads ? (uint32_t)ptd::kSegThreads : p);
    const uint32_t chunks = (n + p - 1) / p;
    per = p;
    blocks = chunks < ptd::kSegGrid ? chunks : ptd::kSegGrid;
}

// pt_lists.hip: enqueues the sort of every segment of more than kListLds slots of the n (<= 2^30) queries whose n + 1 offsets start at
// `off` (clamped to cap), records at `rec`.  floatKey: t (the ray lists), else f (the point lists).
hipError_t ptk_list_sort(const int64_t* off, uint32_t n, int64_t cap, int2* rec, bool floatKey, hipStream_t stream);
