// pt_lists.h — what the sorted query results share (include/pt_api.h: pt_trace_rays_k, pt_nearest_k, pt_list_offsets, pt_trace_rays_list,
// pt_within_radius_list; DESIGN.md sections 30, 34 and 37): the order of the records, the per-lane LDS list of the K kernels and of the
// fill, the fill's sink and its write-out, the clamped segment of a query, the pass over the segments that hands a short one to one
// thread and a long one to the whole workgroup, the detail kernels' body over it, and the launcher of the sort (pt_lists.hip).
// And the query filters (section 40): the wrapper that puts any of these sinks behind a filter, and the one-slot sink of the filtered
// closest and any forms.
//
// Which code sorts a segment of m slots:
//   m <= kListLds          the fill keeps it sorted in the K kernels' per-lane LDS list, with that lane's k = m
//   kListLds < m <= kListShort   the fill appends, list_sort's thread of that query sorts it in place (insertion)
//   m > kListShort         the fill appends, list_sort's whole workgroup sorts it (bitonic: LDS tiles, global steps between them)
#pragma once
#include <hip/hip_runtime.h>
#include "pt_device.h"
#include "pt_math.h"
#include "../../include/pt_api.h"

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
    static constexpr bool kStops = false;       // a walk need not ask done(): the sink wants candidates to the end
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

// The count of the members of a point query's C(p) or a box query's B(Q): the bound stays what it was set to (r2; a box's class bound).
// counts(): its acceptance, and the fill's for a long segment (SlotSeg).
struct KCount {
    static constexpr bool kOrdered = false;     // every child within r2 is visited whatever the order
    static constexpr bool kStops = false;
    int cnt;
    float bound;
    PT_DEV static bool counts(float f, float bound) { return f <= bound; }
    PT_DEV void offer(float f, int) { cnt += counts(f, bound) ? 1 : 0; }
    PT_DEV bool wants(float f, int) const { return counts(f, bound); }      // the two halves of offer(), for pt_lists.h's Filtered
    PT_DEV void take(float, int) { cnt++; }
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

// ---- query filters (include/pt_api.h: "Query filters") --------------------------------------------------------
// A filtered query answers over H' = the members of its twin's set H that the filter keeps, a pure selection.  The whole correctness
// argument: a sink's bound is only ever moved by take(), and Filtered calls the inner take() for members of H' alone — A FILTERED-OUT
// PRIMITIVE NEVER TIGHTENS A BOUND.  So the inner sink sees exactly the walk of a scene that holds H' only, with a bound that is at
// every moment the bound of that walk: whatever the walks' culls prove for H they prove for H'.  The inner sink's own test comes
// first — registers only —, so that only a candidate the sink would take pays the filter's one 4-byte gather.
//
// The filter as a kernel takes it (by value): the three arrays of PtQueryFilter, each null or a device pointer, already advanced to
// the launch's first query where they are per query.
struct QFilter {
    const uint32_t* prim_bits;      // per primitive; null: every bit set
    const uint32_t* query_bits;     // per query; null: `bits`
    const int32_t* skip;            // per query; null: none
    uint32_t bits;
    uint32_t tmin;                  // PT_FILTER_TMIN given: the ray's 7th float is its near bound
};

// One query's filter, in registers.  skip = -1 and tmin = -inf keep everything: no primitive has number -1, no key is below -inf.
struct LaneFilter {
    const uint32_t* prim_bits;
    uint32_t m;
    int skip;
    float tmin;
    // skip, tmin, then the gather; a null prim_bits costs no load (the pointer is uniform: a scalar branch)
    PT_DEV bool keeps(float key, int prim) const
    {
        if (prim == skip) return false;
        if (key < tmin) return false;
        if (!prim_bits) return m != 0u;
        return (prim_bits[prim] & m) != 0u;
    }
};

// Query i's filter.  tmin: the ray's near bound as read by the caller (ignored unless f.tmin).
PT_DEV LaneFilter lane_filter(const QFilter& f, uint32_t i, float tmin)
{
    LaneFilter l;
    l.prim_bits = f.prim_bits;
    l.m = f.query_bits ? f.query_bits[i] : f.bits;
    l.skip = f.skip ? f.skip[i] : -1;
    l.tmin = f.tmin ? tmin : -__builtin_inff();
    return l;
}

// Any sink behind a filter: wants() and offer() are the inner sink's test, then the filter's; take(), bound and kOrdered are the inner
// sink's.  SINK has wants() and take() (a point walk's offer() is the two in a row).
template <class SINK>
struct Filtered : SINK {
    LaneFilter f;
    PT_DEV bool wants(float key, int prim) const { return SINK::wants(key, prim) && f.keeps(key, prim); }
    PT_DEV void offer(float key, int prim)
    {
        if (wants(key, prim)) SINK::take(key, prim);
    }
};

// The sink of the filtered closest and any forms: one slot of SlotList's rule, in registers, no LDS list.  Empty: (bound, boundPrim) =
// (tmax or r2, -1), (key, prim) = (0, -1), the miss record.  ANY: after the first member nothing is wanted any more — bound 0 and the
// largest prim fail both halves of the rule for every key >= 0 —, and the sink says so: kStops makes the walks ask done() before they
// take the next node off their stack (a compile-time choice: a walk over any other sink has no such test).
template <bool ANY>
struct SlotOne {
    static constexpr bool kOrdered = true;
    static constexpr bool kStops = ANY;
    PT_DEV bool done() const { return ANY && prim >= 0; }
    float bound;
    int boundPrim;
    float key;
    int prim;
    PT_DEV bool wants(float k, int p) const { return (k < bound) | ((k == bound) & (p > boundPrim)); }
    PT_DEV void take(float k, int p)
    {
        key = k;
        prim = p;
        bound = ANY ? 0.f : k;
        boundPrim = ANY ? 0x7fffffff : p;
    }
};

// The end of a K kernel: the wave's lists, padded with miss records by their lanes, go out of LDS in record order — record r of the
// block is slot r % k of query r / k —, 64 consecutive records (512 bytes) per store.  base: the wave's first query; the __syncthreads
// between the lanes' last list writes and these reads is the caller's.
PT_DEV void klist_copy_out(const int2* lds_list, int2* __restrict__ out, uint32_t base, uint32_t n, int k)
{
    const uint32_t lane = threadIdx.x;
    const uint32_t live = (n - base < 64u) ? n - base : 64u, total = live * (uint32_t)k;
    int2* dst = out + (size_t)base * (size_t)k;
    const int q64 = 64 / k, m64 = 64 % k;
    int t = (int)lane / k, j = (int)lane % k;      // record r is slot j of query t: r = t * k + j, t < live <= 64
    for (uint32_t r = lane; r < total; r += 64u) {
        dst[r] = lds_list[j * kSlotRow + t];
        j += m64;
        t += q64;
        if (j >= k) { j -= k; t++; }
    }
}

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

// A launch's filter from the caller's (checked by pt_query_args; null: the neutral one), for the batch whose first query is `first`
inline ptd::QFilter pt_filter_dev(const PtQueryFilter* f, int64_t first)
{
    if (!f) return ptd::QFilter{nullptr, nullptr, nullptr, 0xFFFFFFFFu, 0u};
    return ptd::QFilter{f->d_prim_bits, f->d_query_bits ? f->d_query_bits + first : nullptr, f->d_skip_prim ? f->d_skip_prim + first : nullptr, f->bits,
                        f->flags & PT_FILTER_TMIN};
}

// Does the filter keep every member of every query?  Then a _f entry point enqueues its twin's own kernels.
inline bool pt_filter_neutral(const PtQueryFilter* f)
{
    return !f || (!f->d_prim_bits && !f->d_query_bits && !f->d_skip_prim && f->bits == 0xFFFFFFFFu && f->flags == 0u);
}

// pt_lists.hip: enqueues the sort of every segment of more than kListLds slots of the n (<= 2^30) queries whose n + 1 offsets start at
// `off` (clamped to cap), records at `rec`.  floatKey: t (the ray lists), else f (the point lists).
hipError_t ptk_list_sort(const int64_t* off, uint32_t n, int64_t cap, int2* rec, bool floatKey, hipStream_t stream);
// pt_rayhits.hip / pt_knearest.hip: enqueue the filtered closest (or `any`) form for n <= 2^30 queries, (key, prim) per query, for
// pt_query.hip's pt_trace_rays_f and pt_nearest.hip's pt_closest_points_f, whose surface and detail kernels live in those files
hipError_t ptk_rays_one_f(const ptd::DevScene& sc, const float* d_rays8, uint32_t n, bool any, bool quad, const ptd::QFilter& flt, PtRayHit* d_hits,
                          hipStream_t stream);
hipError_t ptk_near_one_f(const ptd::DevScene& sc, const float* d_points4, uint32_t n, bool any, bool quad, const ptd::QFilter& flt, PtNearest* d_out,
                          hipStream_t stream);
