// pt_lists.h — what the variable-length query lists share (include/pt_api.h: pt_list_offsets, pt_trace_rays_list,
// pt_within_radius_list): the clamped segment of a query, the order of the records in a segment, the pass over the
// segments that hands a short one to one thread and a long one to the whole workgroup, and the launcher of the sort (pt_lists.hip).
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

// Does record a (key's bits, prim) strictly precede record b in a list?  Members (prim >= 0) by key ascending, among equal keys the
// larger prim first; a miss record (prim < 0) precedes nothing and every member precedes it, so misses go last.  FKEY: the key is t,
// compared as a float (-0 equals +0); else f >= 0, whose bits order as ints (pt_knearest.hip's comparison).  No two members compare
// equal (the header's order is total), and two misses are the same bits: every correct sort gives the same array.
template <bool FKEY>
PT_DEV bool list_before(int2 a, int2 b)
{
    if (a.y < 0) return false;
    if (b.y < 0) return true;
    if (FKEY) {
        const float x = __int_as_float(a.x), y = __int_as_float(b.x);
        return (x < y) | ((x == y) & (a.y > b.y));
    }
    return (a.x < b.x) | ((a.x == b.x) & (a.y > b.y));
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
