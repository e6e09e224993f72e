// pt_lists.hip — the two pieces of the variable-length query lists that need no scene (include/pt_api.h: pt_list_offsets; DESIGN.md
// section 37): the int64 exclusive scan that turns counts into CSR offsets, and the sort of the segments the fill appended to.
//
// Scan: three launches and no waiting between workgroups — per-span sums over a grid of at most kScanGrid workgroups, one workgroup
// scanning those kScanGrid partials in the caller's scratch, then a rescan of every span from its base.  A span is a whole number of
// kScanChunk chunks.  Integer sums: the result depends on the counts alone, whatever the order.
// Sort: pt_lists.h's for_each_segment; a segment of up to kListShort slots is sorted by insertion by its own thread, a longer one by the
// bitonic network of the whole workgroup, without recursion and without allocating: tiles of kSortTile records in LDS for the stages
// and steps inside a tile, global memory for the steps between tiles, barriers between steps (the workgroup's threads read what others
// of the same workgroup wrote: one CU, __syncthreads() orders it).
#include <hip/hip_runtime.h>
#include "pt_internal.h"
#include "pt_lists.h"

namespace ptd {

// tests/lists_ref.py holds SCAN_CHUNK, SCAN_GRID and SORT_TILE, the boundaries its cases sit on; tests/test_lists.py reads these lines
// and fails when the two disagree.
constexpr int kScanThreads = 256;
constexpr int kScanPer = 8;                                   // counts per thread in a chunk, consecutive
constexpr uint64_t kScanChunk = kScanThreads * kScanPer;       // 2,048
constexpr uint32_t kScanGrid = 256;                            // the most workgroups, and partials: 2 KB of scratch
constexpr int kSortTile = 2 * kSegThreads;                     // 512 records, 4 KB of LDS: two per thread, one pair per thread and step

// Exclusive scan of one int64 per thread over the kScanThreads threads; `total` receives the sum.  Every thread must call it.
PT_DEV int64_t block_exclusive_scan(int64_t v, int64_t* lds, int64_t& total)
{
    const int tid = threadIdx.x;
    lds[tid] = v;
    __syncthreads();
    for (int d = 1; d < kScanThreads; d <<= 1) {
        const int64_t add = tid >= d ? lds[tid - d] : 0;
        __syncthreads();
        lds[tid] += add;
        __syncthreads();
    }
    total = lds[kScanThreads - 1];
    const int64_t incl = lds[tid];
    __syncthreads();      // the caller may reuse lds
    return incl - v;
}

PT_DEV int64_t count_at(const int32_t* __restrict__ count, uint64_t i) { const int32_t c = count[i]; return c > 0 ? c : 0; }

__global__ __launch_bounds__(kScanThreads)
void scan_partials(const int32_t* __restrict__ count, uint64_t n, uint64_t span, int64_t* __restrict__ part)
{
    __shared__ int64_t lds[kScanThreads];
    const uint64_t lo = (uint64_t)blockIdx.x * span, hi = (n - lo < span) ? n : lo + span;
    int64_t s = 0;
    for (uint64_t i = lo + threadIdx.x; i < hi; i += kScanThreads) s += count_at(count, i);
    int64_t total;
    (void)block_exclusive_scan(s, lds, total);
    if (threadIdx.x == 0) part[blockIdx.x] = total;
}

// One workgroup: the partials of `blocks` spans become their bases, in place, and offsets[n] the total
__global__ __launch_bounds__(kScanThreads)
void scan_spine(int64_t* __restrict__ part, uint32_t blocks, uint64_t n, int64_t* __restrict__ offsets)
{
    __shared__ int64_t lds[kScanThreads];
    const uint32_t tid = threadIdx.x;
    const int64_t v = tid < blocks ? part[tid] : 0;
    int64_t total;
    const int64_t base = block_exclusive_scan(v, lds, total);
    if (tid < blocks) part[tid] = base;
    if (tid == 0) offsets[n] = total;
}

__global__ __launch_bounds__(kScanThreads)
void scan_apply(const int32_t* __restrict__ count, uint64_t n, uint64_t span, const int64_t* __restrict__ part, int64_t* __restrict__ offsets)
{
    __shared__ int64_t lds[kScanThreads];
    const uint64_t lo = (uint64_t)blockIdx.x * span, hi = (n - lo < span) ? n : lo + span;
    int64_t base = part[blockIdx.x];
    for (uint64_t c0 = lo; c0 < hi; c0 += kScanChunk) {
        const uint64_t first = c0 + (uint64_t)threadIdx.x * kScanPer;
        int64_t v[kScanPer], s = 0;
#pragma unroll
        for (int j = 0; j < kScanPer; j++) {
            v[j] = first + j < hi ? count_at(count, first + j) : 0;
            s += v[j];
        }
        int64_t total;
        int64_t run = base + block_exclusive_scan(s, lds, total);
#pragma unroll
        for (int j = 0; j < kScanPer; j++) {
            if (first + j < hi) offsets[first + j] = run;
            run += v[j];
        }
        base += total;
    }
}

// ---- the sort ----
template <bool FKEY>
PT_DEV void cswap(int2* a, int2* b)
{
    const int2 x = *a, y = *b;
    if (list_before<FKEY>(y, x)) { *a = y; *b = x; }
}

// Pair q of a step of the network: the lower index i (a zero inserted at bit log2(h)) and its partner, i ^ (2h - 1) on the first step
// of a stage (the "flip", which lets every comparator put the smaller record at the lower index) or i + h on the others
PT_DEV void bitonic_pair(int64_t q, int64_t h, bool flip, int64_t& i, int64_t& p)
{
    i = ((q & ~(h - 1)) << 1) | (q & (h - 1));
    p = flip ? (i ^ (2 * h - 1)) : i + h;
}

// The records [t0, t0 + kSortTile) of a segment of m through LDS: loaded (a position at or past m holds a miss record, which is never
// moved towards a lower index and never written back — the same as comparing with a virtual +inf, so that any m works), then every
// stage of the network up to kSortTile (whole) or the steps below kSortTile of one stage (!whole), then stored.
template <bool FKEY>
PT_DEV void sort_tile(int2* __restrict__ seg, int64_t m, int64_t t0, int2* lds, bool whole)
{
    const int tid = threadIdx.x;
    for (int r = tid; r < kSortTile; r += kSegThreads) lds[r] = t0 + r < m ? seg[t0 + r] : make_int2(0, -1);
    __syncthreads();
    for (int k = whole ? 2 : kSortTile; k <= kSortTile; k <<= 1) {
        for (int h = k / 2; h >= 1; h >>= 1) {
            int64_t i, p;
            bitonic_pair(tid, h, whole && h == k / 2, i, p);
            cswap<FKEY>(&lds[i], &lds[p]);
            __syncthreads();
        }
    }
    for (int r = tid; r < kSortTile; r += kSegThreads)
        if (t0 + r < m) seg[t0 + r] = lds[r];
    __syncthreads();      // lds is loaded again by the next tile
}

// A segment of m > kListShort records, by the whole workgroup.  Network of N = the power of two >= m; comparators with a partner at or
// past m are skipped (a virtual +inf there).  Stages 2 .. kSortTile run inside tiles; each later stage k runs its steps with a stride of
// kSortTile or more over global memory, then the rest inside tiles.
template <bool FKEY>
PT_DEV void sort_long(int2* __restrict__ seg, int64_t m, int2* lds)
{
    for (int64_t t0 = 0; t0 < m; t0 += kSortTile) sort_tile<FKEY>(seg, m, t0, lds, true);
    int64_t N = kSortTile;
    while (N < m) N <<= 1;
    for (int64_t k = 2 * kSortTile; k <= N; k <<= 1) {
        for (int64_t h = k / 2; h >= kSortTile; h >>= 1) {
            for (int64_t q = threadIdx.x; q < N / 2; q += kSegThreads) {
                int64_t i, p;
                bitonic_pair(q, h, h == k / 2, i, p);
                if (p < m) cswap<FKEY>(&seg[i], &seg[p]);
            }
            __syncthreads();
        }
        for (int64_t t0 = 0; t0 < m; t0 += kSortTile) sort_tile<FKEY>(seg, m, t0, lds, false);
    }
}

// Insertion sort by one thread, for kListLds < m <= kListShort
template <bool FKEY>
PT_DEV void sort_short(int2* __restrict__ seg, int64_t m)
{
    for (int64_t j = 1; j < m; j++) {
        const int2 x = seg[j];
        int64_t k = j;
        for (; k > 0; k--) {
            const int2 y = seg[k - 1];
            if (!list_before<FKEY>(x, y)) break;
            seg[k] = y;
        }
        seg[k] = x;
    }
}

template <bool FKEY>
__global__ __launch_bounds__(kSegThreads)
void list_sort(const int64_t* __restrict__ off, uint32_t n, uint32_t per, int64_t cap, int2* __restrict__ rec)
{
    __shared__ int2 lds[kSortTile];
    for_each_segment(off, n, per, cap,
                     [&](uint32_t, int64_t b, int64_t e) { if (e - b > kListLds) sort_short<FKEY>(rec + b, e - b); },
                     [&](uint32_t, int64_t b, int64_t e) { sort_long<FKEY>(rec + b, e - b, lds); });
}

}  // namespace ptd

hipError_t ptk_list_sort(const int64_t* off, uint32_t n, int64_t cap, int2* rec, bool floatKey, hipStream_t stream)
{
    uint32_t per, blocks;
    pt_list_grid(n, per, blocks);
    if (floatKey) hipLaunchKernelGGL((ptd::list_sort<true>), dim3(blocks), dim3(ptd::kSegThreads), 0, stream, off, n, per, cap, rec);
    else hipLaunchKernelGGL((ptd::list_sort<false>), dim3(blocks), dim3(ptd::kSegThreads), 0, stream, off, n, per, cap, rec);
    return hipGetLastError();
}

extern "C" {

int64_t pt_list_offsets_scratch_bytes(int64_t n)
{
    if (n < 0) return -1;
    return n == 0 ? 0 : (int64_t)ptd::kScanGrid * 8;
}

int pt_list_offsets(const int32_t* d_count, int64_t n, int64_t* d_offsets, void* d_scratch, void* hip_stream)
{
    const char* bad = !d_count ? "NULL count" : !d_offsets ? "NULL offsets" : n < 0 ? "n < 0" : (n > 0 && !d_scratch) ? "NULL scratch" :
                      ((uintptr_t)d_count & 3) ? "count must be 4-byte aligned" : ((uintptr_t)d_offsets & 7) ? "offsets must be 8-byte aligned" :
                      ((uintptr_t)d_scratch & 7) ? "scratch must be 8-byte aligned" : nullptr;
    if (bad) { pt_set_error("pt_list_offsets: %s", bad); return PT_ERR_INVALID; }
    const hipStream_t stream = (hipStream_t)hip_stream;
    if (n == 0) {
        HIPCHK(hipMemsetAsync(d_offsets, 0, 8, stream));
        return PT_OK;
    }
    const uint64_t nn = (uint64_t)n, chunks = (nn + ptd::kScanChunk - 1) / ptd::kScanChunk;
    const uint64_t span = (chunks + ptd::kScanGrid - 1) / ptd::kScanGrid * ptd::kScanChunk;
    const uint32_t blocks = (uint32_t)((nn + span - 1) / span);      // <= kScanGrid
    int64_t* part = (int64_t*)d_scratch;
    hipLaunchKernelGGL(ptd::scan_partials, dim3(blocks), dim3(ptd::kScanThreads), 0, stream, d_count, nn, span, part);
    hipLaunchKernelGGL(ptd::scan_spine, dim3(1), dim3(ptd::kScanThreads), 0, stream, part, blocks, nn, d_offsets);
    hipLaunchKernelGGL(ptd::scan_apply, dim3(blocks), dim3(ptd::kScanThreads), 0, stream, d_count, nn, span, (const int64_t*)part, d_offsets);
    HIPCHK(hipGetLastError());
    return PT_OK;
}

// The neutral filter of the _f queries (include/pt_api.h: "Query filters")
void pt_query_filter_default(PtQueryFilter* f)
{
    if (!f) return;
    f->d_prim_bits = nullptr;
    f->d_query_bits = nullptr;
    f->d_skip_prim = nullptr;
    f->bits = 0xFFFFFFFFu;
    f->flags = 0u;
}

}  // extern "C"
