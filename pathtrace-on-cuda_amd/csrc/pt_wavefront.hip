// pt_wavefront.hip — the integrator as a queue-driven pipeline (the default render path).
//
// Why: the one-kernel state machine (pt_kernels.hip, kept as `mode 0`) is issue-bound at
// ~11 % SIMD lane utilisation (profiles/r01_pmc_megakernel_v1.json): rays of very different
// length share a wave, leaf code runs for a few lanes at a time, and the fat shading code
// holds 190 VGPRs (2 waves/SIMD).  Here every (pixel, pass) is a *stream* whose state lives
// in HBM as SoA float4 arrays; each iteration advances every live stream by one step:
//
//   wf_trace  closest hits of all pending path rays and visibility of all pending NEE shadow
//             rays (one queue index space): lean kernel, 7 waves/SIMD, lanes refill from the queue
//   wf_shade  one step of every live stream (pt_stream.h): apply the NEE terms whose shadow rays are back,
//             shade the path hit — and, when that path ends, the first hit of the next sample too
//             (the camera ray's hit is cached) — emit the shadow and path rays, or retire the stream
//             and write its per-pass mean.
//
// The traversal kernel is persistent: a wave takes ray ids from a 16-way sharded queue in
// chunks of <= 128 and, whenever >= 24 of its lanes have finished their ray, hands them new
// ones (ballot + prefix-popcount compaction), so lanes do not idle for the longest ray of the
// wave.  It walks the 4-wide quantised tree (pt_device.h).  Each trip of its loop the wave runs
// ONE of two code paths, a node step or a triangle test; a ray that reaches a leaf parks it and
// keeps walking, so both kinds of trip run fuller.  Rays that exceed a node budget are suspended
// and resumed by the next launch (time slicing).  Shadow rays stop at the first hit that is
// provably in front of the sampled light point (result-neutral, see wf_trace).
// For small renders (one rank of an 8-way tile split, a single full-frame pass) the shade step starts on a second stream beside
// the draining traversal kernel ("early shade", wf_shade PHASE 1 / 2): the launch tail of wf_trace is then not idle time.
//
// Per-stream arithmetic — order of random draws, every float operation — is exactly that of
// render_units / the reference's GetColor_iter, so images are bit-identical across modes.
#include <hip/hip_runtime.h>
#include <cstdlib>
#include <type_traits>
#include "pt_device.h"
#include "pt_math.h"
#include "pt_bxdf.h"
#include "pt_trace.h"
#include "pt_trace_probe.h"
#include "pt_shade.h"
#include "pt_stream.h"
#include "pt_internal.h"

namespace ptd {

constexpr int kWfLdsStack = 16;      // stack entries per lane kept in LDS (4 KB / wave)
constexpr int kWfOvfLevels = 48;     // further levels spill to global memory (never needed on the config scenes: 4-wide depth 12 -> at most 38 entries; tests/test_needle_scene.py renders a scene whose rays do need them)
constexpr int kWfChunk = 128;        // most ray ids a wave takes from a queue shard per atomic (measured optimum 116-229)
constexpr int kDone = (int)0x80000000;
// Scheduling constants of wf_trace.  None of them can change a result; each is the measured optimum on MI355X, and a sweep builds a
// variant of the library with another value (tools/build_variant.sh NAME "-DWF_REFILL=16 ...").
#ifndef SHARD_BLOCK
#define SHARD_BLOCK 2048
#endif
constexpr uint32_t kShardBlock = SHARD_BLOCK;   // queue indices per block of the shard interleave (a power of two)
#ifndef WF_CHUNK_SHIFT
#define WF_CHUNK_SHIFT 12
#endif
constexpr int kWfChunkShift = WF_CHUNK_SHIFT;   // chunk = clamp(n >> this, 16, kWfChunk) ray ids per queue access
#ifndef WF_GUIDE_SHIFT
#define WF_GUIDE_SHIFT 9
#endif
constexpr int kWfGuideShift = WF_GUIDE_SHIFT;   // guided self-scheduling: the chunk shrinks to (rays left in the shard) >> this
#ifndef WF_REFILL
#define WF_REFILL 24
#endif
constexpr int kWfRefill = WF_REFILL;            // refill lanes once this many are idle (measured: 8..16 -2 %, 32 -0.4 %)
#ifndef WF_TRI_TRIG
#define WF_TRI_TRIG 64
#endif
constexpr int kWfTriTrig = WF_TRI_TRIG;         // parked leaves that force a triangle trip (64 = only when blocked rays outnumber walking ones)
// Shards a wave tries (its own included) before it takes the queue to be dry: 4 (16 = all: every wave then spends 16 returning atomics
// on hot words at the end of every launch; the shards are interleaved and equally long, so there is little to help with: 16 -> 4 is
// +1 % on configs[2], +3 % on configs[1], +4.5 % for an 8-way rank, r03_b20.log)
#ifndef WF_HELP_SHARDS
#define WF_HELP_SHARDS 4
#endif
constexpr int kWfHelpShards = WF_HELP_SHARDS;
static_assert(kWfHelpShards >= 1 && kWfHelpShards <= kWfShards, "a wave tries between one and all of the shards");
// wf_trace's waves per SIMD.  7 (72 VGPRs) rather than 8 (64): the two-triangle leaf test needs the room, and
// the kernel is bound by VALU issue, not by latency hiding (measured: 8 waves with 6-9 spilled registers and 6 waves
// with none are both slower; round 2 again: 8 waves +5 % kernel time).
#ifndef TRACE_WAVES
#define TRACE_WAVES 7
#endif
// Time slicing: every launch is followed by a device-wide dependency (the shade kernel needs all
// hits), so one ray that visits thousands of nodes would hold up the whole iteration (measured:
// ~800 us per launch).  A ray that has visited kWfBudget nodes is therefore suspended — cur, sp,
// closest hit and stack go to a record — and its stream simply waits one iteration; the next
// launch resumes it.  hit.prim <= -2 encodes "pending, record = -2 - prim".
constexpr int kWfBudget = 256;        // least node steps a ray may take per launch (measured: 96 cost 8 % on a 2M-stream render, >= 192 is flat)
constexpr int kSuspInts = 4 + kWfLdsStack + kWfOvfLevels;

// block-aggregated append to four lists at once (live streams + one ray queue per kind): one atomicAdd
// per list per block.  (One atomic per wave was the shade kernel's bottleneck: ~100k returning atomics
// per launch on one cache line serialise at ~88 per microsecond; with one atomic per 256-thread block and the
// counters on separate lines they no longer show.)
// Must be called by every thread of the block.
constexpr int kShadeThreads = 1024;      // threads block_append's per-wave counts are sized for (wf_shade's launch bound; it runs 512-thread workgroups, two per CU, the init kernels 256)
constexpr int kLists = 1 + 2 * kRayKinds;      // live streams + per ray kind a front list (through the core box / unknown) and a back list (short rays)
template <int N>
PT_DEV void block_append(const bool (&e)[N], const uint32_t (&id)[N], uint32_t* const (&c)[N], uint32_t* const (&l)[N], const uint32_t (&top)[N])
{
    // top[k] = 0: list k grows upwards from index 0; top[k] = T > 0: it grows DOWNWARDS from index T (the short rays of a kind share
    // the kind's queue array with its other rays, from the other end)
    constexpr int W = kShadeThreads / 64;
    __shared__ uint32_t s_cnt[N][W];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nw = (int)(blockDim.x >> 6);
    unsigned long long m[N];
#pragma unroll
    for (int k = 0; k < N; k++) { m[k] = __ballot(e[k]); if (lane == 0) s_cnt[k][wave] = __builtin_popcountll(m[k]); }
    __syncthreads();
    if (threadIdx.x < N) {
        // one thread per list: the block's total -> one atomic, and every wave's count turned into its start position in place
        // (every thread summing the counts of the waves below its own: 7 lists x up to 7 LDS reads per thread, -1.3 % overall, r03_b26.log)
        uint32_t tot = 0;
        for (int w = 0; w < nw; w++) tot += s_cnt[threadIdx.x][w];
        uint32_t run = tot ? atomicAdd(c[threadIdx.x], tot) : 0u;
        for (int w = 0; w < nw; w++) { const uint32_t v = s_cnt[threadIdx.x][w]; s_cnt[threadIdx.x][w] = run; run += v; }
    }
    __syncthreads();
    const unsigned long long below = (1ull << lane) - 1ull;
#pragma unroll
    for (int k = 0; k < N; k++) {
        const uint32_t pos = s_cnt[k][wave] + (uint32_t)__builtin_popcountll(m[k] & below);
        if (e[k]) l[k][top[k] ? top[k] - pos : pos] = id[k];
    }
}

// The seven lists a kernel appends to, in the order of e[] / ids[]: the live streams (list 0: `liveList`, counted by nActive), then per
// ray kind k the front list (rays through the core box, or of unknown length: grows upwards from index 0 of rq[k], counted by
// nRays[k][0]) and, last, per kind the back list (short rays: grows DOWNWARDS from the last entry of the same array, counted by
// nRays[k][kShortWord]).  wf_trace's queue index space is these six ray lists in a row (QueueSegments).  The caller says which lists
// its thread joins (e) and with what entry (ids: the stream, for a suspended traversal with kResumeBit); where the lists and their
// counters live is known here alone.  Must be called by every thread of the block.
PT_DEV void append_lists(const WfBuf& b, int slot, uint32_t* liveList, const bool (&e)[kLists], const uint32_t (&ids)[kLists])
{
    const uint32_t topIdx = (uint32_t)(b.hit[1] - b.hit[0]) - 1u;      // n16 - 1: the last entry of a queue array
    uint32_t* const c[kLists] = {&b.cnt[slot].nActive, &b.cnt[slot].nRays[0][0], &b.cnt[slot].nRays[1][0], &b.cnt[slot].nRays[2][0],
                                 &b.cnt[slot].nRays[0][kShortWord], &b.cnt[slot].nRays[1][kShortWord], &b.cnt[slot].nRays[2][kShortWord]};
    uint32_t* const l[kLists] = {liveList, b.rq[0], b.rq[1], b.rq[2], b.rq[0], b.rq[1], b.rq[2]};
    const uint32_t top[kLists] = {0u, 0u, 0u, 0u, topIdx, topIdx, topIdx};
    block_append<kLists>(e, ids, c, l, top);
}

// The end of every init kernel: stream sid, if live, joins the live list, and its first ray is queued by class (shortRay implies live).
PT_DEV void append_first_ray(const WfBuf& b, uint32_t sid, bool live, bool shortRay)
{
    const bool e[kLists] = {live, live && !shortRay, false, false, shortRay, false, false};
    const uint32_t ids[kLists] = {sid, sid, sid, sid, sid, sid, sid};
    append_lists(b, 0, b.active[0], e, ids);
}

// ---------------------------------------------------------------------------------------
// wf_init, wf_init_list, wf_init_views, wf_init_rays: StartRender prologue for every stream (pathtracer.cu:70-74).
// This is the only place of the pipeline that turns a stream into a pixel: from here on a stream is its slot, so wf_trace, wf_shade
// and wf_drain are the same for all of them.  The three camera kernels differ in `place` alone: it turns (local tile, pass relative to the job's
// first) into the stream's camera, its tile of the frame and its pass.  TILE_TEST: a tile beyond the frame is a dead stream.
// ---------------------------------------------------------------------------------------
template <bool TILE_TEST, class Place>
PT_DEV void init_streams(const DevScene& sc, const DevParams& prm, const WfBuf& b, uint32_t nStreams, Place place)
{
    const uint32_t sid = blockIdx.x * 256u + threadIdx.x;
    bool live = false, camShort = false;
    if (sid < nStreams) {
        const uint32_t unit = (uint32_t)prm.unit_base + (sid >> 6), lane = sid & 63;
        const int pass_rel = (int)(unit / (uint32_t)prm.n_tiles_local);
        int tile, pass;
        const DevCamera& cam = place(unit % (uint32_t)prm.n_tiles_local, pass_rel, tile, pass);
        const int tx = tile % prm.tiles_x, ty = tile / prm.tiles_x;
        const int px = tx * kTile + (int)(lane & 7), py = ty * kTile + (int)(lane >> 3);
        live = (!TILE_TEST || tile < prm.n_tiles_total) && (px < cam.W) && (py < cam.H);
        if (live) {
            init_stream(cam, prm, b, sid, px, py, pass);
            const float4 d0 = b.ray_d[0][sid];
            camShort = ray_is_short(sc, f3(cam.pos[0], cam.pos[1], cam.pos[2]), f3(d0.x, d0.y, d0.z), 3.0e38f);
        } else {
            b.staging[3 * (size_t)sid + 0] = 0.f; b.staging[3 * (size_t)sid + 1] = 0.f; b.staging[3 * (size_t)sid + 2] = 0.f;
        }
    }
    // the camera ray: queued by class like every other ray (a pixel that looks past the mesh has a short ray)
    append_first_ray(b, sid, live, live && camShort);
}

// one camera, the fixed share of the frame: local tile lt is tile lt * world + rank
__global__ __launch_bounds__(256)
void wf_init(DevScene sc, DevCamera cam, DevParams prm, WfBuf b, uint32_t nStreams)
{
    init_streams<true>(sc, prm, b, nStreams, [&](uint32_t lt, int pass_rel, int& tile, int& pass) -> const DevCamera& {
        tile = (int)lt * prm.world + prm.rank; pass = prm.first_pass + pass_rel; return cam; });
}

// one camera, local tile lt taken from a list (pt_render_tile_list: any n_tiles_local tiles of the frame, in any order)
__global__ __launch_bounds__(256)
void wf_init_list(DevScene sc, DevCamera cam, DevParams prm, WfBuf b, uint32_t nStreams, const int32_t* __restrict__ tileList)
{
    init_streams<true>(sc, prm, b, nStreams, [&](uint32_t lt, int pass_rel, int& tile, int& pass) -> const DevCamera& {
        tile = tileList[(int)lt]; pass = prm.first_pass + pass_rel; return cam; });
}

// a batch of cameras (pt_render_views).  Local tile lt -> (view = lt / tilesPerView, tile = lt % tilesPerView, inside the frame by
// construction): the camera comes from a device array, the pass is the view's own first pass + pass_rel.  prm is that of a world of one
// whose "frame" has n_views x tilesPerView tiles (tiles_x / tiles_y / n_tiles_total are one view's), so the unit and staging
// arithmetic downstream is what it is for one camera.
__global__ __launch_bounds__(256)
void wf_init_views(DevScene sc, DevParams prm, WfBuf b, uint32_t nStreams, const DevCamera* __restrict__ cams, const int32_t* __restrict__ firstPass,
                   uint32_t tilesPerView)
{
    init_streams<false>(sc, prm, b, nStreams, [&](uint32_t lt, int pass_rel, int& tile, int& pass) -> DevCamera {
        const uint32_t view = lt / tilesPerView;
        tile = (int)(lt % tilesPerView); pass = firstPass[view] + pass_rel; return cams[view]; });
}

// the caller's rays (pt_render_rays): no camera and no pixel.  Stream -> unit -> (group g of 64 rays, pass relative to the job's first);
// ray i = 64 g + lane is live iff i < nRays.  Seed: seed_i + pass * seedStride in wrapping 32-bit arithmetic, seed_i = raySeed[i], or i
// when raySeed is null.  The ray is queued by class like a camera ray; the padding lanes of the last group are dead streams.
__global__ __launch_bounds__(256)
void wf_init_rays(DevScene sc, DevParams prm, WfBuf b, uint32_t nStreams, const float4* __restrict__ rays, const int32_t* __restrict__ raySeed,
                  uint32_t seedStride, uint32_t nRays)
{
    const uint32_t sid = blockIdx.x * 256u + threadIdx.x;
    bool live = false, shortRay = false;
    if (sid < nStreams) {
        const uint32_t unit = (uint32_t)prm.unit_base + (sid >> 6);
        const uint32_t i = (unit % (uint32_t)prm.n_tiles_local) * 64u + (sid & 63u);
        const uint32_t pass = (uint32_t)prm.first_pass + unit / (uint32_t)prm.n_tiles_local;
        live = i < nRays;
        if (live) {
            const float4 r0 = rays[2 * (size_t)i], r1 = rays[2 * (size_t)i + 1];      // org.xyz dir.x | dir.yz reserved tmax
            const f3 org(r0.x, r0.y, r0.z), dir(r0.w, r1.x, r1.y);
            init_ray_stream(prm, b, sid, org, dir, r1.w, (raySeed ? (uint32_t)raySeed[i] : i) + pass * seedStride);
            shortRay = ray_is_short(sc, org, dir, r1.w);
        } else {
            b.staging[3 * (size_t)sid + 0] = 0.f; b.staging[3 * (size_t)sid + 1] = 0.f; b.staging[3 * (size_t)sid + 2] = 0.f;
        }
    }
    append_first_ray(b, sid, live, shortRay);
}

// wf_trace's queue index space for one launch, six segments in a row: the rays of kind 0 (path), 1 and 2 (shadow) queued from the front
// of their arrays — rays through the scene's core box, or of unknown length —, then the SHORT rays of each kind, queued from the back of
// the same arrays (pt_stream.h: ray_is_short; append_lists): what is in flight when the queue runs dry is then short, and so is the
// launch tail.  p1..p5 are where segments 1..5 start, n is the number of rays.
struct QueueSegments {
    uint32_t p1, p2, p3, p4, p5, n;
    PT_DEV explicit QueueSegments(const WfCounters& c)
    {
        p1 = c.nRays[0][0];
        p2 = p1 + c.nRays[1][0];
        p3 = p2 + c.nRays[2][0];
        p4 = p3 + c.nRays[0][kShortWord];
        p5 = p4 + c.nRays[1][kShortWord];
        n = p5 + c.nRays[2][kShortWord];
    }
    // queue index q -> kn = kind * n16 and the entry of rq[0] (the per-kind arrays lie back to back) that holds the ray: the front part of a
    // kind's array upwards, its short part downwards from n16 - 1
    PT_DEV uint32_t entry(uint32_t q, uint32_t n16, uint32_t& kn) const
    {
        const bool shortSeg = q >= p3;
        const uint32_t b0 = shortSeg ? p3 : 0u, b1 = shortSeg ? p4 : p1, b2 = shortSeg ? p5 : p2;      // segment starts of kinds 0, 1, 2
        const bool k0 = q < b1, k1 = q < b2;                                   // kind 0 / kind 0 or 1
        kn = k0 ? 0u : (k1 ? n16 : 2u * n16);
        const uint32_t local = q - (k0 ? b0 : (k1 ? b1 : b2));
        return kn + (shortSeg ? n16 - 1u - local : local);
    }
};

// A ray's hit record: (t, primitive), or for a suspended traversal (t, -2 - record).  PUBLISH: stored device-coherently, wf_shade's early
// phase reads it while this kernel drains.
template <bool PUBLISH>
PT_DEV void store_hit(const WfBuf& b, uint32_t hs, float t, int prim)
{
    if (PUBLISH) __hip_atomic_store((unsigned long long*)&b.hit[0][hs], (unsigned long long)__float_as_uint(t) | ((unsigned long long)(uint32_t)prim << 32), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else b.hit[0][hs] = make_float2(t, __int_as_float(prim));
}

// ---------------------------------------------------------------------------------------
// wf_trace: persistent closest-hit kernel with lane refill.
// Shadow rays (kinds 1 and 2, queue indices >= nPath): the ray only decides whether the closest hit is the sampled light point
// (GetLightColor, CudaUtil.cuh:150-166: visible iff |hit.p - P| < EPS, with t_max = |P-p|+1).
// Any hit at t < (t_max - 1) - 5e-4 proves the closest hit is at least ~4e-4 in front of P,
// hence not within EPS = 1e-4 of it, so traversal may stop there; what is reported is then
// some occluder, for which the |hit.p - P| < EPS test fails exactly as it would for the
// closest one.  That test is made here, in the ray's epilogue (pt_shade.h: nee_verdict): the hit
// record of a shadow ray carries the primitive only if it is the light point.
// ---------------------------------------------------------------------------------------
// MODE: 0 production; 1, 2, 3 the diagnostic builds of PTAMD_TSTAT — all they add is in `probe` (pt_trace_probe.h), and so is the
// kernel argument they read.  PUBLISH: hits are stored device-coherently (wf_shade PHASE 1 reads them while this kernel drains).
// budgetShift, budgetMin, lateBudget: WfTuning.
template <int MODE, bool PUBLISH = false>
__global__ __launch_bounds__(256, TRACE_WAVES)
void wf_trace(DevScene sc, WfBuf b, int slot, int ovfStride, int parity, int budgetShift, int budgetMin, int lateBudget, typename TraceProbe<MODE>::Args probeArgs)
{
    TraceProbe<MODE> probe(probeArgs);
    __shared__ int lds_stack[4][kWfLdsStack * 64];
    const QueueSegments seg(b.cnt[slot]);
    const uint32_t n = seg.n;
    if ((uint32_t)blockIdx.x * 256u >= n) return;      // surplus blocks leave before touching the queue (fewer rays per workgroup: no faster, r02_b21.log)

    const int lane = threadIdx.x & 63;
    // node steps a ray may take in this launch before it is suspended: large launches hide long rays,
    // small (latency-bound) launches must not wait for them
    const int budget = (n >> budgetShift) < (uint32_t)budgetMin ? budgetMin : ((n >> budgetShift) > 1024u ? 1024 : (int)(n >> budgetShift));
    const int* __restrict__ suspIn = b.susp[parity ^ 1];
    int* __restrict__ suspOut = b.susp[parity];
    // rays a wave takes per queue access: ~n / (4 x resident waves), between 16 and kWfChunk (one word
    // saturates near 88 returning atomics per microsecond, so large launches take large chunks)
    const uint32_t kChunk = (n >> kWfChunkShift) < 16u ? 16u : ((n >> kWfChunkShift) > (uint32_t)kWfChunk ? (uint32_t)kWfChunk : (n >> kWfChunkShift));

    uint32_t chunkPos = 0, chunkEnd = 0;   // wave-uniform
    uint32_t seenLeft = 0xffffffffu;       // rays this wave last saw left in its current shard (wave-uniform)
    int shard = (int)(blockIdx.x % kWfShards), shardsTried = 0;   // wave-uniform; blockIdx % 8 shares an XCD, so a shard stays in one L2
    bool exhausted = false;                // wave-uniform
    bool hasRay = false;
    // per-ray registers
    // inv: the reference's Normalize(inv(dir)) (CudaUtil.cuh:70) — what its leaf-box test uses, and a perfectly good
    // inverse direction for the tree walk, which then measures t in units of 1/|inv(dir)|; cscale converts the
    // closest hit into those units.  Degenerate rays (a zero direction component): 1/dir clamped to +-1e30, true units.
    f3 org(0.f, 0.f, 0.f), dir(0.f, 0.f, 1.f), inv(0.f, 0.f, 0.f);
    float bestT = 0.f, cscale = 0.f, stopBelow = 0.f;
    int bestPrim = -1, cur = kDone, sp = 0, steps = 0;
    int pend = 0;        // a leaf this ray has reached but not yet tested (0 = none): see "postponed leaves" below
    bool degenerate = false;
    // The per-kind arrays of WfBuf lie back to back (hit[k] = hit[0] + k * n16, rq[k] likewise, ray_o[k] = ray_o[0] + 2 k n16, ray_d[k] = ray_o[k] + n16):
    // a ray is known by hs = kind * n16 + stream id, its hit slot is hit[0][hs], and no pointer is ever selected by kind.
    const uint32_t n16 = (uint32_t)(b.hit[1] - b.hit[0]);
    uint32_t hs = 0;

    // The ray's stack, sp entries: entry k of this lane lives in LDS below kWfLdsStack, in global memory above (5e-7 of the node steps).
    // (an LDS pointer by type: were it a generic one, the compiler could merge the two stores of stack_put into ONE flat_store with a selected address)
    typedef __attribute__((address_space(3))) int LdsInt;
    LdsInt* stack = (LdsInt*)&lds_stack[threadIdx.x >> 6][lane];
    int* ovf = b.ovf + (blockIdx.x * 256 + threadIdx.x);
    // The read: written as a plain select of the two places the compiler merges them into ONE flat_load (LDS through the texture path,
    // waited for with vmcnt(0), i.e. behind every outstanding store); the empty asm pins the LDS read down as a ds_read of its own.
    auto stack_at = [&](int k) -> int {
        int v = stack[(k < kWfLdsStack ? k : 0) * 64];
        asm volatile("" : "+v"(v));
        if (k >= kWfLdsStack) v = ovf[(k - kWfLdsStack) * ovfStride];
        return v;
    };
    auto stack_put = [&](int k, int v) { if (k < kWfLdsStack) stack[k * 64] = v; else ovf[(k - kWfLdsStack) * ovfStride] = v; };
    auto push = [&](int v) { stack_put(sp, v); sp++; };
    // the next entry of the stack becomes the ray's position; an empty stack ends the walk
    auto pop = [&] { if (sp == 0) cur = kDone; else { sp--; cur = stack_at(sp); } };
    // the suspend record of a traversal (kSuspInts words): cur, sp, closest hit, then the stack
    auto save_walk = [&](int* rec) {
        rec[0] = cur; rec[1] = sp; rec[2] = __float_as_int(bestT); rec[3] = bestPrim;
        for (int k = 0; k < sp; k++) rec[4 + k] = (k < kWfLdsStack) ? stack[k * 64] : ovf[(k - kWfLdsStack) * ovfStride];
    };
    auto restore_walk = [&](const int* rec) {
        cur = rec[0]; sp = rec[1]; bestT = __int_as_float(rec[2]); bestPrim = rec[3];
        for (int k = 0; k < sp; k++) stack_put(k, rec[4 + k]);
    };

    for (;;) {
        probe.trip_top();
        // ---- hand new rays to idle lanes (ballot + mbcnt compaction) ----
        const unsigned long long idle = __ballot(!hasRay);
        const int nIdle = __builtin_popcountll(idle);
        if (!exhausted && (nIdle >= kWfRefill)) {
            if (chunkPos == chunkEnd) {
                // The queue index space is cut into kWfShards ranges, each with its own head word (a
                // single word saturates near 88 returning atomics per microsecond, which throttled
                // launches of a few million rays).  A wave drains its home shard, then helps the next.
                for (;;) {
                    // A shard owns every 16th block of kShardBlock queue indices (block b -> shard b % 16), so all shards walk the index
                    // space front to back together: path rays are started first and the (shorter, any-hit) shadow rays last, which
                    // is what is still in flight when the queue runs dry.  chunkPos / chunkEnd are shard-local positions.
                    const uint32_t rounds = n / (kShardBlock * kWfShards), rem = n % (kShardBlock * kWfShards);
                    const uint32_t part = rem > (uint32_t)shard * kShardBlock ? rem - (uint32_t)shard * kShardBlock : 0u;
                    const uint32_t cnt = rounds * kShardBlock + (part < kShardBlock ? part : kShardBlock);      // indices this shard owns
                    // guided self-scheduling: the chunk shrinks with what this wave last saw left in the shard, so the
                    // last rays of a launch are spread over many waves instead of queuing behind one
                    uint32_t want = seenLeft >> kWfGuideShift;
                    want = want < 16u ? 16u : (want > kChunk ? kChunk : want);
                    uint32_t start = 0;
                    if (lane == 0) start = atomicAdd(&b.cnt[slot].head[shard].v, want);
                    probe.queue_atomic();
                    start = __builtin_amdgcn_readfirstlane(start);
                    if (start < cnt) {
                        chunkPos = start; chunkEnd = (cnt - start > want) ? start + want : cnt; seenLeft = cnt - start; break; }
                    seenLeft = 0xffffffffu;
                    shard = (shard + 1) % kWfShards;
                    if (++shardsTried >= kWfHelpShards) { exhausted = true; probe.queue_dry(); break; }
                }
            }
            if (!exhausted) {
                const uint32_t avail = chunkEnd - chunkPos;
                const uint32_t take = ((uint32_t)nIdle < avail) ? (uint32_t)nIdle : avail;
                probe.refilled(take);
                if (!hasRay) {
                    const uint32_t r = (uint32_t)__builtin_popcountll(idle & ((1ull << lane) - 1ull));
                    if (r < take) {
                        const uint32_t j = chunkPos + r;      // shard-local -> queue index
                        const uint32_t q = ((j / kShardBlock) * kWfShards + (uint32_t)shard) * kShardBlock + (j % kShardBlock);
                        uint32_t kn;      // kind * n16
                        const uint32_t qid = b.rq[0][seg.entry(q, n16, kn)];
                        hs = kn + (qid & ~kResumeBit);
                        const float4 o = b.ray_o[0][hs + kn], d = b.ray_d[0][hs + kn];
                        org = f3(o.x, o.y, o.z); dir = f3(d.x, d.y, d.z);
                        ray_setup(dir, inv, cscale, degenerate);      // pt_trace.h
                        stopBelow = kn != 0u ? d.w : -__builtin_inff();      // shadow rays: any hit below this t ends the traversal (pt_stream.h: shadow_stop_t)
                        steps = 0;
                        if (qid & kResumeBit) {
                            // resume a suspended traversal (wf_shade flags the queue entry: the hit slot then holds the record number;
                            // a fresh ray's hit slot is not read at all — 8 scattered bytes per ray that nothing else would fetch)
                            const float2 prev = b.hit[0][hs];
                            restore_walk(suspIn + (size_t)(-2 - __float_as_int(prev.y)) * kSuspInts);
                        } else {
                            bestT = o.w; bestPrim = -1; cur = 0; sp = 0;
                        }
                        pend = 0;
                        hasRay = true;
                    }
                }
                chunkPos += take;
            }
        }
        probe.after_refill();
        if (__ballot(hasRay) == 0ull) { if (exhausted) break; else continue; }
        probe.trip_begins(hasRay, pend, exhausted, lane);
        if (hasRay) {
            // Only one code path runs per trip: a node step or ONE triangle test per lane (the vote is below).
            // (The classic while-while shape made 64 lanes wait for the slowest lane to reach a leaf every
            // round — 24 % VALU lane utilisation; running both paths every trip, "if-if", gave 29 %.)
            if (cur >= 0) {
                // lateBudget (PTAMD_LB, default 64): once the queue is dry and this wave is down to its last two rays, a ray that has already done
                // that many node steps is suspended like one that has spent its budget — the launch then does not wait for a lone ray of several
                // hundred steps (it goes on in the next launch, from the start and among full waves)
                if (steps >= ((lateBudget > 0 && exhausted && nIdle >= 62) ? lateBudget : budget)) {
                    // node budget spent: suspend (or, if the pool is full, carry on)
                    const uint32_t rec = atomicAdd(&b.cnt[slot].nSusp, 1u);
                    if (rec < b.suspCap) {
                        if (pend != 0) { push(pend); pend = 0; }
                        save_walk(suspOut + (size_t)rec * kSuspInts);
                        store_hit<PUBLISH>(b, hs, bestT, -2 - (int)rec);
                        hasRay = false;
                        cur = kDone;
                    } else {
                        steps = -(1 << 28);
                    }
                }
            }
            // Wave vote with postponed leaves.  A ray that reaches a leaf does not wait for a triangle trip:
            // it parks the leaf in `pend` and goes on with the next entry of its stack; only a ray that
            // reaches a SECOND leaf (or has nothing else left) needs a triangle trip.  A triangle trip
            // then serves every ray with a parked leaf, a node trip every ray that still holds a node:
            // both kinds of trip run fuller than when each ray blocked at its first leaf
            // (59 % of lane-trips useful before).  Order of tests does not matter to the result: the tie rule
            // makes the closest hit independent of it; parked leaves only delay the tightening of the cull.
            const int nNode = __builtin_popcountll(__ballot(cur >= 0));
            const int nTri = __builtin_popcountll(__ballot(hasRay && pend != 0));
            const int nBlk = __builtin_popcountll(__ballot(hasRay && pend != 0 && cur < 0));
            const bool doTri = nTri > 0 && (nTri >= kWfTriTrig || nBlk >= nNode);
            const bool doNode = !doTri;
            probe.after_vote(doNode, nNode, nTri, hasRay);
            if (doNode && cur >= 0) {
                // ---- one 4-wide node (pt_trace.h: quad_order): nearest child next, the other hit children to the stack ----
                steps++;
                const uint4* np = sc.quad + 4 * (size_t)cur;
                uint4 n0 = np[0], n1 = np[1], n2 = np[2], n3 = np[3];
                probe.node_arrived(n0, n1, n2, n3);
                int k0, k1, k2, k3, r0, r1, r2, r3;
                quad_order(n0, n1, n2, n3, org, inv, bestT * cscale, k0, k1, k2, k3, r0, r1, r2, r3);
                if (!quad_descend(k0, k1, k2, k3, r0, r1, r2, r3, cur, push)) pop();
                probe.after_node(sp);
                // a leaf: park it, carry on with the next stack entry
                if (cur < 0 && cur != kDone && pend == 0) { pend = cur; pop(); }
            } else if (doTri && hasRay && pend != 0) {
                // ---- the parked leaf: its (up to) two triangles in one go ----
                const int code = ~pend, first = code >> 3, cnt = code & 7;
                pend = 0;
                if (cnt > 0) {
                    tri_test_pairrec(sc, first, cnt > 1, org, dir, inv, degenerate, bestT, bestPrim);
                    if (bestPrim >= 0 && bestT < stopBelow) { cur = kDone; sp = 0; }          // shadow ray: any occluder in front of the light will do
                    else if (cnt > 2) pend = ~(((first + 2) << 3) | (cnt - 2));
                }
                // the ray was waiting with a second leaf: park that one, take the next stack entry
                if (pend == 0 && cur < 0 && cur != kDone) { pend = cur; pop(); }
            }
            probe.after_step(doNode);
            if (hasRay && cur == kDone && pend == 0) {
                spheres_closest(sc, org, dir, bestT, bestPrim);
                // A shadow ray (hs >= n16) that hit something: the verdict is formed here, where org, dir and t are still in registers — is the
                // hit the sampled light point? — and the record carries the primitive only if it is (pt_shade.h: nee_verdict).  wf_shade then
                // needs neither the ray nor the light point.  lp and lpA lie back to back like every per-kind array: lp[(kind - 1) n16 + sid].
                // The light point is fetched here, not at the refill: it must not hold registers during the walk — and only for a hit that
                // can be the light point at all: one below stopBelow is provably in front of it (pt_stream.h: shadow_stop_t, the argument
                // the early stop rests on), so its verdict is known without it.
                if (hs >= n16 && bestPrim >= 0 && bestT < stopBelow) bestPrim = -1;
                if (hs >= n16 && bestPrim >= 0) {
                    const float4 lq = b.lp[hs - n16];
                    bestPrim = nee_verdict(org, dir, f3(lq.x, lq.y, lq.z), bestT, bestPrim);
                }
                store_hit<PUBLISH>(b, hs, bestT, bestPrim);
                hasRay = false;
                probe.ray_end(steps);
            }
            probe.trip_ends();
        }
    }
    probe.wave_end(n, lane);
}

// ---------------------------------------------------------------------------------------
// wf_shade: one thread per live stream, one bounce.
// ---------------------------------------------------------------------------------------
// PHASE (round 3, "early shade"): the launch tail of wf_trace — the last rays of a launch finishing in ever emptier waves — leaves the
// chip idle for ~0.3 ms per iteration, which is most of an iteration for one rank of an 8-way tile split.  With PHASE 1 / 2 the shade
// step of an iteration is cut in two launches:
//   PHASE 1 (early)  runs on a second HIP stream BESIDE the draining wf_trace: its workgroups get wave slots as traversal waves leave.
//                    A stream is shaded only if every ray it is waiting for is already back — wf_trace publishes a hit with a
//                    device-scope store, the slot held kNotReady since the ray was emitted (MARK) and is read here with a device-scope
//                    load (the XCDs' L2s are not coherent with each other) —, otherwise it is left alone.  Nothing is appended here: the
//                    outcome of a shaded stream (alive / which rays it emitted) is parked in res[list position].  No waiting, no
//                    spinning: a stream whose rays are not back is simply skipped.
//   PHASE 2 (rest)   runs after both have finished: shades the streams phase 1 skipped and does ALL the appends, in list order — so the
//                    live list and the ray queues keep stream order exactly as with one launch.
// A stream goes through the same shade_step either way: result-neutral.
enum : uint32_t { R_ALIVE = 1, R_EMIT0 = 2, R_EMIT1 = 4, R_EMIT2 = 8, R_SHORT0 = 16, R_SHORT1 = 32, R_SHORT2 = 64, R_DONE = 128 };      // res[]: what phase 1 did with a list position

// A stream's hit slot, touched once per kernel.  COHERENT (PHASE 1): wf_trace is still publishing hits beside this kernel.
template <bool COHERENT>
PT_DEV float2 load_hit(const float2* p)
{
    if (!COHERENT) return *p;
    const unsigned long long v = __hip_atomic_load((const unsigned long long*)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return make_float2(__uint_as_float((uint32_t)v), __uint_as_float((uint32_t)(v >> 32)));
}

// Cam: a DevCamera, the ViewTable of a batch of views (pt_render_views) or the RayTable of the caller's rays (pt_render_rays) — all that
// differs is where a restarted camera ray takes its origin from (pt_stream.h: camera_origin).
// 4 waves/SIMD (126 VGPRs, nothing spilled since the library is built without the SLP vectoriser): 3 waves/SIMD is 9...13 % slower
// (r02_t16_shade_shapes_after_noslp.log).
// WAVES is 4 and MARK is PHASE != 0 in every instantiation the pipeline names (shade_kernel); both stay template parameters because
// they are part of the kernels' names, which profiles and tests read.
template <int WAVES, bool TWO, int PHASE = 0, bool MARK = false, class Cam = DevCamera>
__global__ __launch_bounds__(WAVES * 256, WAVES)
void wf_shade(DevScene sc, Cam cam, DevParams prm, WfBuf b, int slotIn, int slotOut, int slotClear, int listIn)
{
    static_assert(WAVES == 4 && MARK == (PHASE != 0), "the two-phase step needs the not-ready marks; one launch per step does not");
    const uint32_t nIn = b.cnt[slotIn].nActive;
    if (PHASE != 1 && blockIdx.x == 0) for (int k = threadIdx.x; k < kWfSlotBytes / 4; k += blockDim.x) ((uint32_t*)&b.cnt[slotClear])[k] = 0;
    if ((uint32_t)blockIdx.x * blockDim.x >= nIn) return;
    const uint32_t idx = blockIdx.x * blockDim.x + threadIdx.x;
    const bool have = idx < nIn;
    bool alive = false, emit[kRayKinds] = {false, false, false};
    uint32_t sid = 0, resume = 0;      // resume: the queued rays are suspended traversals (wf_trace then reads their records)
    uint32_t cls = 0;                  // bit k: the ray of kind k this step emitted is short (queued from the back of its queue)
    bool step = have;
    if (have) {
        // While no stream has retired yet (more than half of a render's iterations) every stream is alive, so list position idx can
        // simply take stream idx: one dependent fetch level less for the whole step (the list itself is in stream order only inside the
        // blocks that appended to it; any one-to-one assignment of streams to lanes gives the same result).
        sid = (nIn == (uint32_t)prm.n_units * 64u) ? idx : b.active[listIn][idx];
        if (PHASE == 2) {
            const uint32_t r = b.res[idx];
            if (r & R_DONE) {      // shaded by phase 1: only the appends are left
                step = false;
                alive = (r & R_ALIVE) != 0; emit[0] = (r & R_EMIT0) != 0; emit[1] = (r & R_EMIT1) != 0; emit[2] = (r & R_EMIT2) != 0;
                cls = (r / R_SHORT0) & 7u;
            }
        }
    }
    if (step) {
        SState st;
        const float2 hitP = load_hit<PHASE == 1>(&b.hit[0][sid]), hitS = load_hit<PHASE == 1>(&b.hit[1][sid]), hitA = load_hit<PHASE == 1>(&b.hit[2][sid]);      // same fetch level as the state
        load_state(b, sid, st);
        // a ray of this stream is still being traversed (time-sliced): wait one iteration
        const int pendP = (st.flags & F_PATH) ? __float_as_int(hitP.y) : -1, pendS = (st.flags & F_SHADOW) ? __float_as_int(hitS.y) : -1;
        const int pendA = (st.flags & F_SHADOWA) ? __float_as_int(hitA.y) : -1;
        if (PHASE == 1 && (pendP <= -2 || pendS <= -2 || pendA <= -2)) {
            // phase 1: a ray is not back yet (kNotReady), or a traversal is suspended (its slot keeps the record number until wf_trace
            // resumes it, so the slot cannot tell "back" from "not yet"): phase 2 takes the stream
            step = false;
        } else if (pendP <= -2 || pendS <= -2 || pendA <= -2) {
            alive = true; emit[0] = pendP <= -2; emit[1] = pendS <= -2; emit[2] = pendA <= -2; resume = kResumeBit;
        } else {
            const bool done = shade_step_t<TWO>(sc, cam, prm, b, sid, st, hitP, hitS, hitA);
            if (done) {
                write_mean(b, prm, sid, st);
            } else {
                const uint32_t nf = st.flags;
                store_state(b, sid, st);
                alive = true;
                emit[0] = (nf & F_PATH) != 0; emit[1] = (nf & F_SHADOW) != 0; emit[2] = (nf & F_SHADOWA) != 0;
                cls = st.cls;
            }
        }
    }
    // MARK: the hit slot of every ray this step emitted says "not traced yet" until wf_trace publishes its hit (a suspended traversal
    // that is re-queued keeps its slot: it holds the record number).  Written here, at the end, where nothing else is live.
    if (MARK && step && !resume) {
#pragma unroll
        for (int k = 0; k < kRayKinds; k++) if (emit[k]) b.hit[k][sid] = make_float2(0.f, __int_as_float(kNotReady));
    }
    if (PHASE == 1) {
        if (have) b.res[idx] = (uint8_t)(step ? (R_DONE | (alive ? R_ALIVE : 0u) | (emit[0] ? R_EMIT0 : 0u) | (emit[1] ? R_EMIT1 : 0u) | (emit[2] ? R_EMIT2 : 0u) | (cls & 7u) * R_SHORT0) : 0u);
        return;
    }
    // a re-queued suspended traversal is long by definition: cls = 0 for it (it never went through the step)
    const bool s0 = (cls & 1u) != 0, s1 = (cls & 2u) != 0, s2 = (cls & 4u) != 0;
    const bool e[kLists] = {alive, emit[0] && !s0, emit[1] && !s1, emit[2] && !s2, emit[0] && s0, emit[1] && s1, emit[2] && s2};
    const uint32_t ids[kLists] = {sid, sid | resume, sid | resume, sid | resume, sid, sid, sid};
    append_lists(b, slotOut, b.active[listIn ^ 1], e, ids);
}

// ---------------------------------------------------------------------------------------
// wf_drain: run every remaining stream to its end inside one launch.
// The pipeline's bounce iterations each carry a device-wide dependency, and the last third of
// them serve only the few pixels whose every path runs the full depth (a render of 256 spp
// needs ~1800 iterations while the average stream is done after ~730).  Once few streams are
// left, per-launch latency — not throughput — sets the pace, so they are handed to this kernel:
// one lane per stream (every 2^spreadShift-th lane: the kernel is bound by latency, so thinner waves are faster), state in
// registers, rays traced in place (quad_step on the 4-wide tree, or trace_closest on the binary one when that walk would not fit
// the per-lane stack), same shade_step.  Pending time-sliced traversals are simply redone (they are deterministic).
// On by default for the last 80,000 live streams of a render (pt_scene.h: drain_below).
// ---------------------------------------------------------------------------------------
constexpr int kDrainQuadStack = 40;      // per-lane stack entries of wf_drain's 4-wide walk (40 KB of LDS per workgroup): trees up to 12 levels, the config scenes' depth
#ifndef DRAIN_MINBLOCKS
#define DRAIN_MINBLOCKS 1      // workgroups per CU the register allocation of wf_drain must allow: 1 = free (189 VGPRs with the 4-wide walk: 2 waves/SIMD), 3 = 168 VGPRs (16 spilled)
#endif
// quad_step, one step of one lane's walk through the 4-wide tree, lives in pt_trace.h (pt_query.hip walks with it too).
template <bool QUAD, class Cam = DevCamera>      // QUAD: walk the 4-wide tree (quad_step); the host picks it when the walk fits the per-lane stack.  Cam: as in wf_shade
__global__ __launch_bounds__(kBlockThreads, DRAIN_MINBLOCKS)
void wf_drain(DevScene sc, Cam cam, DevParams prm, WfBuf b, int slotIn, int listIn, int spreadShift)
{
    __shared__ int lds_stack[kWavesPerBlock][(QUAD ? kDrainQuadStack : kStackDepth) * 64];
    const uint32_t nIn = b.cnt[slotIn].nActive;
    // spreadShift: only every 2^s-th lane carries a stream.  The kernel is bound by latency (a wave steps at the pace of its slowest
    // lane, every bounce), and the chip is far from full at this point: thinner waves wait for the maximum of fewer paths
    const uint32_t t = blockIdx.x * (uint32_t)kBlockThreads + threadIdx.x;
    if (t & ((1u << spreadShift) - 1u)) return;
    const uint32_t idx = t >> spreadShift;
    if (idx >= nIn) return;
    int* stack = &lds_stack[threadIdx.x >> 6][threadIdx.x & 63];
    const uint32_t sid = b.active[listIn][idx];
    SState st;
    load_state(b, sid, st);
    load_shadow_ray(b, sid, st);      // this kernel traces the pending shadow ray itself (later ones come from bounce, in registers)
    for (;;) {
        float2 hitP = make_float2(0.f, __int_as_float(-1)), hitS = hitP, hitA = hitP;
        TraceStats ts{0, 0, 0};
        if (QUAD) {
            // The rays of this bounce (second-to-last shadow ray, shadow ray, path ray: any subset) in ONE flat loop: a lane that has finished a ray
            // sets up its next one inside the loop, so the wave waits for the lane with the most steps in all — not, as with one
            // loop per ray kind, for the slowest lane of each kind in turn.
            int todo = ((st.flags & F_SHADOWA) ? 1 : 0) | ((st.flags & F_SHADOW) ? 2 : 0) | ((st.flags & F_PATH) ? 4 : 0);
            f3 org(0.f, 0.f, 0.f), dir(0.f, 0.f, 1.f), inv(0.f, 0.f, 0.f), lightP(0.f, 0.f, 0.f);      // lightP: the light point a shadow ray aims at
            float cscale = 0.f, bestT = 0.f, stopBelow = 0.f;
            bool degenerate = false;
            int bestPrim = -1, cur = 0, sp = 0, kind = -1;
            for (;;) {
                if (kind < 0) {
                    if (todo == 0) break;
                    kind = __builtin_ctz((unsigned)todo); todo &= todo - 1;
                    if (kind == 0) {
                        const float4 ao = b.ray_o[2][sid], ad = b.ray_d[2][sid], la = b.lpA[sid];
                        org = f3(ao.x, ao.y, ao.z); dir = f3(ad.x, ad.y, ad.z); bestT = ao.w; stopBelow = ad.w; lightP = f3(la.x, la.y, la.z);
                    } else if (kind == 1) { org = st.shO; dir = st.shD; bestT = st.shTmax; stopBelow = shadow_stop_t(st.shO, st.shTmax); lightP = st.lightP; }
                    else { org = st.pathO; dir = st.pathD; bestT = primary_tmax(cam, b, sid, st.flags); stopBelow = -__builtin_inff(); }
                    ray_setup(dir, inv, cscale, degenerate);
                    bestPrim = -1; cur = 0; sp = 0;
                }
                if (quad_step(sc, org, dir, inv, cscale, degenerate, stopBelow, stack, cur, sp, bestT, bestPrim)) {
                    spheres_closest(sc, org, dir, bestT, bestPrim);
                    if (kind != 2) bestPrim = nee_verdict(org, dir, lightP, bestT, bestPrim);      // a shadow ray's record carries the verdict
                    const float2 h = make_float2(bestT, __int_as_float(bestPrim));
                    if (kind == 0) hitA = h; else if (kind == 1) hitS = h; else hitP = h;
                    kind = -1;
                }
            }
        } else {
        if (st.flags & F_SHADOWA) {
            const float4 ao = b.ray_o[2][sid], ad = b.ray_d[2][sid], la = b.lpA[sid];
            const f3 o(ao.x, ao.y, ao.z), d(ad.x, ad.y, ad.z);
            float t; const int prim = trace_closest<false>(sc, o, d, ao.w, stack, t, ts); hitA = make_float2(t, __int_as_float(nee_verdict(o, d, f3(la.x, la.y, la.z), t, prim)));
        }
        if (st.flags & F_SHADOW) { float t; const int prim = trace_closest<false>(sc, st.shO, st.shD, st.shTmax, stack, t, ts); hitS = make_float2(t, __int_as_float(nee_verdict(st.shO, st.shD, st.lightP, t, prim))); }
        if (st.flags & F_PATH) { float t; const int prim = trace_closest<false>(sc, st.pathO, st.pathD, primary_tmax(cam, b, sid, st.flags), stack, t, ts); hitP = make_float2(t, __int_as_float(prim)); }
        }
        if (shade_step(sc, cam, prm, b, sid, st, hitP, hitS, hitA)) break;
    }
    write_mean(b, prm, sid, st);
}

// The wf_shade instantiation for one step: every one the pipeline launches is named here, 6 for each of the three camera types.
template <class Cam>
static auto shade_kernel(bool two, int phase) -> void (*)(DevScene, Cam, DevParams, WfBuf, int, int, int, int)
{
    if (phase == 1) return two ? wf_shade<4, true, 1, true, Cam> : wf_shade<4, false, 1, true, Cam>;
    if (phase == 2) return two ? wf_shade<4, true, 2, true, Cam> : wf_shade<4, false, 2, true, Cam>;
    return two ? wf_shade<4, true, 0, false, Cam> : wf_shade<4, false, 0, false, Cam>;
}

// ---------------------------------------------------------------------------------------
// Parity hooks for the integrator's sub-functions (include/pt_api.h: pt_dbg_pixel_dir, pt_dbg_nee): the SAME device
// functions the render kernels call (pt_shade.h), run on rows of inputs so that tests can compare them with the oracle
// one function at a time.
// ---------------------------------------------------------------------------------------
__global__ void dbg_ray_setup(const float* __restrict__ dir3, int n, float* __restrict__ out5)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    f3 inv; float cscale; bool deg;
    ray_setup(f3(dir3[3 * i], dir3[3 * i + 1], dir3[3 * i + 2]), inv, cscale, deg);
    out5[5 * i] = inv.x; out5[5 * i + 1] = inv.y; out5[5 * i + 2] = inv.z; out5[5 * i + 3] = cscale; out5[5 * i + 4] = deg ? 1.f : 0.f;
}
__global__ void dbg_pixel_dir(DevCamera cam, const int* __restrict__ pxpypass, int n, float* __restrict__ out8)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int px = pxpypass[3 * i], py = pxpypass[3 * i + 1], pass = pxpypass[3 * i + 2];
    Rng rng;
    rng.init((uint64_t)(int64_t)(py * cam.W + px + pass * cam.W * cam.H));      // srcs/pathtracer.cu:70-71
    float u1, u2;
    const f3 d = pixel_direction(cam, px, py, rng, u1, u2);
    float* o = out8 + (size_t)i * 8;
    o[0] = u1; o[1] = u2; o[2] = d.x; o[3] = d.y; o[4] = d.z; o[5] = rng.uniform(); o[6] = 0.f; o[7] = 0.f;      // o[5]: the next draw (RNG position)
}

// in5: surface point p.xyz | seed lo | seed hi (uint32 bits).  out12: light index | lightP.xyz | pdfLight | cosA | shadow-ray t_max |
// closest-hit primitive of the shadow ray (int bits) | Le.xyz (GetLightColor) | next uniform draw.
__global__ __launch_bounds__(kBlockThreads)
void dbg_nee(DevScene sc, const float* __restrict__ in5, int n, float* __restrict__ out12)
{
    __shared__ int lds_stack[kWavesPerBlock][kStackDepth * 64];
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    int* stack = &lds_stack[threadIdx.x >> 6][threadIdx.x & 63];
    if (i >= n) return;
    const float* r = in5 + (size_t)i * 5;
    const f3 p(r[0], r[1], r[2]);
    Rng rng;
    rng.init(((uint64_t)__float_as_uint(r[4]) << 32) | (uint64_t)__float_as_uint(r[3]));
    const NeeSample ns = nee_sample(sc, rng, p);
    const float tmax = length(ns.toL) + 1.0f;                               // GetLightColor, CudaUtil.cuh:152-157
    float t; TraceStats ts{0, 0, 0};
    const int prim = trace_closest<false>(sc, p, ns.wl, tmax, stack, t, ts);
    const f3 Le = nee_light_color(nee_verdict(p, ns.wl, ns.lightP, t, prim), prim_emittance(sc, prim < 0 ? 0 : prim));
    float* o = out12 + (size_t)i * 12;
    o[0] = __int_as_float(ns.li); o[1] = ns.lightP.x; o[2] = ns.lightP.y; o[3] = ns.lightP.z; o[4] = ns.pdfLight; o[5] = ns.cosA;
    o[6] = tmax; o[7] = __int_as_float(prim); o[8] = Le.x; o[9] = Le.y; o[10] = Le.z; o[11] = rng.uniform();
}

}  // namespace ptd

// ---------------------------------------------------------------------------------------
// Host driver
// ---------------------------------------------------------------------------------------
extern "C" {

// entries a ray's traversal stack can hold (LDS + global overflow); a 4-wide walk needs at most 3 per level + 2
int ptk_wf_stack_capacity(void) { return ptd::kWfLdsStack + ptd::kWfOvfLevels; }

// ---- work buffer: [ staging (the per-pass means) | what carve() lays out | 256 spare ] ----------------------
static size_t carved_bytes(size_t nStreams, int traceBlocks)
{
    const size_t n16 = (nStreams + 3) & ~(size_t)3;
    size_t b = 0;
    b += n16 * 16 * 11;                       // 11 float4 state arrays
    b += n16 * 16 * 2 * ptd::kRayKinds;       // ray_o/ray_d per kind
    b += n16 * 8 * (ptd::kRayKinds + 1);      // hits per kind + the cached camera-ray hit
    b += n16 * 4 * (2 + ptd::kRayKinds);      // active x2, one ray queue per kind
    b += 3 * ptd::kWfSlotBytes; // counters
    b += (size_t)traceBlocks * 256 * ptd::kWfOvfLevels * 4;
    b += 2 * ((nStreams / 4 + 1024) * ptd::kSuspInts * 4 + 16);
    b += n16 + 16;                            // res: one byte per live-list position (early shade)
    return b + 512;
}
static size_t staging_bytes(size_t nStreams) { return ((nStreams * 12 + 16) + 255) & ~(size_t)255; }

size_t ptk_wf_work_bytes(size_t nUnits, int traceBlocks)
{
    return staging_bytes(nUnits * 64) + carved_bytes(nUnits * 64, traceBlocks) + 256;
}

static void carve(char* p, size_t nStreams, int traceBlocks, ptd::WfBuf& b)
{
    const size_t n16 = (nStreams + 3) & ~(size_t)3;
    auto take = [&](size_t bytes) { char* q = p; p += (bytes + 15) & ~(size_t)15; return q; };
    b.rng0 = (uint4*)take(n16 * 16); b.rng1 = (uint4*)take(n16 * 16);
    b.weight = (float4*)take(n16 * 16); b.rad = (float4*)take(n16 * 16); b.pix = (float4*)take(n16 * 16);
    b.dir0 = (float4*)take(n16 * 16); b.wb = (float4*)take(n16 * 16);
    b.radA = (float4*)take(n16 * 16); b.wbA = (float4*)take(n16 * 16);
    b.lp = (float4*)take(n16 * 16); b.lpA = (float4*)take(n16 * 16);      // back to back: wf_trace reads lp[(kind - 1) n16 + stream]
    for (int k = 0; k < ptd::kRayKinds; k++) { b.ray_o[k] = (float4*)take(n16 * 16); b.ray_d[k] = (float4*)take(n16 * 16); }
    for (int k = 0; k < ptd::kRayKinds; k++) b.hit[k] = (float2*)take(n16 * 8);
    b.hit0 = (float2*)take(n16 * 8);
    for (int k = 0; k < 2; k++) b.active[k] = (uint32_t*)take(n16 * 4);
    for (int k = 0; k < ptd::kRayKinds; k++) b.rq[k] = (uint32_t*)take(n16 * 4);
    b.cnt = (ptd::WfCounters*)take(3 * ptd::kWfSlotBytes);
    b.ovf = (int*)take((size_t)traceBlocks * 256 * ptd::kWfOvfLevels * 4);
    b.suspCap = (uint32_t)(nStreams / 4 + 1024);
    for (int k = 0; k < 2; k++) b.susp[k] = (int*)take((size_t)b.suspCap * ptd::kSuspInts * 4);
    b.res = (uint8_t*)take(n16);
}

const float* ptk_wf_staging(void* work) { return (const float*)work; }

// What the pipeline still reads from the environment, ONCE per process: the node budget of wf_trace, which tests set to force time
// slicing, and the choice of its diagnostic build.  None of them can change a result.  Defaults are the measured
// optima on MI355X.
struct WfTuning {
    int budgetShift;     // PTAMD_BS   node budget = clamp(n >> BS, BM, 1024) steps per launch
    int budgetMin;       // PTAMD_BM
    int lateBudget;      // PTAMD_LB   node steps after which a ray is suspended once the queue is dry and its wave holds at most two rays: 64 (0 = never).
                         // An 8-way rank's big launches wait 15 us on average (20 % of them > 25 us, 3 % > 100 us) for the latest of their 64 stripes of
                         // waves — one ray of several hundred steps, alone on its SIMD (tools/straggler_cost.py, r03_b41.log); cut there it goes on in
                         // the next launch among full waves, and no iteration is added: 4-way rank +3 %, 8-way +0.4 ... +2.5 %, configs[2] / [3] / [4]
                         // +0.3 / +0.5 / +1.2 % (32: -4 %, 48 / 96 / 128 within 1 % of 64; r03_b42.log, r03_b43.log)
    bool tracePool;      // PTAMD_TPOOL with PTAMD_TSTAT=2: also the pooled per-wave histograms (tools/wave_exit_hist.py) — their atomics lengthen the launch tail
    int traceDump;       // PTAMD_TDUMP with PTAMD_TSTAT=2: the wf_trace launch (iteration) whose waves are dumped one by one (pt_dbg_trace_timeline -3003 / -3004)
    int traceStat;       // PTAMD_TSTAT 1 trip counters + histograms (slower build), 2 timeline only (production code path), 3 trip counters + section clocks
};
static const WfTuning& wf_tuning()
{
    static const WfTuning t = [] {
        auto num = [](const char* name, long long def) -> long long { const char* v = getenv(name); return v ? atoll(v) : def; };
        WfTuning w;
        w.budgetShift = (int)num("PTAMD_BS", 14); w.budgetMin = (int)num("PTAMD_BM", ptd::kWfBudget);
        w.lateBudget = (int)num("PTAMD_LB", 64);
        w.traceStat = (int)num("PTAMD_TSTAT", 0);
        w.traceDump = (int)num("PTAMD_TDUMP", -1);
        w.tracePool = num("PTAMD_TPOOL", 0) != 0;
        return w;
    }();
    return t;
}
// The rest of the schedule is fixed; each figure is the measured optimum.
// wf_shade runs 512-thread workgroups, two per CU; other shapes: 256 threads -4 %, 384 / 768 -13 %, 1024 -8 % (r02_t16_shade_shapes_after_noslp.log)
constexpr int kShadeBlock = 512;
// wf_shade's early phase runs one-wave workgroups: one free wave slot is enough (512 / 256 / 128 / 64 threads -> 0.488 / 0.481 / 0.473 / 0.472 s for an 8-way rank)
constexpr int kEarlyBlock = 64;
// wf_shade: may a stream whose path has just ended start its next sample in the same step (a second trip through the bounce code)?
// It saves one iteration per sample but doubles the step's dependent chain: shadeRounds 0 / 1 forces it (pt_set_shade_rounds,
// PTAMD_TR), -1 switches to it below this many live streams.  The result does not depend on it (pt_stream.h: shade_step_t).
constexpr uint32_t kTwoRoundsBelow = 4000000;
constexpr int kDrainSpread = 3;      // wf_drain: at most every 2^this-th lane carries a stream
int ptk_wf_trace_stat(void) { return wf_tuning().traceStat; }

}  // extern "C"

// One launch of wf_trace<MODE, PUBLISH> for iteration `it`.  A diagnostic build also gets the counter buffer and the launch's slot of its
// timeline (later launches share the last one); the production kernel has no such argument (pt_trace_probe.h).
template <int MODE, bool PUBLISH = false>
static void launch_trace(const ptd::WfJob& job, const ptd::WfBuf& b, int blocks, int ovfStride, int it, const WfTuning& tn)
{
    using namespace ptd;
    const typename TraceProbe<MODE>::Args probeArgs{job.traceStat, it < kStatLaunches ? it : kStatLaunches - 1};
    hipLaunchKernelGGL((wf_trace<MODE, PUBLISH>), dim3(blocks), dim3(256), 0, job.stream, *job.scene, b, it % 3, ovfStride, it & 1, tn.budgetShift, tn.budgetMin, tn.lateBudget, probeArgs);
}

// The pipeline for one job whose streams take their pixel and camera from `cam` (DevCamera: a frame share or a tile list; ViewTable; RayTable):
// `init` launches the kind's init kernel, and every later launch names the Cam instantiation of its kernel.
// Blocks the host until the render has drained (it polls the live-stream count every 16..64 iterations; every 16 with wf_drain off).
template <class Cam, class Init>
static hipError_t pipeline(const ptd::WfJob& job, const ptd::WfBuf& b, const Cam& cam, Init init)
{
    using namespace ptd;
    const DevParams& prm = job.prm;
    const hipStream_t stream = job.stream, aux = job.lent->aux;
    const hipEvent_t *toAux = job.lent->toAux, *toMain = job.lent->toMain;
    uint32_t* const h_cnt = job.lent->h_poll;
    hipError_t e;
    const size_t nStreams = (size_t)prm.n_units * 64;
    if ((e = hipMemsetAsync(b.cnt, 0, 3 * kWfSlotBytes, stream)) != hipSuccess) return e;
    const int nb = (int)((nStreams + 255) / 256);
    init(dim3(nb), (uint32_t)nStreams);
    const int ovfStride = job.traceBlocks * 256;
    const int tb = job.traceBlocks < nb ? job.traceBlocks : nb;
    // every sample needs at most max_bounce + (max_refract + 2) bounces, +1 iteration to retire
    // (time-sliced rays add iterations; 64x is far beyond anything a finite tree can need)
    const long long hardCap = ((long long)prm.spp_per_pass * (prm.max_bounce + prm.max_refract + 3) + 8) * 64;
    const WfTuning& tn = wf_tuning();
    if (job.traceStat && tn.traceStat == 2 && tn.tracePool) {
        static const unsigned long long one = 1ull;
        if ((e = hipMemcpyAsync(job.traceStat + 5, &one, 8, hipMemcpyHostToDevice, stream)) != hipSuccess) return e;
    }
    if (job.traceStat && tn.traceStat == 2 && tn.traceDump >= 0) {
        // diagnostic: wf_trace dumps a record per wave for this one launch (the word was cleared with the rest of the buffer by the caller)
        static unsigned long long dumpWord; dumpWord = (unsigned long long)tn.traceDump + 1ull;
        if ((e = hipMemcpyAsync(job.traceStat + 6, &dumpWord, 8, hipMemcpyHostToDevice, stream)) != hipSuccess) return e;
    }
    // early shade (wf_shade PHASE 1 / 2): for a render of few enough streams that the traversal's launch tail is a large part of
    // every iteration (one rank of an 8-way tile split), the shade step starts on `aux` beside the draining wf_trace and the rest
    // follows both (result-neutral).  Decided once per render: a large render gains nothing from it in its last iterations.
    // (not below ~1/8 of the limit either: a render that small is bound by launch latency, and this adds a launch and two waits per iteration)
    const bool early = job.earlyBelow > 0 && nStreams <= (size_t)job.earlyBelow && nStreams >= (size_t)job.earlyBelow / 8 && !job.traceStat;
    // the production kernel (it publishes its hits when the early phase reads them), or the diagnostic build PTAMD_TSTAT names
    const auto trace = job.traceStat ? (tn.traceStat == 3 ? launch_trace<3> : tn.traceStat == 1 ? launch_trace<1> : launch_trace<2>) : early ? launch_trace<0, true> : launch_trace<0>;
    int it = 0;
    int poll = 16;
    // streams only ever retire, so the live count of the last poll bounds every later one: the shade grid
    // shrinks with it instead of launching thousands of workgroups that find nothing to do
    uint32_t liveBound = (uint32_t)nStreams;
    for (;;) {
        for (int k = 0; k < poll; k++, it++) {
            const int sIn = it % 3, sOut = (it + 1) % 3, sClr = (it + 2) % 3;
            const bool timed = job.trace_ev && it < job.trace_ev_triples;
            if (timed) (void)hipEventRecord(job.trace_ev[3 * it], stream);
            if (early) {
                // aux may start once the previous iteration's shade (everything on `stream` so far) is done
                if ((e = hipEventRecord(toAux[it & 1], stream)) != hipSuccess) return e;
                if ((e = hipStreamWaitEvent(aux, toAux[it & 1], 0)) != hipSuccess) return e;
            }
            trace(job, b, tb, ovfStride, it, tn);
            if (timed) (void)hipEventRecord(job.trace_ev[3 * it + 1], stream);
            const dim3 sg((liveBound + kShadeBlock - 1) / kShadeBlock), sb(kShadeBlock);
            const bool twoRounds = job.shadeRounds >= 0 ? (job.shadeRounds != 0) : (liveBound < kTwoRoundsBelow);
            // one launch for every instantiation of wf_shade
            auto shade = [&](int phase, hipStream_t s, dim3 g, dim3 blk) {
                hipLaunchKernelGGL(shade_kernel<Cam>(twoRounds, phase), g, blk, 0, s, *job.scene, cam, prm, b, sIn, sOut, sClr, it & 1);
            };
            if (early) {
                // phase 1 in small workgroups: a 256-thread workgroup needs one free wave slot per SIMD, i.e. two traversal workgroups of
                // the CU gone, a 512-thread one four — it gets onto the chip earlier in the drain
                shade(1, aux, dim3((liveBound + kEarlyBlock - 1) / kEarlyBlock), dim3(kEarlyBlock));
                if ((e = hipEventRecord(toMain[it & 1], aux)) != hipSuccess) return e;
                if ((e = hipStreamWaitEvent(stream, toMain[it & 1], 0)) != hipSuccess) return e;
                shade(2, stream, sg, sb);
            }
            else shade(0, stream, sg, sb);
            if (timed) (void)hipEventRecord(job.trace_ev[3 * it + 2], stream);      // [3it+1, 3it+2] brackets this iteration's wf_shade
        }
        if ((e = hipGetLastError()) != hipSuccess) return e;
        if ((e = hipMemcpyAsync(h_cnt, &b.cnt[it % 3].nActive, 4, hipMemcpyDeviceToHost, stream)) != hipSuccess) return e;
        if ((e = hipStreamSynchronize(stream)) != hipSuccess) return e;
        const uint32_t live = *h_cnt;
        if (live == 0) break;
        liveBound = live;
        if (live <= (uint32_t)job.drainBelow) {
            // few streams left: finish them in one launch instead of hundreds of latency-bound iterations
            // the 4-wide tree if its walk fits the per-lane stack (any tree the builder makes for the config scenes does), else the binary one
            const bool quadWalk = 3 * job.scene->quad_depth + 2 <= kDrainQuadStack;
            // 2 (4-wide walk: 189 VGPRs) or 3 (165) waves per SIMD of wf_drain fit: spread the streams over at most that many lanes
            const size_t drainLanes = (size_t)((quadWalk && DRAIN_MINBLOCKS < 3) ? 2 : 3) * 4 * 256 * 64;
            int spread = 0;
            while (spread < kDrainSpread && ((size_t)live << (spread + 1)) <= drainLanes) spread++;
            const int db = (int)((((size_t)live << spread) + kBlockThreads - 1) / kBlockThreads);
            hipLaunchKernelGGL((quadWalk ? wf_drain<true, Cam> : wf_drain<false, Cam>), dim3(db), dim3(kBlockThreads), 0, stream, *job.scene, cam, prm, b, it % 3, it & 1, spread);
            if ((e = hipGetLastError()) != hipSuccess) return e;
            if ((e = hipStreamSynchronize(stream)) != hipSuccess) return e;
            break;
        }
        if (it > hardCap) return hipErrorLaunchFailure;      // cannot happen for a well-formed scene; never spin forever
        // with wf_drain off the render ends at the first poll that finds no stream alive, and every iteration launched after the last
        // stream retired is an empty one: keep looking every 16, so that at most 15 of them are launched (and counted: pt_last_iterations)
        if (poll < 64 && job.drainBelow != 0) poll *= 2;
        if (job.drainBelow > 0 && (unsigned long long)live <= (unsigned long long)job.drainBelow * 8ull) poll = 16;      // near the hand-over: look again soon
    }
    *job.iters = it;
    *job.trace_ev_used = job.trace_ev ? (it < job.trace_ev_triples ? it : job.trace_ev_triples) : 0;
    return hipSuccess;
}

extern "C" {

// Runs the whole pipeline for one job (pt_internal.h: WfJob) on the caller's stream and blocks the host until the render has drained.
// The pixel source is decided here, once: its init kernel and its camera type.
hipError_t ptk_wf_render(const ptd::WfJob& job)
{
    using namespace ptd;
    const hipStream_t stream = job.stream;
    const DevParams& prm = job.prm;
    const WfSource& src = job.src;
    const size_t nStreams = (size_t)prm.n_units * 64;
    WfBuf b{};
    carve((char*)job.work + staging_bytes(nStreams), nStreams, job.traceBlocks, b);
    b.staging = (float*)job.work;
    hipError_t e;
    if ((e = hipEventRecord(job.ev_begin, stream)) != hipSuccess) return e;
    switch (src.kind) {
    case WfSource::kFrame:
        e = pipeline(job, b, src.frame.cam, [&](dim3 g, uint32_t n) { hipLaunchKernelGGL(wf_init, g, dim3(256), 0, stream, *job.scene, src.frame.cam, prm, b, n); });
        break;
    case WfSource::kTileList:
        e = pipeline(job, b, src.list.cam, [&](dim3 g, uint32_t n) { hipLaunchKernelGGL(wf_init_list, g, dim3(256), 0, stream, *job.scene, src.list.cam, prm, b, n, src.list.tiles); });
        break;
    case WfSource::kViews: {
        const ViewTable views{src.views.org, (uint32_t)prm.n_tiles_total};
        e = pipeline(job, b, views, [&](dim3 g, uint32_t n) { hipLaunchKernelGGL(wf_init_views, g, dim3(256), 0, stream, *job.scene, prm, b, n, src.views.cams, src.views.firstPass, views.tilesPerView); });
        break;
    }
    case WfSource::kRays:
        e = pipeline(job, b, RayTable{src.rays.rays8}, [&](dim3 g, uint32_t n) { hipLaunchKernelGGL(wf_init_rays, g, dim3(256), 0, stream, *job.scene, prm, b, n, src.rays.rays8, src.rays.seed, (uint32_t)src.rays.seedStride, src.rays.nRays); });
        break;
    }
    if (e != hipSuccess) {
        // nothing of a failed run left running: callers free the work buffer on that path, and kernels already launched — the
        // early-shade ones on the auxiliary stream too — may still be using it.  The first error is what is returned.
        (void)hipStreamSynchronize(stream);
        (void)hipStreamSynchronize(job.lent->aux);
        return e;
    }
    return hipEventRecord(job.ev_end, stream);
}

hipError_t ptk_dbg_ray_setup(const float* dir3, int n, float* out5, hipStream_t stream)
{
    const int nb = (n + 255) / 256;
    if (nb > 0) hipLaunchKernelGGL(ptd::dbg_ray_setup, dim3(nb), dim3(256), 0, stream, dir3, n, out5);
    return hipGetLastError();
}
hipError_t ptk_dbg_pixel_dir(const ptd::DevCamera* cam, const int* pxpypass, int n, float* out8, hipStream_t stream)
{
    const int nb = (n + 255) / 256;
    if (nb > 0) hipLaunchKernelGGL(ptd::dbg_pixel_dir, dim3(nb), dim3(256), 0, stream, *cam, pxpypass, n, out8);
    return hipGetLastError();
}
hipError_t ptk_dbg_nee(const ptd::DevScene* sc, const float* in5, int n, float* out12, hipStream_t stream)
{
    const int nb = (n + ptd::kBlockThreads - 1) / ptd::kBlockThreads;
    if (nb > 0) hipLaunchKernelGGL(ptd::dbg_nee, dim3(nb), dim3(ptd::kBlockThreads), 0, stream, *sc, in5, n, out12);
    return hipGetLastError();
}

}  // extern "C"
