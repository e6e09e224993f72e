// pt_trace_probe.h — what the diagnostic builds of wf_trace (PTAMD_TSTAT) measure, kept out of the kernel's loop.
//
// wf_trace<MODE> owns one TraceProbe<MODE> and calls its hooks at fixed points of the loop; the production build (MODE 0) gets the empty
// specialisation at the bottom, so nothing of this file reaches its code.  The other builds:
//   MODE 1  trip counters, the per-step and per-ray histograms (one atomic each: a slower build), section clocks, launch timeline
//   MODE 2  the production code path plus the launch timeline; for one chosen launch (PTAMD_TDUMP; stat[6] = launch + 1) a record per
//           wave and a per-trip log of every kStatLogEvery-th wave; with PTAMD_TPOOL (stat[5] != 0) the pooled per-wave histograms
//   MODE 3  trip counters and section clocks, no per-step atomics
// Everything goes to the counter buffer whose sections pt_device.h lays out (kStat*); tools/*.py read them by position.
#pragma once
#include <hip/hip_runtime.h>
#include "pt_device.h"
#include "pt_math.h"

namespace ptd {

template <int MODE>
struct TraceProbe {
    static constexpr bool STAT = MODE == 1 || MODE == 3, HIST = MODE == 1;
    // the kernel argument: the counter buffer and this launch's slot of its timeline
    struct Args { unsigned long long* stat; int launch; };

    unsigned long long* const stat;
    const int launch;
    const unsigned long long t0;      // wave start, 100 MHz
    unsigned long long tExh = 0;      // when this wave found the queue dry
    unsigned long long clk[5] = {0, 0, 0, 0, 0}, mark = 0;      // STAT: shader clocks in refill / vote + budget / node step / triangle step / ray epilogue
    unsigned long long nodeTrips = 0, nodeLanes = 0, triTrips = 0, triLanes = 0, refills = 0, refillLanes = 0, noRayLanes = 0, rays = 0;
    unsigned int trips = 0, tripsDry = 0;      // MODE 2: trips of this wave in all, and after it found the queue dry
    // MODE 2, the dumped launch: a record per wave (kStatWaves) and a per-trip log of every kStatLogEvery-th wave
    const bool dump;
    const uint32_t wave;
    const bool log;
    uint32_t w0 = 0, w1 = 0, atomics = 0, took = 0;      // trip log: time and shader clock at the top of the loop, queue atomics and rays taken in this trip
    uint32_t* logAt = nullptr;

    PT_DEV explicit TraceProbe(const Args& a)
        : stat(a.stat), launch(a.launch), t0(__builtin_amdgcn_s_memrealtime()),
          dump(MODE == 2 && a.stat[6] == (unsigned long long)a.launch + 1ull), wave(blockIdx.x * 4u + (threadIdx.x >> 6)),
          log(dump && wave % kStatLogEvery == 0 && wave / kStatLogEvery < (uint32_t)kStatLogWaves) {}

    PT_DEV uint32_t ticks() const { return (uint32_t)((__builtin_amdgcn_s_memrealtime() - t0) & 0xfffffull); }      // 10-ns ticks since the wave started, 20 bits
    PT_DEV void section(int k) { if (STAT) { const unsigned long long now = __builtin_amdgcn_s_memtime(); clk[k] += now - mark; mark = now; } }

    PT_DEV void trip_top()
    {
        if (STAT) mark = __builtin_amdgcn_s_memtime();
        w0 = 0; w1 = 0; atomics = 0; took = 0;
        // A = top of the loop, on the constant 100 MHz clock, and the shader clock counter at the same moment (their ratio is the clock the SIMD runs at)
        if (MODE == 2 && log) { w0 = ticks(); w1 = (uint32_t)__builtin_amdgcn_s_memtime(); }
    }
    PT_DEV void queue_atomic() { if (MODE == 2) atomics++; }
    PT_DEV void queue_dry() { tExh = __builtin_amdgcn_s_memrealtime(); }
    PT_DEV void refilled(uint32_t take)
    {
        if (STAT && take) { refills++; refillLanes += take; }
        if (MODE == 2) took = take;
    }
    PT_DEV void after_refill() { section(0); }
    // a trip that serves at least one ray begins (every lane of the wave calls this)
    PT_DEV void trip_begins(bool hasRay, int pend, bool exhausted, int lane)
    {
        if (MODE != 2) return;
        trips++; if (exhausted) tripsDry++;
        logAt = nullptr;
        if (log && 4 * trips <= (unsigned)kStatLogTrips) {
            // four words per trip (10-ns ticks since the wave started in the low 20 bits).  w0: A, top of the loop | lanes with a ray (7 bits) | queue
            // already dry | queue atomics of the refill (2 bits, saturating); w1: the shader clock counter at A (low 32 bits);
            // w2: C, after the refill | rays taken (7) | some lane holds a leaf; w3: D, node data of a node trip arrived (0 for a triangle trip)
            const uint32_t lanesNow = (uint32_t)__builtin_popcountll(__ballot(hasRay)), pendNow = (uint32_t)__builtin_popcountll(__ballot(hasRay && pend != 0));
            logAt = (uint32_t*)(stat + kStatWords + (size_t)kStatWaves * 8) + (size_t)(wave / kStatLogEvery) * kStatLogTrips + 4 * (trips - 1);
            if (lane == 0) {
                logAt[0] = w0 | (lanesNow << 20) | (exhausted ? 1u << 27 : 0u) | ((atomics > 3u ? 3u : atomics) << 28);
                logAt[1] = w1;
                logAt[2] = ticks() | ((took > 127u ? 127u : took) << 20) | (pendNow ? 1u << 27 : 0u);
                logAt[3] = 0u;
            }
        }
    }
    // the wave has voted for a node trip or a triangle trip (lanes with a ray call this)
    PT_DEV void after_vote(bool doNode, int nNode, int nTri, bool hasRay)
    {
        if (STAT) {
            if (doNode) { nodeTrips++; nodeLanes += nNode; } else { triTrips++; triLanes += nTri; }
            noRayLanes += 64 - __builtin_popcountll(__ballot(hasRay));
        }
        section(1);
    }
    // the four words of a node have been asked for: the trip log wants the moment they arrive
    PT_DEV void node_arrived(uint4& n0, uint4& n1, uint4& n2, uint4& n3)
    {
        if (MODE == 2 && logAt) {
            asm volatile("s_waitcnt vmcnt(0)" : "+v"(n0.x), "+v"(n1.x), "+v"(n2.x), "+v"(n3.x) :: "memory");
            logAt[3] = ticks();      // every lane of the node trip writes the same word
        }
    }
    PT_DEV void after_node(int sp) { if (HIST) atomicAdd(&stat[kStatDepthHist + (sp > 31 ? 31 : sp)], 1ull); }      // stack depth after this node step
    PT_DEV void after_step(bool doNode) { section(doNode ? 2 : 3); }
    PT_DEV void ray_end(int steps)
    {
        rays++;
        // node steps of this ray (this launch), bins of 4.  steps < 0: the ray spent its budget while the suspend pool was full and carried
        // on — the last bin, never an index below the buffer
        if (HIST) atomicAdd(&stat[kStatStepHist + ((steps < 0 || steps >= 252) ? 63 : steps >> 2)], 1ull);
    }
    PT_DEV void trip_ends() { section(4); }

    // n: rays of this launch
    PT_DEV void wave_end(uint32_t n, int lane)
    {
        // per-lane ray count -> wave total
        unsigned long long r = rays;
        for (int o = 32; o > 0; o >>= 1) r += __shfl_xor(r, o);
        if (lane != 0) return;
        if (dump) {
            // the dumped launch: one record per wave and none of the pooled statistics below (their atomics on a few hot words come from
            // every wave as it leaves, i.e. all through the launch tail that is being looked at)
            if (wave < (uint32_t)kStatWaves) {
                unsigned long long* w = stat + kStatWords + (size_t)wave * 8;
                w[0] = t0; w[1] = tExh; w[2] = __builtin_amdgcn_s_memrealtime(); w[3] = trips; w[4] = tripsDry; w[5] = r;
                w[6] = __builtin_amdgcn_s_getreg(4 | (31 << 11));       // HW_ID: wave slot [3:0], SIMD [5:4], CU [11:8], SH [12], SE [15:13]
                w[7] = __builtin_amdgcn_s_getreg(20 | (31 << 11));      // XCC_ID
            }
            return;
        }
        if (STAT) { atomicAdd(&stat[0], nodeTrips); atomicAdd(&stat[1], nodeLanes); atomicAdd(&stat[2], triTrips); atomicAdd(&stat[3], triLanes); }
        // launch timeline (100 MHz ticks): earliest wave start, earliest "queue empty", latest wave exit
        // MODE 2 keeps it in kStatStripes copies and nothing else unless stat[5] asks for the pooled histograms (PTAMD_TPOOL=1): atomics from
        // every leaving wave on a handful of words stretched the very tail they were meant to measure (r03_b27.log: a launch of 100 us
        // became one of 287 us)
        unsigned long long* tl = MODE == 2 ? stat + kStatStripeOff / 8 + 3 * ((size_t)launch * kStatStripes + (blockIdx.x % kStatStripes)) : stat + kStatTimeline + 3 * (size_t)launch;
        const unsigned long long tEnd = __builtin_amdgcn_s_memrealtime();
        atomicMax(&tl[0], ~t0); if (tExh) atomicMax(&tl[1], ~tExh); atomicMax(&tl[2], tEnd);
        if (blockIdx.x == 0 && threadIdx.x == 0) stat[kStatLaunchRays + launch] = n;
        if (MODE == 2 && stat[5] == 0ull) return;
        // distribution of wave exit times over the launch, all launches pooled (absolute: 32 us bins)
        const unsigned long long dtk = (tEnd - t0) / 3200ull;      // 100 MHz ticks
        atomicAdd(&stat[kStatLifeHist + (dtk < 31 ? dtk : 31)], 1ull);
        if (MODE == 2) {
            // per-wave work, all launches pooled: trips per wave (64 bins of 4), trips after the wave found the queue dry (32 bins of 2: in the
            // slots of MODE 1's per-ray histograms), and rays per wave summed into stat[7] / trips into stat[0] for averages
            atomicAdd(&stat[kStatStepHist + (trips >= 252 ? 63 : trips >> 2)], 1ull);
            atomicAdd(&stat[kStatDepthHist + (tripsDry >= 62 ? 31 : tripsDry >> 1)], 1ull);
            atomicAdd(&stat[7], r); atomicAdd(&stat[0], (unsigned long long)trips); atomicAdd(&stat[2], (unsigned long long)tripsDry);
        }
        if (STAT) {
            atomicAdd(&stat[4], refills); atomicAdd(&stat[5], refillLanes); atomicAdd(&stat[6], noRayLanes); atomicAdd(&stat[7], r);
            for (int k = 0; k < 5; k++) atomicAdd(&stat[kStatClocks + k], clk[k]);
        }
    }
};

// the production build: no argument, no state, no code
template <>
struct TraceProbe<0> {
    struct Args { __host__ __device__ Args(unsigned long long*, int) {} };
    PT_DEV explicit TraceProbe(const Args&) {}
    PT_DEV void trip_top() {}
    PT_DEV void queue_atomic() {}
    PT_DEV void queue_dry() {}
    PT_DEV void refilled(uint32_t) {}
    PT_DEV void after_refill() {}
    PT_DEV void trip_begins(bool, int, bool, int) {}
    PT_DEV void after_vote(bool, int, int, bool) {}
    PT_DEV void node_arrived(uint4&, uint4&, uint4&, uint4&) {}
    PT_DEV void after_node(int) {}
    PT_DEV void after_step(bool) {}
    PT_DEV void ray_end(int) {}
    PT_DEV void trip_ends() {}
    PT_DEV void wave_end(uint32_t, int) {}
};

}  // namespace ptd
