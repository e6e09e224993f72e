// oracle/curand_shim.h — TEST INFRASTRUCTURE ONLY.  Written for this repository.
//
// The one header the reference's integrator (include/CudaUtil.cuh, include/Bxdf.cuh) needs that this image does not
// have: <curand_kernel.h>.  oracle/Makefile copies this file to oracle/_ref/fwd/curand_kernel.h (next to an empty
// curand.h) for the build of oracle/_ref/ptref_int, so the reference's headers compile unmodified where they lie.
//
// The engine is this repository's RNG contract, not cuRAND's: XORWOW with rocRAND's seed scramble
// (/opt/rocm/include/rocrand/rocrand_xorwow.h), subsequence 0 and offset 0 — curand_init's second and third arguments
// are ignored —, uniform = 2.3283064e-10f + x * 2.3283064e-10f in (0, 1].  tests/golden/ref_rocrand_xorwow.npz
// (rocRAND's own engine on the host) pins it through `ptref_int rng`.  Every draw is counted so the driver can report
// how many a function consumed.
#ifndef PTAMD_CURAND_SHIM_H
#define PTAMD_CURAND_SHIM_H

#include <cassert>
#include <cfloat>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <iostream>

#include <device_launch_parameters.h>   // the real header: threadIdx / blockIdx / blockDim / gridDim (CudaUtil.cuh:50-58, never called)

struct curandStateXORWOW {
    unsigned int x[5];
    unsigned int d;
    long long draws;
};
typedef curandStateXORWOW curandState;
typedef curandStateXORWOW curandState_t;

static inline void curand_init(unsigned long long seed, unsigned long long /*subsequence*/, unsigned long long /*offset*/, curandState* s)
{
    s->x[0] = 123456789U; s->x[1] = 362436069U; s->x[2] = 521288629U; s->x[3] = 88675123U; s->x[4] = 5783321U;
    s->d = 6615241U;
    const unsigned int s0 = (unsigned int)seed ^ 0x2c7f967fU;
    const unsigned int s1 = (unsigned int)(seed >> 32) ^ 0xa03697cbU;
    const unsigned int t0 = 1228688033U * s0;
    const unsigned int t1 = 2073658381U * s1;
    s->x[0] += t0; s->x[1] ^= t0; s->x[2] += t1; s->x[3] ^= t1; s->x[4] += t0;
    s->d += t1 + t0;
    s->draws = 0;
}

static inline unsigned int curand(curandState* s)
{
    const unsigned int t = s->x[0] ^ (s->x[0] >> 2);
    s->x[0] = s->x[1]; s->x[1] = s->x[2]; s->x[2] = s->x[3]; s->x[3] = s->x[4];
    s->x[4] = (s->x[4] ^ (s->x[4] << 4)) ^ (t ^ (t << 1));
    s->d += 362437U;
    s->draws++;
    return s->d + s->x[4];
}

static inline float curand_uniform(curandState* s)
{
    return 2.3283064e-10f + (float)curand(s) * 2.3283064e-10f;
}

#endif
