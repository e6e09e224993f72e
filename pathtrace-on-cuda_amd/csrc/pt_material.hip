// pt_material.hip — changing the materials and the set of lights of an uploaded scene in place (include/pt_api.h: "Materials and
// lights of an uploaded scene").
//
// A render reads a material in two places only: floats 36..47 of the surface record, and the `lights` array with its two kernel
// arguments n_lights and nee_prune.  No traversal array depends on a material, so nothing of the trees is touched.
//   * mat_apply (phase A), one thread per triangle: the twelve floats go into the surface record; the light test and the
//     emittance test of pt_scene_create (csrc/pt_scene.hip: pack_surfaces, emittance_ok) are taken, and every block leaves its
//     number of lights and the AND of its emittance tests in a partials array;
//   * mat_scan, one workgroup: exclusive scan of the block counts in place; the total and the combined flag go to the word the
//     host reads — they are kernel arguments of every later render, and they size the `lights` array, so the host waits here, once;
//   * mat_lights (phase B), one thread per triangle: light k (in ascending triangle index: block offset + rank inside the block,
//     from a ballot) gets its 64-byte record from the scene's position mirror with the expressions of the vertex update
//     (pt_dyn_device.h: write_light), and its entry in the light -> triangle map that update reads.
// A kernel boundary is the only ordering between two workgroups; there are no atomics, and the same input gives the same bytes.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <utility>

#include "pt_scene.h"
#include "pt_dyn_device.h"

namespace {

// What the three kernels share.  `partial`: one (lights, emittance ok) pair per block, turned into (first light slot, ok) by the scan,
// and one more pair at the end: (number of lights, ok of the whole scene).
struct MatScene {
    float4* surf;                // surface records, 12 x float4 per triangle
    const float* pos;            // the scene's position mirror, 9 floats per triangle
    float4* lights;              // phase B: room for every light the scan counted
    int32_t* light_prim;         // phase B: the same number of entries
    int2* partial;
    int32_t n_tris, n_blocks, cap_lights;
};

// pack_surfaces' light test on one material, float32, every operation rounded once; NaN makes no light
__device__ __forceinline__ bool is_light(float ex, float ey, float ez) { return sqrtf((ex * ex + ey * ey) + ez * ez) > 0.0001f; }
// emittance_ok's test: finite, >= 0, <= 1e8 (a NaN or an infinity fails a comparison)
__device__ __forceinline__ bool emit_ok(float e) { return e >= 0.f && e <= 1e8f; }

// the number of set flags in the waves before this one, and in the whole block; lds: one word per wave
__device__ __forceinline__ int2 block_offsets(unsigned long long mask, int* lds)
{
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) lds[wave] = __popcll(mask);
    __syncthreads();
    int before = 0, all = 0;
    for (int w = 0; w < kMatBlock / 64; w++) { const int c = lds[w]; all += c; if (w < wave) before += c; }
    return make_int2(before, all);
}

__global__ __launch_bounds__(kMatBlock) void mat_apply(MatScene m, const float* __restrict__ mat)
{
    __shared__ int cnt[kMatBlock / 64];
    __shared__ int bad[kMatBlock / 64];
    const int i = blockIdx.x * kMatBlock + threadIdx.x;
    bool light = false, ok = true;
    if (i < m.n_tris) {
        const float* src = mat + (size_t)i * 12;      // the caller's pointer: 4-byte alignment is all it promises
        float v[12];
        for (int k = 0; k < 12; k++) v[k] = src[k];
        float4* rec = m.surf + (size_t)i * 12 + 9;      // floats 36..47
        rec[0] = make_float4(v[0], v[1], v[2], v[3]);
        rec[1] = make_float4(v[4], v[5], v[6], v[7]);
        rec[2] = make_float4(v[8], v[9], v[10], v[11]);
        light = is_light(v[0], v[1], v[2]);
        ok = emit_ok(v[0]) && emit_ok(v[1]) && emit_ok(v[2]);
    }
    const unsigned long long notOk = __ballot(!ok);
    if ((threadIdx.x & 63) == 0) bad[threadIdx.x >> 6] = notOk != 0ull;
    const int2 c = block_offsets(__ballot(light), cnt);      // its barrier covers `bad` as well
    if (threadIdx.x == 0) {
        int anyBad = 0;
        for (int w = 0; w < kMatBlock / 64; w++) anyBad |= bad[w];
        m.partial[blockIdx.x] = make_int2(c.y, anyBad ? 0 : 1);
    }
}

__global__ __launch_bounds__(256) void mat_scan(MatScene m)
{
    __shared__ int sums[4];
    __shared__ int oks[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int carry = 0, okAll = 1;
    for (int base = 0; base < m.n_blocks; base += 256) {
        const int idx = base + (int)threadIdx.x;
        const int2 p = idx < m.n_blocks ? m.partial[idx] : make_int2(0, 1);
        int v = p.x;      // inclusive scan inside the wave
        for (int off = 1; off < 64; off <<= 1) {
            const int t = __shfl_up(v, off, 64);
            if (lane >= off) v += t;
        }
        const int okWave = __all(p.y != 0);
        if (lane == 63) { sums[wave] = v; oks[wave] = okWave; }
        __syncthreads();
        int before = 0, all = 0;
        for (int w = 0; w < 4; w++) { all += sums[w]; if (w < wave) before += sums[w]; okAll &= oks[w]; }
        if (idx < m.n_blocks) m.partial[idx] = make_int2(carry + before + v - p.x, p.y);
        carry += all;
        __syncthreads();      // the next round writes sums / oks again
    }
    if (threadIdx.x == 0) m.partial[m.n_blocks] = make_int2(carry, okAll);
}

__global__ __launch_bounds__(kMatBlock) void mat_lights(MatScene m)
{
    __shared__ int cnt[kMatBlock / 64];
    const int i = blockIdx.x * kMatBlock + threadIdx.x;
    bool light = false;
    if (i < m.n_tris) {
        const float4 e = m.surf[(size_t)i * 12 + 9];      // the emittance phase A stored
        light = is_light(e.x, e.y, e.z);
    }
    const unsigned long long mask = __ballot(light);
    const int rank = (int)__builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0u));
    const int2 c = block_offsets(mask, cnt);
    const int slot = m.partial[blockIdx.x].x + c.x + rank;
    if (light && slot < m.cap_lights) {      // slot < the scan's total <= cap_lights by construction
        ptd::write_light(m.lights + (size_t)slot * 4, ptd::load_tri(m.pos, i));
        m.light_prim[slot] = i;
    }
}

bool spheres_emit_ok(const PtScene* s)
{
    for (int i = 0; i < s->dev.n_spheres; i++) {
        const float* e = &s->h_spheres[(size_t)i * 16 + 4];
        for (int k = 0; k < 3; k++) if (!(std::isfinite(e[k]) && e[k] >= 0.f && e[k] <= 1e8f)) return false;
    }
    return true;
}

void set_nee_prune(PtScene* s) { s->dev.nee_prune = (s->tri_emit_ok && spheres_emit_ok(s) && pt_prune_allowed()) ? 1 : 0; }

// room for `count` elements of `elem` bytes in b, byte count of the scene kept; the old block goes only once the new one exists
hipError_t grow(PtScene* s, DevBuf& b, int count, size_t elem)
{
    if (b && b.bytes() >= (size_t)count * elem) return hipSuccess;
    DevBuf fresh;
    const hipError_t e = fresh.alloc((size_t)count * elem);
    if (e != hipSuccess) return e;
    s->bytes += (int64_t)fresh.held() - (int64_t)b.held();
    b = std::move(fresh);      // the old block is freed with `fresh`
    return hipSuccess;
}

}  // namespace

extern "C" {

int pt_scene_update_materials(PtScene* s, const float* d_mat12, void* hip_stream)
{
    if (!s || !d_mat12) { pt_set_error("pt_scene_update_materials: NULL %s", !s ? "scene" : "d_mat12"); return PT_ERR_INVALID; }
    HIPCHK(hipSetDevice(s->device));
    int rc;
    if ((rc = pt_dyn_prepare(s)) != PT_OK) return rc;
    hipStream_t st = (hipStream_t)hip_stream;
    MatScene m;
    m.surf = s->dyn.surf; m.pos = s->dyn_buf[kDynPos].as<const float>(); m.partial = s->dyn_buf[kDynMatPartial].as<int2>();
    m.n_tris = s->dev.n_tris; m.n_blocks = (m.n_tris + kMatBlock - 1) / kMatBlock;
    m.lights = nullptr; m.light_prim = nullptr; m.cap_lights = 0;
    hipLaunchKernelGGL(mat_apply, dim3((unsigned)m.n_blocks), dim3(kMatBlock), 0, st, m, d_mat12);
    hipLaunchKernelGGL(mat_scan, dim3(1), dim3(256), 0, st, m);
    HIPCHK(hipGetLastError());
    // the one wait: the number of lights and the flag are kernel arguments of every later render, and the number sizes `lights`
    HIPCHK(hipMemcpyAsync(s->h_mat, m.partial + m.n_blocks, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    const int n_lights = s->h_mat[0];
    s->tri_emit_ok = s->h_mat[1] != 0;
    if (n_lights > 0) {
        // nothing on the device reads the old blocks: the stream is idle, and the scene runs one update, query or render at a time
        HIPCHK(grow(s, s->arr[kArrLights], n_lights, 64));
        HIPCHK(grow(s, s->dyn_buf[kDynLightPrim], n_lights, 4));
        m.lights = s->arr[kArrLights].as<float4>(); m.light_prim = s->dyn_buf[kDynLightPrim].as<int32_t>(); m.cap_lights = n_lights;
        s->dev.lights = s->dyn.lights = m.lights;
        s->dyn.light_prim = m.light_prim;
        hipLaunchKernelGGL(mat_lights, dim3((unsigned)m.n_blocks), dim3(kMatBlock), 0, st, m);
        HIPCHK(hipGetLastError());
    }
    s->n_lights = s->dev.n_lights = s->dyn.n_lights = n_lights;
    set_nee_prune(s);
    return PT_OK;
}

int pt_scene_update_materials_host(PtScene* s, const float* h_mat12)
{
    if (!s || !h_mat12) { pt_set_error("pt_scene_update_materials_host: NULL %s", !s ? "scene" : "h_mat12"); return PT_ERR_INVALID; }
    HIPCHK(hipSetDevice(s->device));
    DevBuf d_mat;
    HIPCHK(d_mat.upload(h_mat12, (size_t)s->dev.n_tris * 48));
    const int rc = pt_scene_update_materials(s, d_mat.as<float>(), nullptr);
    if (rc != PT_OK) return rc;
    HIPCHK(hipStreamSynchronize(nullptr));
    return PT_OK;
}

int pt_scene_update_sphere_materials(PtScene* s, const PtSphere* h_spheres, int32_t n_spheres)
{
    if (!s || !h_spheres) { pt_set_error("pt_scene_update_sphere_materials: NULL %s", !s ? "scene" : "h_spheres"); return PT_ERR_INVALID; }
    if (n_spheres != s->dev.n_spheres || n_spheres < 1) {
        pt_set_error("pt_scene_update_sphere_materials: %d spheres given, the scene has %d", n_spheres, s->dev.n_spheres);
        return PT_ERR_INVALID;
    }
    HIPCHK(hipSetDevice(s->device));
    static_assert(sizeof(PtSphere) == 64, "a sphere record is the PtSphere itself");
    memcpy(s->h_spheres.data(), h_spheres, (size_t)n_spheres * 64);      // pt_scene_update_spheres checks against these from now on
    HIPCHK(hipMemcpy(s->arr[kArrSpheres].as<>(), s->h_spheres.data(), (size_t)n_spheres * 64, hipMemcpyHostToDevice));      // ordered on the NULL stream
    set_nee_prune(s);
    return PT_OK;
}

int32_t pt_scene_nee_prune(const PtScene* s) { return s ? s->dev.nee_prune : 0; }

}  // extern "C"
