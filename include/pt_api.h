/* include/pt_api.h — C-ABI drop-in boundary of the MI355X-native path tracer.
 *
 * One shared library (libptamd.so, built from pathtrace-on-cuda_amd/) exports exactly the
 * entry points below.  Plain pointers and sizes only: no C++ types, no torch types.
 * Citations `file:line` are relative to the reference tree (WaterPlease/PathTrace-on-CUDA).
 * INTEGRATION.md shows the reference-side adaptor (`PathTracer::Render` re-implemented on
 * top of these calls) a maintainer would add.
 *
 * Every function returns PT_OK (0) or a negative PtStatus and records a message that
 * pt_last_error() returns (thread-local).  The reference's own convention for GPU errors
 * — print to stderr, reset the device, exit(99) (include/CudaUtil.cuh:28-36) — is kept by
 * the C++ adaptor `PathTracer::Render` (pathtrace-on-cuda_amd/host/ref_surface.cpp), not
 * imposed on C callers.
 */
#ifndef PT_API_H
#define PT_API_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PT_API __attribute__((visibility("default")))

typedef enum PtStatus {
    PT_OK = 0,
    PT_ERR_INVALID = -1,      /* bad argument / inconsistent scene */
    PT_ERR_NO_LIGHT = -2,     /* no emissive triangle: `curand(s) % Nl` is UB in the reference (include/CudaUtil.cuh:235) */
    PT_ERR_DEVICE = -3,       /* HIP runtime error (message carries hipGetErrorString) */
    PT_ERR_IO = -4,           /* file could not be read / written */
    PT_ERR_UNSUPPORTED = -5   /* e.g. BVH deeper than the traversal stack */
} PtStatus;

/* ----------------------------------------------------------------------------------
 * Host scene types: byte-compatible mirrors of the reference's host structs, so the
 * adaptor can pass `bvh->primitives.data()` straight through.
 * -------------------------------------------------------------------------------- */
typedef struct PtVec3 { float x, y, z; } PtVec3;                 /* glm::vec3 */
typedef struct PtVec2 { float x, y; } PtVec2;                    /* glm::vec2 */

typedef struct PtMaterialOnCPU {                                 /* include/mesh.h:11-19 */
    PtVec3 emittance, albedo, specular;
    float opacity, metallic, roughness;
} PtMaterialOnCPU;

typedef struct PtVertex {                                        /* include/mesh.h:21-37, 112 B */
    PtVec3 Position, Normal;
    PtVec2 TexCoords;
    PtVec3 Tangent, Bitangent;
    PtMaterialOnCPU mat;
    float u, v;
} PtVertex;

typedef struct PtPrimitive { PtVertex v1, v2, v3; } PtPrimitive; /* include/bvh.h:8-13, 336 B */

typedef struct PtMaterial {                                      /* include/CudaPrimitive.cuh:15-23, 48 B */
    float emittance[3], albedo[3], specular[3];
    float opacity, roughness, metallic;
} PtMaterial;

typedef struct PtSphere {                                        /* include/CudaPrimitive.cuh:249-323 (data members), 64 B */
    float center[3];
    float rad;
    PtMaterial mat;
} PtSphere;

typedef struct PtBVHNode {                                       /* CudaBVHNode, include/CudaPrimitive.cuh:237-247, 40 B */
    float bMin[3], bMax[3];
    int32_t childL, childR;                                      /* -1 = none */
    int32_t primStart, primEnd;                                  /* inclusive range, -1 = interior */
} PtBVHNode;

/* Flattened triangle = the data members of the reference's `Triangle`
 * (include/CudaPrimitive.cuh:217-234) after Triangle::Copy, without the vptr.  352 B. */
typedef struct PtTriangle {
    float V0[3], V1[3], V2[3];
    float T0[3], T1[3], T2[3];
    float B0[3], B1[3], B2[3];
    float N0[3], N1[3], N2[3];
    float normal[3], E1[3], E2[3];
    float u0, v0, u1, v1, u2, v2;
    PtMaterial mat0, mat1, mat2;
    float area;
} PtTriangle;

typedef struct PtCamera {                                        /* what PathTracer::Render reads, srcs/pathtracer.cu:128-129,193-198 */
    float pos[3];
    float forward[3], up[3], right[3];                           /* Camera::GetForward/GetUp/GetRight */
    float fovy_deg;                                              /* Camera::fovy (degrees) */
    float aspect;                                                /* Camera::aspect */
    int32_t W, H;                                                /* Camera::Screen_W / Screen_H */
} PtCamera;

typedef struct PtParams {                                        /* the reference's compile-time tunables, include/CudaUtil.cuh:15-19 */
    int32_t passes;           /* NUM_MULTI_SAMPLE (8)   */
    int32_t spp_per_pass;     /* NUM_SAMPLE (1024)      */
    int32_t max_bounce;       /* MAX_BOUNCE (8)         */
    int32_t rr_bounce;        /* RUSSIAN_ROULETTE_BOUNCE (3) */
    float   rr_floor;         /* PROB_STOP_BOUNCE (0.5).  Not validated: the roulette keeps a path with probability q = (m > floor) ? m : floor, m = min(maxcomp(weight), 1),
                               * the reference's select-style max.  NaN: q is NaN and the path ends at the roulette; a negative floor is the same as 0;
                               * above 1 the path always survives and its weight shrinks by 1 / floor per bounce. */
    int32_t max_refract;      /* the literal 8 of `RefractCnt++>8`, include/CudaUtil.cuh:354 */
    int32_t first_pass;       /* SampleIDX of the first pass of this call (seed = offset + SampleIDX*W*H, srcs/pathtracer.cu:71) */
    /* Tile split (new; the reference is single-device).  The frame is cut into 8x8-pixel
     * tiles numbered row-major; this call renders tiles t with t % world == rank.
     * world = 1, rank = 0 renders the whole frame. */
    int32_t rank, world;
} PtParams;

PT_API void pt_params_default(PtParams* p);                      /* the reference's values */

PT_API const char* pt_last_error(void);
PT_API const char* pt_version(void);

/* ----------------------------------------------------------------------------------
 * (a1,a2) Host acceleration-structure build + flatten.
 * Replaces SAHBVH::GenBVHTree (srcs/bvh.cpp:426-511) followed by LoadFromBVH
 * (srcs/CudaPrimitive.cu:8-145) and the Triangle::Copy loop (srcs/pathtracer.cu:164-166).
 * -------------------------------------------------------------------------------- */
typedef struct PtFlatBVH PtFlatBVH;
PT_API int  pt_bvh_build_sah(const PtPrimitive* prims, int32_t n_prims, PtFlatBVH** out);
PT_API void pt_bvh_free(PtFlatBVH* b);
PT_API int32_t pt_bvh_num_nodes(const PtFlatBVH* b);
PT_API int32_t pt_bvh_num_tris(const PtFlatBVH* b);
PT_API int32_t pt_bvh_max_depth(const PtFlatBVH* b);             /* "Maximum depth of tree", CudaPrimitive.cu:144 */
PT_API const PtBVHNode*  pt_bvh_nodes(const PtFlatBVH* b);       /* == CudaBVH  */
PT_API const PtTriangle* pt_bvh_tris(const PtFlatBVH* b);        /* == CudaPrims after Copy */

/* ----------------------------------------------------------------------------------
 * (a3) Scene upload.  Replaces the cudaMallocManaged + host-fill block of
 * PathTracer::Render (srcs/pathtracer.cu:142-188).  `device` is the HIP device ordinal.
 * The scene owns its HBM allocations until pt_scene_destroy.
 * -------------------------------------------------------------------------------- */
typedef struct PtScene PtScene;
PT_API int  pt_scene_create(const PtBVHNode* nodes, int32_t n_nodes,
                            const PtTriangle* tris, int32_t n_tris,
                            const PtSphere* spheres, int32_t n_spheres,
                            int32_t device, PtScene** out);
PT_API void pt_scene_destroy(PtScene* s);
PT_API int32_t pt_scene_num_lights(const PtScene* s);            /* "ADD light" count, pathtracer.cu:167-173 */
PT_API int64_t pt_scene_device_bytes(const PtScene* s);

/* ----------------------------------------------------------------------------------
 * (a3-a11) Render.  Replaces the StartRender launch loop (srcs/pathtracer.cu:236-246).
 *
 * pt_render_tiles: device-resident; all GPU work is enqueued on `hip_stream` (a hipStream_t, may be NULL) and ordered after
 *   whatever the caller enqueued there before.  Writes this rank's tiles, tile-major, into d_tiles:
 *     d_tiles[((lt * 64) + (ty*8+tx)) * 3 + c],  lt = local tile index (global tile
 *     t = lt*world + rank), float32, size pt_tiles_floats().  Value = sum over the call's
 *     passes of the per-pass mean radiance (the reference's `image[offset] += mean`,
 *     pathtracer.cu:81), starting from 0.  d_work is scratch of pt_work_bytes() bytes.
 *   BLOCKING in the default render path (mode 1, the queue-driven pipeline): the number of bounce iterations is
 *   data-dependent, so the call polls the live-stream count (a 4-byte read-back + hipStreamSynchronize every 16-64
 *   iterations) and returns only when the render has drained; on return only the final pass-sum kernel may still be
 *   running on `hip_stream`.  As blocking as the reference's own Render (cudaDeviceSynchronize after every launch,
 *   srcs/pathtracer.cu:236-246).  A caller that drives several scenes or GPUs from one process gives each its own host
 *   thread.  Mode 0 (pt_set_mode, the one-kernel state machine) is fully asynchronous.  One render at a time per PtScene
 *   (the scene owns the pinned poll word, events and counters the render uses); different scenes are independent.
 * pt_untile: scatter gathered tile buffers (rank-major: world buffers of
 *   pt_tiles_floats() each) into a row-major W*H*3 frame, on the device.
 * pt_render: convenience, whole frame (world=1) into a host buffer, synchronous;
 *   h_accum_rgb[W*H*3] is overwritten.
 * -------------------------------------------------------------------------------- */
PT_API int64_t pt_tiles_floats(const PtCamera* cam, const PtParams* prm);
PT_API int64_t pt_work_bytes(const PtCamera* cam, const PtParams* prm);
PT_API int  pt_render_tiles(PtScene* s, const PtCamera* cam, const PtParams* prm,
                            float* d_tiles, void* d_work, void* hip_stream);
PT_API int  pt_untile(const float* d_gathered, const PtCamera* cam, int32_t world,
                      float* d_frame_rgb, void* hip_stream);
PT_API int  pt_render(PtScene* s, const PtCamera* cam, const PtParams* prm, float* h_accum_rgb);
/* Duration of the most recent pt_render_tiles launch sequence on this scene, measured with
 * HIP events on the stream it was launched on (ms), and the kernel's own work counters. */
PT_API int  pt_last_render_ms(PtScene* s, float* ms);
/* Durations (ms) of the most recent render_units launches on this scene (up to 64, oldest
 * first), each measured with a HIP event pair recorded on the launch stream around that
 * kernel only.  Returns the count written (<= cap) or a negative PtStatus; reset != 0 clears
 * the history.  Blocks until those launches have finished. */
PT_API int  pt_render_timings(PtScene* s, float* ms_out, int32_t cap, int32_t reset);

/* ----------------------------------------------------------------------------------
 * (e) Multi-GPU exchange (new: the reference is single-device, srcs/pathtracer.cu:124-259).  One process per GPU; rank r
 * renders tiles t % world == r with pt_render_tiles, then ONE collective — a gather of the tile buffers to rank 0,
 * RCCL ncclGather (rccl.h:745) over xGMI — and pt_untile on rank 0 assemble the frame.  No torch, no MPI needed:
 *   rank 0:  pt_comm_unique_id(id) and hand the 128 bytes to the other processes (any channel), or let
 *            pt_comm_create_from_file do it through a file for the processes of one node;
 *   all:     pt_comm_create(id, rank, world, device, &comm); ... pt_render_tiles(...);
 *            pt_gather_frame(comm, d_tiles, &cam, &prm, d_gathered, d_frame, stream);   (both asynchronous on `stream`)
 * world == 1 never loads RCCL (the gather is a device copy).  INTEGRATION.md shows the 8-process C++ use.
 * -------------------------------------------------------------------------------- */
#define PT_COMM_ID_BYTES 128
typedef struct PtComm PtComm;
PT_API int  pt_comm_unique_id(uint8_t id[PT_COMM_ID_BYTES]);
PT_API int  pt_comm_create(const uint8_t id[PT_COMM_ID_BYTES], int32_t rank, int32_t world, int32_t device, PtComm** out);
/* Rendezvous through a file for the processes of one node: rank 0 removes any file at `path`, writes { world, job_tag, id },
 * joins and removes the file again; ranks > 0 wait (timeout_s) for a file carrying THEIR world and job_tag — the file of an
 * earlier job is ignored.  job_tag = any value the ranks of one job share and other jobs do not (launcher pid, job id).
 * pt_comm_create_from_file = the same with job_tag 0.  ncclCommInitRank itself has no timeout: a rank that never arrives
 * leaves the others waiting in it, as with any RCCL program. */
PT_API int  pt_comm_create_from_file_tagged(const char* path, uint64_t job_tag, int32_t rank, int32_t world, int32_t device, int32_t timeout_s, PtComm** out);
PT_API int  pt_comm_create_from_file(const char* path, int32_t rank, int32_t world, int32_t device, int32_t timeout_s, PtComm** out);
PT_API void pt_comm_destroy(PtComm* c);
PT_API int32_t pt_comm_rank(const PtComm* c);
PT_API int32_t pt_comm_world(const PtComm* c);
/* d_gathered: rank 0 only (NULL elsewhere), world x n_floats floats, rank-major — what pt_untile reads. */
PT_API int  pt_gather_tiles(PtComm* c, const float* d_tiles, int64_t n_floats, float* d_gathered, void* hip_stream);
PT_API int  pt_gather_frame(PtComm* c, const float* d_tiles, const PtCamera* cam, const PtParams* prm,
                            float* d_gathered, float* d_frame_rgb, void* hip_stream);
/* The multi-GPU sibling of pt_render for hosts without HIP code of their own: this rank's tiles, the gather, and on rank 0 the
 * assembled frame in h_accum_rgb[W*H*3] (ignored elsewhere).  Rank and world come from the communicator; the scene must live on the
 * communicator's device.  Synchronous.  Before the gather the ranks exchange a 4-byte status (max all-reduce): if ANY rank failed to
 * render its tiles, EVERY rank returns an error and nobody waits in the gather. */
PT_API int  pt_render_split(PtScene* s, const PtCamera* cam, const PtParams* prm, PtComm* c, float* h_accum_rgb);

/* ----------------------------------------------------------------------------------
 * First-hit feature buffers ("AOVs") and a feature-guided denoiser (new: the reference has neither).
 * Opt-in and separate from the render: they read only the scene's immutable data, never a render's state, and leave every
 * frame of pt_render / pt_render_tiles / pt_render_split as it is.
 *
 * pt_render_aov: for every pixel of the FULL frame, the camera ray of the first path of each pass first_pass + j of the call
 *   (j = 0 .. passes-1; the ray pt_dbg_pixel_dir reproduces, origin cam->pos, t_max 999999), traced to its closest hit.
 *   Writes pt_aov_floats() floats, 8 per pixel, row-major (d_aov[(py*W + px)*8 + k]), float32 sums in pass order and one
 *   IEEE division at the end:
 *     k 0..2  sum of the hit material's albedo / passes          (a miss adds 0)
 *     k 3..5  sum of the ray-facing shading normal / passes      (not renormalised; a miss adds 0)
 *     k 6     sum of t over the hitting samples / their number   (0 if none)
 *     k 7     hits / passes                                      (coverage)
 *   d_prim (may be NULL): int32 per pixel, the primitive the ray of pass first_pass hit (triangles, then spheres, as
 *   pt_dbg_raycast's out_prim), -1 for a miss.  Only prm->passes and prm->first_pass are read: rank, world, spp_per_pass and
 *   the bounce settings are ignored, the buffer is always the whole frame.  Asynchronous on `hip_stream`; d_aov 16-byte aligned.
 * pt_aov: the same into host buffers (h_prim may be NULL), synchronous.
 *
 * pt_denoise: edge-avoiding a-trous wavelet filter (Dammertz et al. 2010) with albedo demodulation, guided by the AOVs.
 *   d_rgb is a row-major W*H*3 frame as pt_render returns it (the sum over passes of per-pass means, NaN pixels allowed);
 *   d_out receives a frame of the same shape and scale (pt_tonemap_u8(out, sample_cnt) works unchanged).  Definition:
 *     c_p = rgb_p / sample_cnt;  div_p = albedo_p where > 1e-3, else 1 (per channel; 1 without demodulation);  e_p = c_p / div_p
 *     finite_p = all three components of c_p (after an iteration: of e_p) are finite
 *     iteration i = 0 .. L-1, step s = 2^i, taps q = p + s*(dx, dy), dx, dy in -2..2, inside the frame and finite_q:
 *       w = h(dx) h(dy) exp(-E),  h = (1/16, 1/4, 3/8, 1/4, 1/16),  w = 0 exactly when E > 80
 *       E = |e_p - e_q|^2 / (sigma_color^2 4^-i)   (left out when !finite_p)
 *         + |n_p - n_q|^2 / sigma_normal^2          (n = AOV 3..5)
 *         + |z_p - z_q| / (sigma_depth max(z_p, z_q)) (z = AOV 6; 0 when both are 0)
 *     e_p <- sum w e_q / sum w (kept when sum w = 0: a NaN pixel with a finite neighbour becomes finite, a NaN never spreads)
 *     out_p = e_p * div_p * sample_cnt after L iterations;  L = 0 copies d_rgb bit for bit.
 *   All of it in float32, every operation rounded once (tests/denoise_ref.py: denoise32 restates it; on inputs whose every exp
 *   argument is 0 the result is that restatement's bit for bit).  The edges of the definition:
 *     - the albedo is compared in float32 against the float32 nearest 1e-3 (0x3A83126F = 0.001000000047...): an albedo of exactly
 *       that value, or below it, divides by 1; the next float above divides by itself.
 *     - the cutoff is inclusive: a tap with E == 80 is used, the next float above is not.  A tap whose E is NaN is not used.
 *     - a pixel whose normal has a NaN (a zero-area triangle's normal, pt_scene_update_vertices below) has a NaN E against every
 *       tap, itself included: sum w = 0 and it keeps its value.  It is no tap of another pixel either, as that pixel's E against it
 *       is NaN.  A depth of +inf does the same (inf - inf at the centre tap, inf / inf against a finite neighbour).
 *     - max(z_p, z_q) is z_p > z_q ? z_p : z_q, and the depth term is added only when that is > 0: a pair with max <= 0 (misses,
 *       negative depths) adds no depth term.  A NaN depth is therefore no edge where it is the max (as a tap, and at its own centre
 *       tap) and a NaN E against the positive depths around it when it is the centre: give misses depth 0, not NaN.
 *     - kc = 1 / (sigma_color * sigma_color), times 4 per iteration, in float32.  A sigma_color whose square overflows (> 1.8e19)
 *       makes kc zero: the colour term is switched off.  One whose square underflows to 0, or is small enough that kc overflows
 *       (at once below 5.4e-20, after i iterations below 2^i times that), makes kc infinite: the centre tap's 0 * inf is NaN, no
 *       tap is used and from that iteration on the filter keeps every finite pixel (a non-finite one has no colour term).
 *     - sample_cnt is converted to float32 once (2^24 + 1 becomes 2^24, 2^31 - 1 becomes 2^31).
 *   d_work: pt_denoise_work_bytes(W, H) bytes; d_aov and d_work 16-byte aligned; d_out must not overlap d_rgb, d_aov or d_work,
 *   and the inputs are not modified.  Asynchronous on `hip_stream`.
 * pt_denoise_host: the same on host buffers, on HIP device `device`, synchronous.
 * Bad arguments (NULL pointers, W or H < 2, sample_cnt <= 0, iterations outside 0..12, a sigma <= 0, overlapping buffers)
 * return PT_ERR_INVALID before any HIP call.
 * -------------------------------------------------------------------------------- */
typedef struct PtDenoiseParams {
    int32_t iterations;       /* L, 0..12 (default 5: steps 1..16, a 125-pixel footprint) */
    float   sigma_color;      /* default 16 (chosen on 4-pass x 1-spp frames) */
    float   sigma_normal;     /* default 0.1 */
    float   sigma_depth;      /* default 0.1 (relative depth difference) */
    int32_t demodulate;       /* 1: filter colour / albedo, remodulate afterwards (default) */
} PtDenoiseParams;

PT_API int64_t pt_aov_floats(const PtCamera* cam);                /* W * H * 8, or -1 */
PT_API int  pt_render_aov(PtScene* s, const PtCamera* cam, const PtParams* prm, float* d_aov, int32_t* d_prim, void* hip_stream);
PT_API int  pt_aov(PtScene* s, const PtCamera* cam, const PtParams* prm, float* h_aov, int32_t* h_prim);
PT_API void pt_denoise_params_default(PtDenoiseParams* p);
PT_API int64_t pt_denoise_work_bytes(int32_t W, int32_t H);         /* 48 * W * H, or -1 */
PT_API int  pt_denoise(const float* d_rgb, const float* d_aov, int32_t W, int32_t H, int32_t sample_cnt, const PtDenoiseParams* p,
                       float* d_out, void* d_work, void* hip_stream);
PT_API int  pt_denoise_host(int32_t device, const float* h_rgb, const float* h_aov, int32_t W, int32_t H, int32_t sample_cnt,
                            const PtDenoiseParams* p, float* h_out);

/* ----------------------------------------------------------------------------------
 * Feature buffers and the denoiser for a pixel window, a batch of views and the caller's rays (csrc/pt_aov.hip).
 * Opt-in: every call above is as it was.  The eight floats per pixel and the filter are those of the section above; these calls extend
 * where they can be applied, not what they compute.  Like pt_render_aov they read only the scene's data, never a render's state,
 * and follow the rule in force for every call that takes a scene: one render, update or query at a time per scene.
 *
 * pt_render_aov_window: the row-major (y1 - y0) x (x1 - x0) x 8 buffer of the half-open window [x0, x1) x [y0, y1), bit for bit
 *   pt_render_aov(...)[y0:y1, x0:x1]; d_prim (may be NULL) likewise.  Only the 8x8 tiles that overlap the window are traced.  The
 *   window must lie inside the frame as pt_tiles_of_window requires, else PT_ERR_INVALID.  Asynchronous on `hip_stream`, allocates
 *   nothing and reads nothing back: enqueued after pt_scene_update_vertices or a tree rebuild on the same stream it sees their result.
 *   pt_aov_window_floats: (y1 - y0) * (x1 - x0) * 8, or -1.
 * pt_render_aov_views: n_views cameras of one size (HOST arrays as in pt_render_views; h_first_pass may be NULL: prm->first_pass for
 *   every view).  Output is view-major: view v's slice d_aov[v * W*H*8 ..] is bit for bit pt_render_aov(s, &h_cams[v], prm with
 *   first_pass = first of v, ...); d_prim[v * W*H ..] likewise.  Checked on the host before any HIP call: n_views >= 1, equal W, H >= 2,
 *   every h_first_pass[v] >= 0, the seed limit for every view's first + passes, and n_views * W * H <= 2^28.  As in pt_render_aov only
 *   passes and first_pass of prm are read.  The cameras go into the buffer the scene owns for pt_render_views (grown on demand — the one
 *   allocation these calls may make; pt_scene_device_bytes does not count it).  The call WAITS for `hip_stream` ONCE, until that table
 *   has been copied from the host (as pt_untile_list waits for its list): h_cams and h_first_pass are free when it returns; the kernel
 *   itself is asynchronous on the stream.  One launch whatever n_views is.
 *   pt_aov_views_floats: n_views * W * H * 8, or -1.
 * pt_aov_rays: for ray i of the DEVICE buffer d_rays8 (RAY8 as in pt_trace_rays: the reserved float is not read, the direction is used as
 *   given, the range is [0, tmax]) d_aov[8 i ..] holds the hit material's albedo, the ray-facing shading normal, t and coverage 1; all
 *   eight floats are 0 for a miss.  d_prim[i] (may be NULL): the primitive, or -1.  The bits are those of fields 20..22, 8..10 and 1 of
 *   the 29-float record pt_trace_rays(PT_QUERY_CLOSEST) gives the same ray, passed through (0 + x) / 1: a ray is a pixel with one
 *   pass, and no RNG value is drawn.  d_rays8 and d_aov 16-byte aligned; n_rays >= 0, and n_rays = 0 returns PT_OK without a HIP call.
 *   Asynchronous.  With the caller's own W x H grid of rays (a panorama: ptamd.equirect_rays) the buffer is what pt_denoise takes.
 * The _host variants (pt_aov_window, pt_aov_views, pt_aov_rays_host) are the same into host buffers, synchronous, on the NULL stream.
 *
 * pt_untile_views: the view-major tile buffer of pt_render_views -> n_views row-major frames, stacked, in ONE launch; frame v is bit
 *   for bit pt_untile(d_tiles + v * T, &cam, 1, frame_v) with T = pt_tiles_floats(cam0, world 1).  Only W and H of cam0 are read.
 * pt_denoise_batch: n_frames frames of one size, stacked: d_rgb is n x H x W x 3, d_aov n x H x W x 8, d_out n x H x W x 3.  Slice k of
 *   d_out is bit for bit pt_denoise of slice k: taps never cross a frame boundary.  pt_denoise IS the batch of one frame.  Cost:
 *   iterations + 2 launches whatever n is (iterations = 0: one copy).  n_frames in 1..65535, n * W * H <= 2^28, d_work of
 *   pt_denoise_batch_work_bytes() = 48 * W * H * n bytes, and pt_denoise's argument checks with every extent multiplied by n.
 *
 * The exact windowed denoise.  A pixel of the L-iteration filter depends on pixels at most M = 2 * (2^L - 1) away in x and in y: the sum
 *   of the reaches 2 * 2^i of its iterations.  pt_denoise_margin(L) returns M (-1 outside 0..12).  pt_window_expand (host only) grows a
 *   window by `margin` on every side and clips it to the frame; margin -1 means M of the default iterations, else margin >= 0.
 *   Render the EXPANDED window (pt_render_window / pt_render_tile_list) and its feature buffers (pt_render_aov_window), run pt_denoise
 *   on that buffer and crop: with margin >= M the crop is BIT FOR BIT the crop of the full frame's pt_denoise — every tap a window
 *   pixel's value depends on lies inside the expanded window or outside the frame in both runs, and the filter's arithmetic does not
 *   depend on absolute position.  With a smaller margin the result is defined as pt_denoise of the expanded window, cropped, with no
 *   equality claim.  The price: at the default L = 5, M = 62 pixels per side — a 256 x 256 window becomes 380 x 380, 2.2 x the pixels.
 * Bad arguments return PT_ERR_INVALID (the size queries: -1) before any HIP call; pointers are not dereferenced on that path.
 * When to use, measured on an MI355X: 16 views of 240 x 136 take 0.54 ms through pt_untile_views +
 *   pt_render_aov_views + pt_denoise_batch (9 launches) against 4.9 ms per view (144 launches) — batch whenever there is more than one
 *   frame of a size.  A 256 x 256 window of a 1080p preview (4 passes x 1 spp) renders, denoises exactly and downloads in 4.0 ms, in 3.1 ms
 *   at margin 0, against 20.6 ms for the full frame's route — take the exact margin unless the window is small against 62 pixels.
 *   pt_render_aov itself runs the same kernel over the whole frame: 0.89 ms at 1080p and 1.96 ms at 4K for 8 passes.
 * -------------------------------------------------------------------------------- */
PT_API int64_t pt_aov_window_floats(const PtCamera* cam, int32_t x0, int32_t y0, int32_t x1, int32_t y1);   /* (y1-y0)*(x1-x0)*8, or -1 */
PT_API int  pt_render_aov_window(PtScene* s, const PtCamera* cam, const PtParams* prm, int32_t x0, int32_t y0, int32_t x1, int32_t y1,
                                 float* d_aov, int32_t* d_prim /* may be NULL */, void* hip_stream);
PT_API int  pt_aov_window(PtScene* s, const PtCamera* cam, const PtParams* prm, int32_t x0, int32_t y0, int32_t x1, int32_t y1,
                          float* h_aov, int32_t* h_prim /* may be NULL */);
PT_API int64_t pt_aov_views_floats(const PtCamera* cam0, int32_t n_views);                                  /* n_views*W*H*8, or -1 */
PT_API int  pt_render_aov_views(PtScene* s, const PtCamera* h_cams, int32_t n_views, const PtParams* prm, const int32_t* h_first_pass /* may be NULL */,
                                float* d_aov, int32_t* d_prim /* may be NULL */, void* hip_stream);
PT_API int  pt_aov_views(PtScene* s, const PtCamera* h_cams, int32_t n_views, const PtParams* prm, const int32_t* h_first_pass /* may be NULL */,
                         float* h_aov, int32_t* h_prim /* may be NULL */);
PT_API int  pt_aov_rays(PtScene* s, const float* d_rays8, int64_t n_rays, float* d_aov, int32_t* d_prim /* may be NULL */, void* hip_stream);
PT_API int  pt_aov_rays_host(PtScene* s, const float* h_rays8, int64_t n_rays, float* h_aov, int32_t* h_prim /* may be NULL */);
PT_API int  pt_untile_views(const float* d_tiles, const PtCamera* cam0, int32_t n_views, float* d_frames_rgb, void* hip_stream);
PT_API int64_t pt_denoise_batch_work_bytes(int32_t W, int32_t H, int32_t n_frames);                         /* 48*W*H*n, or -1 */
PT_API int  pt_denoise_batch(const float* d_rgb, const float* d_aov, int32_t W, int32_t H, int32_t n_frames, int32_t sample_cnt,
                             const PtDenoiseParams* p, float* d_out, void* d_work, void* hip_stream);
PT_API int  pt_denoise_batch_host(int32_t device, const float* h_rgb, const float* h_aov, int32_t W, int32_t H, int32_t n_frames, int32_t sample_cnt,
                                  const PtDenoiseParams* p, float* h_out);
PT_API int32_t pt_denoise_margin(int32_t iterations);                                                       /* 2 * (2^L - 1); -1 outside 0..12 */
PT_API int  pt_window_expand(const PtCamera* cam, const int32_t window[4], int32_t margin, int32_t expanded[4]);   /* host only */

/* ----------------------------------------------------------------------------------
 * Per-pixel variance across passes, an error estimate, render-to-target (new: the reference has none of them).
 * Opt-in and beside the render: these calls only READ what a render left behind, and leave every frame as it is.
 *
 * Contract of the work buffer (new): after pt_render_tiles(s, cam, prm, d_tiles, d_work, stream) the start of d_work holds the
 *   per-pass means the frame was summed from — prm->passes x pt_tiles_floats(cam, prm) float32, pass-major, each pass in the
 *   layout of d_tiles (value = pixelColor / spp_per_pass, srcs/pathtracer.cu:81; padding pixels of ragged edge tiles and of tiles
 *   past the last one are exactly 0) — in both render modes, valid until d_work is next written.  d_tiles is their sum in pass
 *   order starting from 0.
 * Why passes: the reference draws ONE jittered direction per pixel per pass and sends all spp_per_pass paths down it
 *   (srcs/pathtracer.cu:74-80), so the samples inside a pass are not independent; the per-pass means are.
 *
 * pt_accumulate_passes: folds those means into running moments, per float, S = their sum and M2 = the sum of their squared
 *   deviations from their mean, in the layout of d_tiles (pt_tiles_floats() floats each; pt_gather_frame / pt_untile move them
 *   unchanged).  cam / prm are those of the render (prm->passes means are read; rank / world as rendered); n_before = passes
 *   folded in so far (0: d_sum and d_m2 are overwritten, not read).  For pass k = n_before + 1, ... with mean m, IEEE float32:
 *     S_prev = S;  S = S_prev + m                                                  (k = 1: S = 0 + m)
 *     k >= 2:  d1 = m - S_prev / (k - 1);  d2 = m - S / k;  M2 = M2 + d1 * d2      (k = 1: M2 = 0)
 *   Welford's update with the means taken from S: S is bit for bit the frame pt_render_tiles returns for the same passes in one
 *   call, however they were split over calls.  Non-finite means propagate (the reference produces NaN pixels).
 * pt_variance: d_var = max(M2, 0) * n / (n - 1), the estimated variance of S, i.e. of the frame value pt_render returns
 *   (rounding can leave M2 a hair below 0 on a converged pixel; a NaN M2 stays NaN).  n_passes >= 2; any float count.
 * pt_error_estimate: whole-buffer figures over the pixels of this rank's tiles that lie inside the frame (hence cam and
 *   prm->rank / world; prm->passes is not read) and whose S and M2 are all finite.  Per-pixel terms in float32 as written below, summed
 *   in float64 in a fixed order (per-block partial sums in d_scratch, added up on the host; no atomics): two calls return the
 *   same bits.  The only call here that waits for the stream (it reads the partial sums back).  The order, restated in
 *   tests/stats_ref.py (estimate32): min(1024, ceil(floats / 3072)) blocks of 256 threads, each thread its groups of 4 pixels at the
 *   stride of the grid, the lanes of a wave in a shuffle tree, the four waves in order, the blocks in order on the host.
 *   Two degenerate outcomes, as the formulas give them: a buffer whose used pixels all have S = 0 and M2 = 0 (an all-black frame)
 *   has rel_rms = NaN (0 / 0) and mean_rel_se = 0; a buffer with no used pixel (pixels == 0: every in-frame pixel skipped) has NaN
 *   in both.  A caller that compares rel_rms with a target must decide what NaN means to it.
 * Buffers are caller-owned; float buffers must be 4-byte aligned and d_scratch 8-byte aligned; 16-byte aligned ones are read and
 * written with 16-byte accesses (others work, slower, and give the same bits).  Everything is enqueued on `hip_stream` on the
 * current device.  Bad arguments (NULL, a misaligned buffer, n_before < 0, n_passes < 2, camera / params that pt_tiles_floats
 * rejects) return PT_ERR_INVALID before any HIP call.
 *
 * pt_render_converge: host convenience like pt_render (whole frame, world = 1, synchronous).  Renders batches of prm->passes
 *   passes (first_pass advancing from prm->first_pass), folds each batch, estimates after each batch once two passes are in,
 *   and stops after the first batch whose rel_rms <= target_rel_rms, or at max_passes (>= 2; the last batch is shortened to
 *   fit, and prm->first_pass + max_passes must respect the seed limit of pt_render).  h_accum_rgb[W*H*3] = S, bit for bit what
 *   pt_render returns for passes = *passes_done (divide by it: pt_tonemap_u8(out, *passes_done)); h_var_rgb (may be NULL) =
 *   pt_variance of it; *est = the last estimate.  On an all-black frame rel_rms is NaN (above), NaN <= target is false, and the call
 *   runs to max_passes.  A batch costs a pipeline drain and a 40 KB read-back: measured at
 *   1080p on 8 passes x 256 spp, batches of 1 / 4 / 8 passes take 1.48 / 1.10 / 1.00 x the time of one pt_render call (DESIGN.md
 *   section 10) — use batches of 8 (4 if the finer stopping grain is worth 10 %), never 1; a tile-split version would need the
 *   ranks to agree on when to stop and is not provided (the three calls above take any rank / world).
 * -------------------------------------------------------------------------------- */
typedef struct PtErrorEstimate {
    double rel_rms;           /* sqrt( sum Var_i / sum S_i^2 ) over the floats of the pixels used: the expected relative RMS error of the frame */
    double mean_rel_se;       /* mean over the pixels used of sqrt((Var_r + Var_g) + Var_b) / (((|S_r| + |S_g|) + |S_b|) + 0.03 n):
                                 rel_rms is dominated by whatever is brightest, this figure weighs every pixel alike */
    int64_t pixels, skipped;  /* pixels used; in-frame pixels left out because S or M2 is not finite */
} PtErrorEstimate;

PT_API int  pt_accumulate_passes(const void* d_work, const PtCamera* cam, const PtParams* prm, int32_t n_before,
                                 float* d_sum, float* d_m2, void* hip_stream);
PT_API int  pt_variance(const float* d_m2, int64_t n_floats, int32_t n_passes, float* d_var, void* hip_stream);
PT_API int64_t pt_error_scratch_bytes(int64_t n_floats);           /* 40 * min(1024, ceil(n_floats / 3072)), or -1 (n_floats < 1) */
PT_API int  pt_error_estimate(const float* d_sum, const float* d_m2, const PtCamera* cam, const PtParams* prm, int32_t n_passes,
                              void* d_scratch, PtErrorEstimate* h_out, void* hip_stream);
PT_API int  pt_render_converge(PtScene* s, const PtCamera* cam, const PtParams* prm, double target_rel_rms, int32_t max_passes,
                               float* h_accum_rgb, float* h_var_rgb, int32_t* passes_done, PtErrorEstimate* est);

/* ----------------------------------------------------------------------------------
 * A pixel window or any list of tiles without the full frame (new: the reference renders whole frames only).
 * Opt-in: every call above is as it was.  A tile is the 8x8 tile of the tile split, numbered row-major over the FULL frame
 * (tile t covers pixels x = 8 (t % tiles_x) .., y = 8 (t / tiles_x) .., tiles_x = ceil(W / 8)).  Seeds depend on the pixel, the
 * pass and the full frame's W, H only, so a pixel has the same value whichever call renders it.
 *
 * pt_render_tile_list: renders the n_tiles tiles whose numbers are in the HOST array h_tiles, in any order, for passes
 *   prm->first_pass .. first_pass + passes - 1.  Output is list-major in the layout of pt_render_tiles:
 *     d_tiles[((i * 64) + (ty*8+tx)) * 3 + c] for list position i, pt_tile_list_floats(n_tiles) floats; value = sum over the
 *   call's passes of the per-pass mean starting from 0, pixels outside the frame exactly 0 — bit for bit the floats tile
 *   h_tiles[i] has in pt_render_tiles' buffer.  Checked on the host before any HIP call, else PT_ERR_INVALID: n_tiles >= 1,
 *   every entry in [0, tiles_x * tiles_y), no entry twice, prm->rank == 0 && prm->world == 1 (a caller splits a frame by making
 *   lists).  The list is copied into a buffer the scene owns (grown on demand, in stream order) and has been read when the call
 *   returns.  Otherwise pt_render_tiles' contract: one render at a time per scene, BLOCKING as mode 1 is, all GPU work on
 *   `hip_stream`; pt_last_render_ms and pt_last_iterations report it.
 *   Render mode: a list is always rendered by the queue-driven pipeline.  pt_set_mode(0), PTAMD_MODE=0, pt_enable_counters,
 *   pt_enable_trace_timing and the PTAMD_TSTAT diagnostics do not apply to it and are left as they are for the next pt_render_tiles
 *   (both modes give the same bits, so nothing is lost).
 *   Work buffer: d_work is scratch of pt_tile_list_work_bytes() bytes, and the contract of the section above holds for it —
 *   after the call its start holds the per-pass means, prm->passes x n_tiles x 192 float32, pass-major, each pass in list order
 *   in the layout of d_tiles, valid until d_work is next written.
 * pt_tile_list_work_bytes: what the render of that many tiles needs, not the full frame's figure: the pipeline's need depends
 *   on the number of work units only, so this is pt_work_bytes of any frame that has n_tiles tiles (8 n_tiles x 8 pixels, say)
 *   with the same prm — a part proportional to n_tiles x passes plus a fixed part sized by the resident traversal grid (1 tile x
 *   8 passes: 88.9 MB, against 7.94 GB for 1080p x 8 passes).  -1 for arguments pt_render_tile_list would reject.
 * pt_tiles_of_window (host only): the tiles that overlap the half-open pixel window [x0, x1) x [y0, y1), ascending.  Returns
 *   their number and writes at most `cap` of them (h_tiles may be NULL when cap is 0); a window that is empty, inverted or not
 *   inside the frame returns PT_ERR_INVALID.
 * pt_untile_list: scatters a list-major tile buffer into d_out, a row-major (y1 - y0) x (x1 - x0) x 3 buffer that stands for
 *   that window of the frame.  Pure copy, bit for bit.  Pixels of the window that no listed tile covers are NOT written, and
 *   pixels of listed tiles outside the window are dropped: with the whole frame as the window this re-renders a region into a
 *   frame one already has.  Entries are checked as above (a tile listed twice is merely written twice).  The call waits for
 *   `hip_stream` once (until the list has been read from h_tiles); the copy itself is asynchronous on it.
 * pt_render_window: host convenience like pt_render, synchronous; h_rgb[(y1 - y0) * (x1 - x0) * 3] is the window, bit for bit
 *   pt_render(...)[y0:y1, x0:x1].  prm->rank / world are ignored as pt_render ignores them.
 * Feature buffers and the denoiser of a window: pt_render_aov_window and pt_window_expand above; the moments of a list: the adaptive section below.
 * -------------------------------------------------------------------------------- */
PT_API int64_t pt_tile_list_floats(int32_t n_tiles);                /* 192 * n_tiles, or -1 */
PT_API int64_t pt_tile_list_work_bytes(const PtCamera* cam, const PtParams* prm, int32_t n_tiles);
PT_API int  pt_render_tile_list(PtScene* s, const PtCamera* cam, const PtParams* prm, const int32_t* h_tiles, int32_t n_tiles,
                                float* d_tiles, void* d_work, void* hip_stream);
PT_API int32_t pt_tiles_of_window(const PtCamera* cam, int32_t x0, int32_t y0, int32_t x1, int32_t y1, int32_t* h_tiles, int32_t cap);
PT_API int  pt_untile_list(const float* d_tiles, const int32_t* h_tiles, int32_t n_tiles, const PtCamera* cam,
                           int32_t x0, int32_t y0, int32_t x1, int32_t y1, float* d_out, void* hip_stream);
PT_API int  pt_render_window(PtScene* s, const PtCamera* cam, const PtParams* prm, int32_t x0, int32_t y0, int32_t x1, int32_t y1,
                             float* h_rgb);

/* ----------------------------------------------------------------------------------
 * A batch of camera views in one pipeline run (new: the reference renders one camera per call).
 * Opt-in: every call above is as it was.  Many small frames of one scene (a turntable, multi-view data, thumbnails) rendered one
 * after the other are bound by launch latency: the number of bounce iterations of a render does not fall with its size.  The
 * streams of all views of a batch share the iterations of ONE render.
 *
 * pt_render_views: renders the n_views cameras in the HOST array h_cams, for passes first .. first + prm->passes - 1 of each view,
 *   first = h_first_pass[v] (HOST array of n_views entries), or prm->first_pass for every view when h_first_pass is NULL.
 *   Cameras: all share W and H; pos, forward, up, right, fovy_deg and aspect are free per view.
 *   Output is view-major: d_tiles[v * T + ...], T = pt_tiles_floats(cam, world 1), pt_views_floats() floats in all.  View v's slice is
 *   bit for bit the buffer pt_render_tiles(s, &h_cams[v], prm with first_pass = first of v, rank 0, world 1) writes, padding pixels
 *   of ragged tiles exactly 0, so pt_untile(d_tiles + v * T, &h_cams[v], 1, frame_v, stream) assembles view v's frame.
 *   Work buffer: d_work is scratch of pt_views_work_bytes() bytes, and the contract of the moments section holds for it — after
 *   the call its start holds the per-pass means, prm->passes x n_views x T float32, pass-major, within a pass view-major in the
 *   layout of d_tiles, valid until d_work is next written: a caller can fold moments per view from it.
 *   Checked on the host before any HIP call, else PT_ERR_INVALID: n_views >= 1, no NULL pointer, equal W, H >= 2 across the views,
 *   prm->rank == 0 && prm->world == 1, every h_first_pass[v] >= 0, the seed limit of pt_render_tiles for every view's
 *   first + passes, and a stream count a single frame of that many tiles may have: n_views x tiles x passes work units within
 *   pt_render_tiles' own limit and 64 x that below 2^31.
 *   Otherwise pt_render_tile_list's contract: BLOCKING as mode 1 is, one render at a time per scene, all GPU work on `hip_stream`,
 *   always the queue-driven pipeline (pt_set_mode(0), pt_enable_counters and the PTAMD_TSTAT diagnostics do not apply and are
 *   left as set for the next pt_render_tiles; pt_enable_trace_timing does apply); pt_last_render_ms and pt_last_iterations report
 *   it.  pt_set_shade_rounds, pt_set_drain_threshold and pt_set_early_shade act on the batch's stream count as on a frame's.  The
 *   cameras and first passes are copied into buffers the scene owns (grown on demand, in stream order) and have been read when
 *   the call returns.
 * pt_views_floats: n_views * pt_tiles_floats(cam0, world 1), or -1.
 * pt_views_work_bytes: pt_work_bytes of a frame that has n_views x tiles tiles (8 tiles_x x 8 tiles_y n_views pixels, say) with the
 *   same prm, as pt_tile_list_work_bytes: the pipeline's need depends on the number of work units only.  -1 for arguments
 *   pt_render_views would reject.
 * pt_render_views_host: host convenience like pt_render, synchronous; h_rgb[n_views x H x W x 3], view v = pt_render of h_cams[v].
 * Feature buffers and the denoiser of a batch: pt_render_aov_views, pt_untile_views and pt_denoise_batch above.
 * Out of scope: views of different sizes, views x tile lists, a tile split of a batch over ranks.
 * -------------------------------------------------------------------------------- */
PT_API int64_t pt_views_floats(const PtCamera* cam0, int32_t n_views);
PT_API int64_t pt_views_work_bytes(const PtCamera* cam0, const PtParams* prm, int32_t n_views);
PT_API int  pt_render_views(PtScene* s, const PtCamera* h_cams, int32_t n_views, const PtParams* prm, const int32_t* h_first_pass,
                            float* d_tiles, void* d_work, void* hip_stream);
PT_API int  pt_render_views_host(PtScene* s, const PtCamera* h_cams, int32_t n_views, const PtParams* prm, const int32_t* h_first_pass,
                                 float* h_rgb);

/* ----------------------------------------------------------------------------------
 * Dynamic geometry (new: the reference uploads a scene once).  Opt-in: every call above is as it was.
 * The triangles of an uploaded scene move without a rebuild: the topology of both traversal trees is kept and every array a
 * render reads that depends on a vertex is recomputed on the GPU from the new positions (csrc/pt_dynamic.hip).  A render is
 * defined by the triangles and the reference leaf boxes only — the traversal trees steer the search — so the result is exact:
 * after an update the scene is, for every entry point, the scene pt_scene_create(nodes', tris', ...) would give.
 *
 * pt_scene_update_vertices: d_pos is a DEVICE pointer to n_tris x 9 float32, V0 V1 V2 of every triangle in the order of the
 *   `tris` array given to pt_scene_create.  d_frames is a DEVICE pointer to n_tris x 27 float32, N0 N1 N2 T0 T1 T2 B0 B1 B2
 *   (floats 9..35 of the surface record), stored as given (the caller normalises), or NULL: the shading frames are kept.
 *   tris' = tris with, in float32, every operation rounded once, in this order: V0 V1 V2 from d_pos; E1 = V1 - V0, E2 = V2 - V0;
 *   c = (E1y E2z - E1z E2y, -(E1x E2z - E1z E2x), E1x E2y - E1y E2x); len = sqrt((cx cx + cy cy) + cz cz); normal = c / len;
 *   area = len * 0.5f; the frames, if given.  nodes' = nodes with every leaf's box the min / max over its triangles in index
 *   order, mn = min2(mn, min2(a, min2(b, c))), min2(a, b) = b < a ? b : a, starting from FLT_MAX / lowest, and every interior box
 *   min2 / max2 of its children (childR first).  Positions must be finite; a zero-area triangle gets a NaN normal as on the host.
 *   Materials, uv, the topology of both trees, the number of triangles and the set of emissive triangles stay as they are
 *   (as uploaded, or as the last pt_scene_update_materials left them).
 *   Every kernel is enqueued on `hip_stream` on the scene's device; no host synchronisation, nothing is read back, and nothing
 *   is allocated after the first call (which allocates and uploads the maps of the build: pt_scene_device_bytes includes them
 *   from then on).  A render enqueued on the same stream afterwards sees the new geometry; d_pos / d_frames must stay valid
 *   until the stream has passed the update.  One update or render at a time per scene.
 * pt_scene_update_vertices_host: h_pos / h_frames are HOST arrays; uploads them, updates on the NULL stream and waits.
 * pt_scene_update_spheres: a HOST array of the scene's sphere count; centre and radius may change, the material bytes must be
 *   those uploaded, or those of the last pt_scene_update_sphere_materials (else PT_ERR_INVALID).  A stream-ordered copy on the NULL stream.
 * pt_scene_tree_inflation: *ratio = sum of the surface areas (float32 each, summed in float64 in a fixed order) of all boxes of
 *   the binary traversal tree now / the same sum at upload or at the last pt_scene_rebuild_tree: the caller's signal that refits
 *   have degraded the tree (what to do about it: "Tree rebuild" below).  Exactly 1.0 for a scene never updated.  Otherwise waits for the whole device (hipDeviceSynchronize: the
 *   stream of the last update need not exist any more) and reduces on the NULL stream.
 * pt_dbg_scene_array (parity hook, tests only): copies one device array of the scene to the host after a device synchronisation;
 *   which = 0 nodes, 1 quad, 2 tri, 3 tripair, 4 leafbox, 5 surf, 6 lights, 7 spheres, 8 core (0 bytes if none; layouts:
 *   csrc/pt_device.h).  Returns the array's size in bytes and writes at most cap_bytes (h_out may be NULL when cap_bytes is 0).
 * NULL scene, NULL d_pos / h_pos / h_spheres / ratio, n_spheres different from the scene's and an unknown `which` return
 * PT_ERR_INVALID before any HIP call.
 * Out of scope: a change of the triangle count; an automatic rebuild; a tile-split update (every rank updates
 * its own scene).  The materials and the set of emissive triangles change through the calls of the next section.
 * -------------------------------------------------------------------------------- */
PT_API int  pt_scene_update_vertices(PtScene* s, const float* d_pos, const float* d_frames, void* hip_stream);
PT_API int  pt_scene_update_vertices_host(PtScene* s, const float* h_pos, const float* h_frames);
PT_API int  pt_scene_update_spheres(PtScene* s, const PtSphere* h_spheres, int32_t n_spheres);
PT_API int  pt_scene_tree_inflation(PtScene* s, double* ratio);
PT_API int64_t pt_dbg_scene_array(PtScene* s, int32_t which, void* h_out, int64_t cap_bytes);

/* ----------------------------------------------------------------------------------
 * Materials and lights of an uploaded scene (new: the reference uploads a scene once).  Opt-in: every call above is as it was.
 * A lamp switched on, a light dimmed, a wall recoloured, without pt_scene_create and its tree build: a render reads a material
 * only in floats 36..47 of the surface record and in the `lights` array with its count and the pruning flag, and no traversal
 * array depends on one (csrc/pt_material.hip).
 *
 * pt_scene_update_materials: d_mat12 is a DEVICE pointer to n_tris x 12 float32, one PtMaterial per triangle in the order of the
 *   `tris` given to pt_scene_create: emittance albedo specular opacity roughness metallic.  All three vertex materials of
 *   triangle i become that material m_i.  After the call the scene is, for every entry point (pt_render*, pt_render_aov,
 *   pt_render_views, pt_render_rays, pt_render_tile_list, pt_render_adaptive, pt_trace_rays with surface records, pt_dbg_raycast,
 *   pt_dbg_nee, both render modes), the scene pt_scene_create(nodes_cur, tris', spheres_cur) would give.  tris' = the scene's
 *   current triangles — as uploaded, or as the last pt_scene_update_vertices left them, normal and area restated from the current
 *   positions by that call's expressions — with mat0 = mat1 = mat2 = m_i.  So: surface-record floats 36..47 become m_i; triangle
 *   i is a light iff sqrtf((ex*ex + ey*ey) + ez*ez) > 0.0001f for its new emittance, in float32, every operation rounded once (a
 *   NaN makes no light); `lights` holds the records V0 V1 V2 normal area 0 0 0 of the lights in ascending triangle index, made
 *   from the scene's own copy of the current positions; pt_scene_num_lights and the lights a later vertex update moves follow
 *   the new set; the pruning flag (pt_scene_nee_prune) is 1 iff every triangle's new emittance and every sphere's emittance is
 *   finite, >= 0 and <= 1e8 and PTAMD_PRUNE is not 0.  The traversal arrays, uv, the shading schedule and the core box are
 *   untouched.  A scene may end up with no light: it then behaves like a scene created so (renders and pt_dbg_nee return
 *   PT_ERR_NO_LIGHT, queries and AOVs work), and a later update may bring lights back.
 *   Every kernel is enqueued on `hip_stream` on the scene's device.  The call waits for that stream ONCE: the number of lights
 *   and the flag are kernel arguments of every later render, so 8 bytes are read back, and the same number sizes `lights`.
 *   d_mat12 is free when the call returns; the light records are written in stream order after it, so a render enqueued on the
 *   same stream sees them.  `lights` grows on demand and never shrinks (pt_scene_device_bytes follows); an update with no more
 *   lights than any earlier one allocates nothing, except that the first update of either kind uploads the maps of the build and
 *   the positions, as pt_scene_update_vertices states.  One update, query or render at a time per scene.  After PT_ERR_DEVICE
 *   the materials of the scene are unspecified: update again or destroy it.
 * pt_scene_update_materials_host: h_mat12 is a HOST array; uploads it, updates on the NULL stream and waits.
 * pt_scene_update_sphere_materials: a HOST array of the scene's sphere count; centre, radius and material may all change.  A
 *   stream-ordered copy on the NULL stream; the pruning flag is formed again from these spheres and the triangles' current
 *   materials.  pt_scene_update_spheres compares against these materials from then on.
 * pt_scene_nee_prune (parity hook): the pruning flag as the next render will see it; 0 for NULL.
 * NULL scene, NULL d_mat12 / h_mat12 / h_spheres and n_spheres different from the scene's return PT_ERR_INVALID before any HIP
 * call; the pointers are not dereferenced on that path.
 * Out of scope: per-vertex materials that differ within a triangle (the device shades with mat0 alone); a change of the
 * triangle or sphere count; a tile-split update (every rank updates its own scene); a ptrender option; asynchronous operation
 * without the one wait.
 * -------------------------------------------------------------------------------- */
PT_API int  pt_scene_update_materials(PtScene* s, const float* d_mat12, void* hip_stream);
PT_API int  pt_scene_update_materials_host(PtScene* s, const float* h_mat12);
PT_API int  pt_scene_update_sphere_materials(PtScene* s, const PtSphere* h_spheres, int32_t n_spheres);
PT_API int32_t pt_scene_nee_prune(const PtScene* s);

/* ----------------------------------------------------------------------------------
 * Tree rebuild (new: the reference builds its tree once, on the host).  Opt-in: every call above is as it was.
 * pt_scene_update_vertices keeps the topology of both traversal trees, so they degrade as the mesh deforms
 * (pt_scene_tree_inflation).  pt_scene_rebuild_tree builds both trees anew on the GPU from the scene's CURRENT positions — as
 * uploaded, or as the last pt_scene_update_vertices left them — on `hip_stream`, on the scene's device, without
 * pt_bvh_build_sah + pt_scene_create and without losing what the scene has accumulated (materials, the light set, the position
 * mirror).  The tree is a linear BVH over 30-bit Morton codes of the triangle centroids (csrc/pt_rebuild.hip, DESIGN.md
 * section 23).
 *
 * Results: a render is defined by the triangles and the reference leaf boxes alone, so after the call the scene is, for every
 *   entry point (pt_render*, pt_render_aov, pt_render_views, pt_render_rays, pt_render_tile_list, pt_render_adaptive,
 *   pt_trace_rays closest hit with surface records, pt_dbg_raycast, pt_dbg_nee, both render modes, wf_drain on either tree), bit
 *   for bit the scene it was before the call.  PT_QUERY_ANY keeps its own contract: the same hit / no-hit verdict; which hit is
 *   returned may change.
 * Arrays: leafbox, surf, lights, spheres, core, the light set and the pruning flag are not touched.  nodes, quad, tri and tripair
 *   are replaced and the record counts of nodes and quad may change; tri is a permutation of its records.
 * Function of the geometry alone: the four rebuilt arrays depend only on the current positions and the triangle -> reference
 *   leaf assignment.  A scene moved to positions P and rebuilt has byte for byte the nodes, quad, tri and tripair of a scene
 *   created at P and rebuilt; two rebuilds in a row change nothing.  No atomic operation decides an index or an order.
 * Later updates: pt_scene_update_vertices, pt_scene_update_materials and pt_scene_update_spheres work on the new trees exactly
 *   as specified above.  pt_scene_tree_inflation returns exactly 1.0 right after a rebuild: its denominator becomes the new
 *   tree's area sum, from the same reduction in the same fixed order.
 * Limits: those pt_scene_create enforces — binary depth <= 32, and 3 * (4-wide depth) + 2 <= the traversal kernel's stack
 *   capacity.  A rebuilt topology that breaks one returns PT_ERR_UNSUPPORTED WITH THE SCENE EXACTLY AS IT WAS: the topology is
 *   built and checked in buffers of its own before the first write to an array a render reads.  "As it was" is what a render,
 *   a query or an update sees: the refused call has still run and waited for the whole build (every retry does), and what the
 *   first rebuild allocated stays allocated (Memory).  After PT_ERR_DEVICE the trees are unspecified: rebuild again or destroy
 *   the scene.
 * Waiting: the call waits for `hip_stream` TWICE: once for the level offsets, the record counts and the two depths (they are
 *   checked, steer the per-height launches and become kernel arguments of every later render), once for the area sums.  The
 *   first rebuild of a scene waits a third time, before it frees the smaller blocks it replaces.  A render enqueued on the same
 *   stream afterwards sees the new trees.  One update, query, render or rebuild at a time per scene.
 * Memory: the first rebuild allocates for the worst case (2 n - 1 nodes of the binary tree, n - 1 `nodes` records, n - 1 `quad`
 *   records, the sort's temporary storage) and moves nodes, quad and the maps of the build into blocks of that size; a failed
 *   allocation leaves the scene as it was.  What a scene holds for rebuilding follows the PARAMETERS of the rebuilds it has seen,
 *   through whichever of the three entry points they came: a later rebuild allocates only what its parameters need and no
 *   earlier call did — for large_fraction > 0 and for passes > 0, see the two "Memory" paragraphs below — and a call with
 *   parameters already seen allocates nothing.  pt_scene_device_bytes reports what is held: it grows with the first rebuild,
 *   whether that rebuild is accepted or refused (the 278,268-triangle scene: 126 MB at upload, 259 MB from the first rebuild
 *   on), and does not shrink again.
 * When to call it (measured on the MI355X, DESIGN.md sections 23 and 24): prefer pt_scene_rebuild_tree_ex with its defaults
 *   (below) to this call, and neither to the refit tree while pt_scene_tree_inflation is small.  Both calls are cheap (this one
 *   0.5 ms for 69,576 triangles and 0.8 ms for 278,268, the extended one 12 - 18 % more; the host rebuild takes 114 ms and
 *   506 ms).  After turns of 10, 25 and 90 degrees of the stand-in mesh (inflation 1.06 - 1.12) the tree of THIS call rendered
 *   12 - 18 % slower than the refit tree and 19 - 20 % slower than a fresh host upload, with 35 - 40 % more node records fetched:
 *   a Morton-order tree files the room's big triangles among the mesh's small ones.  Its 4-wide tree has no depth cap (14 - 15
 *   levels against 11 - 12): pt_trace_rays and the render's drain walk the 4-wide tree only up to level 12 and the binary tree
 *   beyond, with the same results but not the same speed (a closest-hit query of 2.07 M rays: 0.63 - 0.73 ms against 0.20 -
 *   0.22 ms).  And the tree can be too deep altogether: the 278,268-triangle scene turned by 25 degrees reaches binary depth 33
 *   and is refused.  The tree of pt_scene_rebuild_tree_ex with {26, 1/16} has none of the last two problems - depth 25 / 12 on
 *   every scene measured, the 25 degree pose accepted, the query at 0.19 - 0.24 ms - and a smaller first one: it rendered
 *   2.7 - 7.4 % slower than the refit tree and 7.0 - 9.6 % slower than a fresh host upload (the refit tree: 1 - 6 % slower than
 *   the fresh one).  So that tree does NOT beat the refit tree at any inflation reached there.  pt_scene_rebuild_tree_opt
 *   ("Tree rebuild with treelet restructuring" below) improves it by surface area: 2 - 4 % faster to render, ahead of the refit
 *   tree at the 25 degree pose (inflation 1.12) and 2 - 5 % behind it at the other two.  A GPU rebuild pays where refits have cost
 *   more than about 4 - 7 % of render time against a fresh tree, so time a render before and after.
 * pt_scene_tree_info (host only, no HIP call): the current counts of `nodes` and `quad` records, the depth of the binary and of
 *   the 4-wide tree, from upload or from the last rebuild, and the number of rebuilds so far.
 * pt_dbg_tree_limits (parity hook, host only): the limit check as pt_scene_create and pt_scene_rebuild_tree apply it to a pair
 *   of depths — PT_OK or PT_ERR_UNSUPPORTED — and, through the non-NULL pointers, the largest depths it accepts.
 * A NULL scene (pt_scene_tree_info: or a NULL out) returns PT_ERR_INVALID before any HIP call.
 * Out of scope: a change of the triangle count; an automatic rebuild (the caller decides from pt_scene_tree_inflation); a full
 * SAH or PLOC build on the GPU (the treelet pass of pt_scene_rebuild_tree_opt is the quality step there is); a rebuild of the
 * reference leaf assignment (it defines the result); a tile-split rebuild (every rank rebuilds its own scene and, the tree being
 * a function of the positions alone, gets the same one); a ptrender option.
 * -------------------------------------------------------------------------------- */
typedef struct PtTreeInfo { int32_t n_wide, n_quad, depth, quad_depth, rebuilds; } PtTreeInfo;
PT_API int  pt_scene_rebuild_tree(PtScene* s, void* hip_stream);
PT_API int  pt_scene_tree_info(const PtScene* s, PtTreeInfo* out);   /* host only, no HIP call */
PT_API int  pt_dbg_tree_limits(int32_t depth, int32_t quad_depth, int32_t* max_depth, int32_t* max_quad_depth);

/* ----------------------------------------------------------------------------------
 * Tree rebuild with a depth budget and two size classes (new).  Opt-in: pt_scene_rebuild_tree is exactly what it was.
 * pt_scene_rebuild_tree_ex is pt_scene_rebuild_tree with two parameters that answer its three weaknesses (csrc/pt_rebuild.hip,
 * DESIGN.md section 24).  Everything "Tree rebuild" above promises holds for it unchanged: bit-for-bit results of every entry
 * point (PT_QUERY_ANY: the same verdict), the untouched arrays, staging before commit with the limit check before the first
 * write to anything a render reads, the two waits (three for a scene's first rebuild), `rebuilds`, inflation of exactly 1.0
 * afterwards.  The four rebuilt arrays are a function of the current positions, the reference leaf assignment and the two
 * parameters alone.  With {0, 0} the call produces byte for byte what pt_scene_rebuild_tree produces.
 *
 * depth_budget D (0 = none): the binary tree is at most D deep, a leaf counting as a node — PtTreeInfo::depth <= D - 1 — and the
 *   4-wide tree at most (D - 1) / 2.  The radix tree is built as before; then every subtree v over more than two triangles with
 *   depth(v) + clog2(size(v)) >= D nearest the root is replaced by the balanced tree over the ranks of its triangles in Morton
 *   order (each triangle walks its parent links, rewrites its key below the bits v's keys share, and the radix tree is built a
 *   second time over the new keys; clog2(m) = the bit length of m - 1).  The tree above such a v is unchanged.  With D > 0 the
 *   call never returns PT_ERR_UNSUPPORTED (D <= 32 gives a 4-wide depth <= 15, the limit is 20), and with D <= 26 the 4-wide
 *   tree has at most 12 levels, which pt_trace_rays and the render's drain walk 4-wide throughout.  The budget adds no wait.
 * large_fraction f (0 = one class): a triangle whose own box is longer, on its longest axis, than f times the longest side of
 *   the box of all centroids is "large".  Each class quantises its centroids in a centroid box of its own (the same two-stage
 *   reduction, no float atomics) and the class is bit 62 of the sort key, so the root of the tree joins the tree of the small
 *   triangles and the tree of the large ones and the room's walls no longer sit among the mesh's triangles.  An empty class
 *   changes nothing.  All in float32, every operation rounded once.
 * report (may be NULL): n_large, the number of large triangles (0 when f = 0), and n_flattened_tris, the number of triangles
 *   whose key the budget changed.  Both are read back with the words the first wait already reads, and are valid for a refused
 *   call too.
 * Errors, before any HIP call: PT_ERR_INVALID for a NULL scene or params, D < 0 or D > 32, f negative, NaN or infinite, and
 *   D > 0 with D < clog2(n) for a scene of n >= 3 triangles (no tree over n triangles is that shallow).
 * Memory: by the parameters ("Memory" above).  large_fraction > 0 needs the boxes of the two classes, 16,384 + 64 bytes, and
 *   where the sort over all 64 key bits asks for more temporary storage than the rebuild already holds, storage of that size;
 *   the first such call of a scene allocates them.  depth_budget needs nothing: with large_fraction == 0 the call holds exactly
 *   what pt_scene_rebuild_tree holds.
 * When to call it: "When to call it" above; the call costs 0.53 ms for 69,576 triangles and 0.95 ms for 278,268.  Its tree is
 *   the starting point of pt_scene_rebuild_tree_opt (below), whose tree rendered 2 - 4 % faster for 2.5 - 4 ms more per call.
 * Out of scope: more than two classes; an automatic choice of the parameters; a ptrender option.
 * -------------------------------------------------------------------------------- */
typedef struct PtRebuildParams {
    int32_t depth_budget;    /* 0: none (today's tree).  Else the binary tree is at most this deep (a leaf counts as a node), <= 32 */
    float   large_fraction;  /* 0: one class.  Else a triangle whose box is longer than this fraction of the centroid box is "large" */
} PtRebuildParams;
typedef struct PtRebuildReport { int32_t n_large, n_flattened_tris; } PtRebuildReport;
PT_API void pt_rebuild_params_default(PtRebuildParams* p);          /* 26, 0.0625f */
PT_API int  pt_scene_rebuild_tree_ex(PtScene* s, const PtRebuildParams* p, PtRebuildReport* report /* may be NULL */, void* hip_stream);

/* ----------------------------------------------------------------------------------
 * Tree rebuild with treelet restructuring (new).  Opt-in: pt_scene_rebuild_tree and pt_scene_rebuild_tree_ex build exactly what
 * they did, and a scene that never asks for a pass holds nothing of a pass's ("Memory" below).
 * pt_scene_rebuild_tree_opt is pt_scene_rebuild_tree_ex(s, p, ...) with `passes` restructuring passes over the binary topology by
 * surface area (Karras and Aila 2013, "Fast parallel construction of high-quality bounding volume hierarchies";
 * csrc/pt_rebuild.hip).  The passes run after the last radix tree is built (after the rekey where there is a
 * budget) and before the numbering.  Everything "Tree rebuild" and "Tree rebuild with a depth budget" promise holds unchanged:
 * bit-for-bit results of every entry point (PT_QUERY_ANY: the same verdict), the untouched arrays, staging before commit with the
 * limit check before the first write to anything a render reads, `rebuilds`, inflation of exactly 1.0 afterwards, later updates on
 * the new trees.  The four rebuilt arrays are a function of the current positions, the reference leaf assignment, p and passes
 * alone.  passes == 0 is pt_scene_rebuild_tree_ex byte for byte.  Scenes of n <= 2 triangles take the single-leaf path and passes
 * is ignored.
 *
 * The pass.  Nodes are the raw nodes of the radix tree.  A LEAF is a singleton or an internal node over exactly two triangles;
 *   leaves are never opened, moved into or changed, so the order of tri, the maps and every leaf ref are those of
 *   pt_scene_rebuild_tree_ex.  An INTERIOR node is an internal node over more than two triangles.
 *   Boxes: a singleton's is the min / max of its three vertices, every other node's the min / max of (left child, right child);
 *   the box of a subset of a treelet's entries is the entry of the lowest bit joined with the others in ascending order (min2(so
 *   far, entry)).  Area is 2 * (dx * dy + dy * dz + dz * dx) in float32, every operation rounded once, no contraction.
 *   Levels: heights (leaf = 0), depths and the depth of the tree are those of the topology a pass starts from.  Interior nodes
 *   are processed in ascending start-of-pass height, one launch per height.  Nodes of one height are roots of disjoint subtrees
 *   and a restructure rearranges nodes inside its root's subtree only, so a node's subtree is complete and the node still sits at
 *   its start-of-pass depth when its turn comes, and no data passes between workgroups within a launch.
 *   Per interior node v: (1) box and height of v from its current children.  (2) The treelet: L = [left, right]; while |L| < 7
 *   and an entry is interior, the interior entry of largest area (the first of them in list order unless a later one is strictly
 *   larger) is replaced by its left child and its right child is appended; the opened node joins the list I.  Fewer than 3
 *   entries: nothing to do, the treelet is not counted.  (3) For every non-empty subset S of L (bit k = entry k): a[S] = area of
 *   its box; c[S] = 0 for one entry, else (S == full ? 0 : a[S]) + min over P of (c[P] + c[S \ P]), P the proper subsets of S
 *   that contain S's lowest bit, in ascending numeric order, a later P taken only where strictly smaller; h[S] = the height of
 *   the entry, else 1 + max(h[P], h[S \ P]) of the chosen P.  (4) Accept only if c[full] < area(I[0]) + area(I[1]) + ... (summed
 *   in opening order), strictly, and h[full] <= max(height(v), H_lim - depth(v)); H_lim = D - 1 for a budget D > 0, else the
 *   depth of the tree THIS PASS started from (PtTreeInfo::depth of that topology).  So the tree never gets deeper than the budget,
 *   or than it was, and a pass never turns an accepted rebuild into a refused one.  (5) Rewire: v stands for the full set, the
 *   node of S has the node of P on its left and the node of S \ P on its right, and every other subset of two or more entries
 *   takes the next unused node of I in pre-order (node, left subtree, right subtree).
 * report (may be NULL): n_large and n_flattened_tris as pt_scene_rebuild_tree_ex reports them; n_roots, the treelets solved,
 *   and n_restructured, the treelets accepted, both summed over all passes.  They travel with the words the first wait already
 *   reads (integer atomic sums; no atomic decides an index) and are valid for a refused call too.
 * Errors, before any HIP call: those of pt_scene_rebuild_tree_ex, and PT_ERR_INVALID for passes < 0 or passes > 8.  The report
 *   is left untouched on that path.
 * Waiting: as pt_scene_rebuild_tree_ex — the passes add no wait: the per-height launches are steered by level offsets that stay
 *   in device memory (a fixed grid walks the slice of its height; heights 1 .. D - 1, or 1 .. 63 without a budget, are launched
 *   whatever the tree's height is). Without a budget every pass enqueues 63 such launches, most over an empty
 *   slice: (0, 1/16) with 2 passes cost 4.44 - 4.47 ms for 69,576 triangles against 3.04 - 3.06 ms with the budget of 26.
 * Memory: by the parameters ("Memory" of "Tree rebuild").  passes > 0 needs 28 bytes per raw node (a height and a box; 2 n - 1
 *   raw nodes) and the 516 bytes of a pass's level offsets — 15.6 MB for 278,268 triangles — which the first such call of a
 *   scene allocates; with passes == 0 the call holds exactly what pt_scene_rebuild_tree_ex with the same p holds.
 * When to call it (measured on the MI355X): whenever you rebuild on the GPU, prefer this call with its
 *   defaults to pt_scene_rebuild_tree_ex; against the refit tree, still time a render before and after.  Two passes take 8 - 9 %
 *   off the sum of the interior boxes' areas on the stand-in scene at 18,252 triangles (a third pass 0.2 %, so 2 is the default).
 *   After turns of 10, 25 and 90 degrees of the stand-in mesh (69,576 triangles, inflation 1.06 - 1.12) the tree of this call
 *   rendered 2.4 - 4.4 % faster than the tree of pt_scene_rebuild_tree_ex and fetched 5.1 - 6.9 % fewer node records - fewer
 *   than the refit tree on all three poses (1.7 - 6.9 %), 2.2 - 2.6 % more than a fresh host upload.  In render time it beat the
 *   refit tree at 25 degrees (2.8 % faster, inflation 1.12) and not at 10 and 90 degrees (1.8 % and 5.1 % slower); it stayed
 *   3.5 - 7.3 % behind a fresh host upload (pt_scene_rebuild_tree_ex: 6.2 - 10.2 %).  So a GPU rebuild now pays from an inflation
 *   of about 1.1 on, or wherever refits have cost more than about 4 - 7 % of render time against a fresh tree.  The call costs
 *   more than estimated: 3.0 - 3.1 ms for 69,576 triangles and 4.8 ms for 278,268 (pt_scene_rebuild_tree_ex: 0.55 - 0.57 ms and
 *   0.94 - 0.99 ms, so 4.8 - 5.6 times), 1.1 - 1.4 ms and 1.6 - 2.2 ms per pass: a pass is up to 25 launches one after the other,
 *   each as long as its slowest treelet.  That is 37 and 106 times below the host rebuild (114 ms and 506 ms).  The closest-hit
 *   query of 2.07 M rays stays where it was (0.22 - 0.28 ms; depth 25 / 12 on every pose).
 * Out of scope: optimising a refit or an uploaded tree in place; the host build's area-driven 4-wide collapse (the 4-wide tree
 *   is still every second level of the binary one); an automatic choice of passes; a ptrender option.
 * -------------------------------------------------------------------------------- */
typedef struct PtRebuildOptReport { int32_t n_large, n_flattened_tris, n_roots, n_restructured; } PtRebuildOptReport;
PT_API int32_t pt_rebuild_opt_passes_default(void);   /* 2 */
PT_API int  pt_scene_rebuild_tree_opt(PtScene* s, const PtRebuildParams* p, int32_t passes,
                                      PtRebuildOptReport* report /* may be NULL */, void* hip_stream);

/* ----------------------------------------------------------------------------------
 * Ray queries (new: the reference casts rays only from inside its integrator).  Opt-in: every call above is as it was.
 * The caller's own rays against an uploaded scene, on the device and in stream order (csrc/pt_query.hip): visibility between
 * points, baking, picking, range simulation, collision probes against a mesh that pt_scene_update_vertices moves.
 *
 * Rays are RAY8 records (oracle/pt_oracle.h, pt_dbg_raycast): org.xyz | dir.xyz | reserved | tmax.  The reserved float is the
 *   oracle's tmin: it must be 0 and the device does not read it.  The direction is used as given — not normalised —, t is the
 *   parameter along it and the range is [0, tmax].  Semantics are the reference's RayCast (include/CudaUtil.cuh:93-148):
 *   triangles are back-face culled, spheres are tested after the triangles, and among equal t the largest primitive index wins.
 *   A triangle counts iff Triangle::hit accepts it and the ray enters its reference leaf box (the reference's slab arithmetic).  For
 *   |(1/dx, 1/dy, 1/dz)| >= 1 — every direction with components in [-1, 1] — that IS the reference's result; for longer directions
 *   the reference's box cull (a normalised entry distance against the un-scaled closest t) drops hits in an order-dependent way,
 *   which the device, here as in pt_dbg_raycast, does not imitate: it returns the closest hit in [0, tmax].
 *   Known defect (found by tests/test_slack.py, not yet fixed).  Float Moeller-Trumbore is ill-conditioned for thin
 *   triangles and far origins: its barycentric error is about e = 2^-24 * kappa * |T|, kappa = |E1| |E2| / |E1 x E2|, T = org - V0.  Within
 *   e of an edge it accepts rays that pass OUTSIDE the triangle's own box by more than the traversal trees' pads, while the
 *   reference's leaf box (up to four triangles) still lets them through: the reference reports the hit and no walk of the trees here
 *   reaches it.  Such a ray gets the closest hit among the triangles whose boxes it does enter (another primitive, or a miss), and
 *   the 4-wide walk, the binary walk (PTAMD_QUERY_QUAD=0), pt_dbg_raycast and a tree after pt_scene_rebuild_tree need not agree on it.
 *   The pads bound where it can happen: a ray is safe when e * (the triangle's longest edge) is within the absolute pad of the
 *   4-wide boxes, maxabs * 2^-20 (maxabs: the scene's largest coordinate) — in a room 40 wide, an ordinary mesh triangle
 *   (kappa 1.5, edge 2.6) seen from within about 160 units; the searches find the first such ray at e = 4.8 * 10^-5.  Outside that
 *   it is rare, not absent: of 10^6 rays aimed at the ends and edges of 10 x 10^-3 slivers from inside the room 39, at box corners
 *   of an ordinary mesh from 2^10 .. 2^19.5 away 34.  Every entry point that traces rays shares it.
 * PT_QUERY_CLOSEST: d_hits[i] = (t, prim) of the closest hit, bit for bit what pt_dbg_raycast and the reference return (but for the
 *   rays of the known defect above); prim
 *   counts triangles first (the order of `tris`) and spheres after them; a miss is prim = -1, t = 0.  d_surface29 is NULL or
 *   receives, per ray, the 29-float HIT record exactly as pt_dbg_raycast writes it (zeros for a miss).
 * PT_QUERY_ANY: prim >= 0 exactly when the closest-hit query of the same ray hits.  The hit returned is SOME hit the reference
 *   would accept in [0, tmax] — t <= tmax, t >= the closest t —, not necessarily the closest; which one is unspecified and may
 *   change between versions.  d_surface29 must be NULL.
 * pt_trace_rays: d_rays8 (16-byte aligned), d_hits (8-byte aligned) and d_surface29 are DEVICE pointers on the scene's device
 *   holding n records.  Everything is enqueued on `hip_stream`: no host wait, nothing is read back, nothing is allocated
 *   (pt_scene_device_bytes stays what it was).  A query enqueued
 *   after pt_scene_update_vertices on the same stream sees the moved geometry.  The buffers must stay valid until the stream has
 *   passed the query.  A query leaves every render state alone: frames, pt_last_iterations, pt_last_counters, pt_last_render_ms.
 *   Concurrency: ONE query, update or render at a time per scene (a query in flight on one stream while another query, an update
 *   or a render of the same scene runs on another stream is not supported; different scenes are independent).
 * pt_trace_rays_host: the same on HOST arrays: uploads, queries on the NULL stream, waits and downloads.
 * NULL scene / rays / hits, n < 0, an unknown mode, misaligned d_rays8 / d_hits / d_surface29 and a surface buffer given with
 *   PT_QUERY_ANY return PT_ERR_INVALID before any HIP call; n = 0 returns PT_OK without one.
 * Rays with a non-finite component or a zero direction: the result for THAT ray is unspecified (prim stays in [-1, number of
 *   primitives)), the other rays of the batch are unaffected, and the call ends: the walk is a depth-first search over a finite
 *   tree, its stack bounded by the depth of the tree whatever the floats are (csrc/pt_trace.h: quad_step).
 * Out of scope: tmin other than 0, sorting rays for coherence, hit callbacks, primitive masks, a tile-split or multi-GPU query.
 * -------------------------------------------------------------------------------- */
typedef struct PtRayHit { float t; int32_t prim; } PtRayHit;      /* 8 bytes */
#define PT_QUERY_CLOSEST 0
#define PT_QUERY_ANY     1
PT_API int  pt_trace_rays(PtScene* s, const float* d_rays8, int64_t n, int32_t mode, PtRayHit* d_hits, float* d_surface29, void* hip_stream);
PT_API int  pt_trace_rays_host(PtScene* s, const float* h_rays8, int64_t n, int32_t mode, PtRayHit* h_hits, float* h_surface29);

/* ----------------------------------------------------------------------------------
 * Closest-point queries (new: the reference has no such query).  Opt-in: every call above is as it was.
 * The other half of a BVH query set: what is near a POINT of the caller's, on the device and in stream order (csrc/pt_nearest.hip):
 * distance and penetration probes against a mesh that pt_scene_update_vertices moves, snapping a picked point to the surface,
 * signed-distance and proximity baking, "is anything within r of this sensor".
 *
 * Points are POINT4 records: p.xyz | radius.  The radius must be >= 0; +inf is allowed.  The search bound is r2 = radius * radius in
 *   float32.  Primitives are numbered as in pt_trace_rays: triangles first, in the order of `tris`, spheres after them.  None of the
 *   ray rules apply: distance is two-sided, nothing is culled by facing, and the reference leaf boxes play no part.
 * Arithmetic: IEEE float32, every operation below rounded once and none contracted, in the order written;
 *     dot(a, b)   = (ax*bx + ay*by) + az*bz
 *     cross(a, b) = (ay*bz - az*by, -(ax*bz - az*bx), ax*by - ay*bx)
 *     min / max of two floats (no NaN arises from finite input), component-wise on vectors.
 * f(p, k) for triangle k, V0 E1 E2 = its vertex 0 and the float32 edges V1 - V0, V2 - V0 (the PtTriangle fields v0, E1, E2):
 *     a = V0, ab = E1, ac = E2, bc = ac - ab, ap = p - a, bp = ap - ab
 *     seg(q, e):  t = dot(q, e) / dot(e, e);  t = (t > 0) ? t : 0;  t = (t < 1) ? t : 1;      (a zero edge gives a NaN t: the first clamp makes it 0)
 *                 r = q - t * e;  seg = dot(r, r)
 *     d_edge = min(min(seg(ap, ab), seg(ap, ac)), seg(bp, bc))
 *     n = cross(ab, ac);  nn = dot(n, n);  h = dot(ap, n)
 *     inside = nn > 0 && dot(cross(ab, ap), n) >= 0 && dot(cross(bc, bp), n) >= 0 && dot(cross(ap, ac), n) >= 0
 *     d_raw  = (inside && (h*h)/nn < d_edge) ? (h*h)/nn : d_edge
 *     lo, hi = component-wise min(min(a, a + ab), a + ac), max(max(a, a + ab), a + ac)      (the box of the triangle the record describes)
 *     boxdist2(p, lo, hi):  per axis g = max(max(lo - p, p - hi), 0);  boxdist2 = (gx*gx + gy*gy) + gz*gz
 *     f = max(d_raw, boxdist2(p, lo, hi))
 *   The edge candidates make a wrong inside / outside call near an edge harmless (the two meet there), and no input, zero-area
 *   triangles included, gives a NaN.  The last line is a floor: the float32 normal of a thin triangle is tilted, so the plane term can
 *   fall below the true distance; the floor moves f towards the true distance only, and it gives f(p, k) >= boxdist2(p, box of k)
 *   EXACTLY — the inequality that lets a tree walk prune without ever disagreeing with the definition below.
 * f(p, k) for sphere j (k = number of triangles + j):  pc = p - center;  l = sqrt(dot(pc, pc));  g = l - rad;  f = g * g.
 * PT_NEAREST_CLOSEST: defined without reference to any tree.  Among the primitives k with f(p, k) <= r2, d_out[i] = (f(p, k), k) of
 *   the smallest f; among equal f the largest k (the tie rule of the ray queries).  No such primitive: a miss, (0, -1).  The result
 *   is therefore bit for bit the same before and after a refit or any rebuild, and equals a brute-force evaluation over the scene's
 *   current positions.
 * PT_NEAREST_ANY: prim >= 0 exactly when the closest query of the same record finds something.  The primitive returned is SOME k with
 *   f(p, k) <= r2 and dist2 = f(p, k) bit for bit; which k is unspecified and may change between versions (the walk stops at the
 *   first).  d_detail8 must be NULL.
 * d_detail8 (PT_NEAREST_CLOSEST only; may be NULL): 8 floats per point about the winning primitive, zeros for a miss:
 *     c.xyz | v | w | side | feature | 0
 *   For a triangle, with t1, t2, t3 the clamped parameters and d1, d2, d3 the values of seg(ap, ab), seg(ap, ac), seg(bp, bc):
 *     interior = inside && (h*h)/nn < d_edge
 *     interior:            feature 0;  v = dot(cross(ap, ac), n) / nn;  w = dot(cross(ab, ap), n) / nn;  c = p - (h / nn) * n
 *     else d1 == d_edge:   feature 1 (edge AB);  v = t1;  w = 0;  c = a + t1 * ab
 *     else d2 == d_edge:   feature 2 (edge AC);  v = 0;  w = t2;  c = a + t2 * ac
 *     else                 feature 3 (edge BC);  v = 1 - t3;  w = t3;  c = (a + ab) + t3 * bc
 *     side = (h >= 0) ? +1 : -1      (h = dot(p - V0, cross(E1, E2)))
 *   so that c ~ V0 + v E1 + w E2; a clamped parameter puts c on a vertex.  (c is the point d_raw measures to; where the floor decides f,
 *   |p - c|^2 is below dist2 by the rounding the floor repairs.)  For a sphere: feature 4, v = w = 0, side = (l >= rad) ? +1 : -1 and
 *   c = center + (rad / l) * pc, or (center.x + rad, center.y, center.z) when l == 0.
 * pt_closest_points: d_points4 (16-byte aligned), d_out (8-byte aligned) and d_detail8 (4-byte aligned) are DEVICE pointers on the
 *   scene's device holding n records.  Everything is enqueued on `hip_stream`: no host wait, nothing is read back, nothing is allocated
 *   (pt_scene_device_bytes stays what it was); batches of at most 2^30 points go per launch.  A query enqueued after
 *   pt_scene_update_vertices, pt_scene_rebuild_tree, pt_scene_rebuild_tree_ex or pt_scene_rebuild_tree_opt on the same stream sees
 *   their result.  The buffers must stay valid until the stream has passed the query.  A query leaves every render state alone:
 *   frames, pt_last_iterations, pt_last_counters, pt_last_render_ms.  Concurrency: ONE query, update or render at a time per scene.
 * pt_closest_points_host: the same on HOST arrays: uploads, queries on the NULL stream, waits and downloads.
 * NULL scene / points / out, n < 0, an unknown mode, misaligned d_points4 / d_out / d_detail8 and a detail buffer given with
 *   PT_NEAREST_ANY return PT_ERR_INVALID before any HIP call, no pointer dereferenced; n = 0 returns PT_OK without one.
 * A point with a non-finite coordinate, or a negative or NaN radius: the result for THAT point is unspecified (prim stays in [-1,
 *   number of primitives)), the other points of the batch are unaffected, and the call ends by the argument of quad_step
 *   (csrc/pt_trace.h): a depth-first walk over a finite tree, its stack bounded by the depth of the tree whatever the floats are.
 * Out of scope: per-primitive masks, a multi-GPU split, a CLI option, sorting the points for coherence.  The k nearest and the number
 * of primitives within a radius: the next section.
 * -------------------------------------------------------------------------------- */
typedef struct PtNearest { float dist2; int32_t prim; } PtNearest;     /* 8 bytes */
#define PT_NEAREST_CLOSEST 0
#define PT_NEAREST_ANY     1
PT_API int  pt_closest_points(PtScene* s, const float* d_points4, int64_t n, int32_t mode, PtNearest* d_out, float* d_detail8 /* may be NULL */,
                              void* hip_stream);
PT_API int  pt_closest_points_host(PtScene* s, const float* h_points4, int64_t n, int32_t mode, PtNearest* h_out, float* h_detail8 /* may be NULL */);

/* ----------------------------------------------------------------------------------
 * K nearest and counts within a radius (new: the reference has no such query).  Opt-in: every call above is as it was.
 * pt_closest_points returns one primitive per point; these return several (csrc/pt_knearest.hip): the contact set of a probe, the
 * neighbours a smooth distance field is blended from, several candidates for registration or snapping, "how crowded is it around
 * this sensor".
 *
 * Points are POINT4 records p.xyz | radius exactly as pt_closest_points takes them: r2 = radius * radius in float32, radius >= 0, +inf
 *   allowed; triangles are numbered first, in the order of `tris`, spheres after them.  f(p, k) is the function of the section above,
 *   operation for operation, for triangles and spheres.  Let C(p) = { k : f(p, k) <= r2 }.
 * pt_nearest_k: the K nearest within the radius, sorted; defined without reference to any tree.  Order C(p_i) by f ascending, among
 *   equal f the larger primitive index first (the tie rule of the closest query; no two members share both, so the order is total).
 *   Slot j of point i, d_out[i * k + j], is (f, prim) of the j-th member for j < min(k, |C|); every later slot is the miss record
 *   (0, -1).  Hence slot 0 is bit for bit what pt_closest_points(PT_NEAREST_CLOSEST) writes for the same record, k = 1 is that call,
 *   the result equals a brute-force evaluation over the scene's current positions, and it is the same bits before and after a refit
 *   or any rebuild.  1 <= k <= PT_NEAREST_KMAX.
 * d_detail8 (may be NULL): one 8-float record per slot, d_detail8[(i * k + j) * 8 ..], in the layout of the section above,
 *   c.xyz | v | w | side | feature | 0.  The record of a slot depends only on the point and the slot's primitive; a miss slot holds zeros.
 * pt_count_within: d_count[i] = |C(p_i)|, uncapped.  With pt_nearest_k it tells whether the K slots were all there is; with k = 32 the
 *   two calls together are "all primitives within a radius" for any neighbourhood of up to 32.  An infinite radius counts every
 *   primitive by walking the whole tree: allowed, and the caller's cost.
 * pt_nearest_k, pt_count_within: d_points4 (16-byte aligned), d_out (8-byte aligned), d_detail8 and d_count (4-byte aligned) are DEVICE
 *   pointers on the scene's device holding n, n * k, n * k * 8 and n records.  Everything is enqueued on `hip_stream`: no host wait,
 *   nothing is read back, nothing is allocated (pt_scene_device_bytes stays what it was); batches of at most 2^30 points go per
 *   launch.  A query enqueued after pt_scene_update_vertices, pt_scene_rebuild_tree, pt_scene_rebuild_tree_ex or
 *   pt_scene_rebuild_tree_opt on the same stream sees their result.  The buffers must stay valid until the stream has passed the
 *   query.  A query leaves every render state alone: frames, pt_last_iterations, pt_last_counters, pt_last_render_ms.  Concurrency:
 *   ONE query, update or render at a time per scene.
 * pt_nearest_k_host, pt_count_within_host: the same on HOST arrays: upload, query on the NULL stream, wait and download.  h_out has
 *   n * k records.
 * NULL scene / points / out, n < 0, k < 1 or k > PT_NEAREST_KMAX and a misaligned device pointer return PT_ERR_INVALID before any
 *   HIP call, no pointer dereferenced, the message naming the entry point; n = 0 returns PT_OK without one.
 * A point with a non-finite coordinate, or a negative or NaN radius: the result for THAT point is unspecified (every prim stays in
 *   [-1, number of primitives), every count in [0, number of primitives]), the other points of the batch are unaffected, and the
 *   call ends by the argument of quad_step (csrc/pt_trace.h).
 * Out of scope: k above 32 (every primitive within a radius: pt_within_radius_list, two sections on), per-primitive masks, the k nearest along a ray (the next section),
 * sorting the points for coherence, a multi-GPU split, a CLI option.
 * -------------------------------------------------------------------------------- */
#define PT_NEAREST_KMAX 32
PT_API int  pt_nearest_k(PtScene* s, const float* d_points4, int64_t n, int32_t k, PtNearest* d_out /* n * k */,
                         float* d_detail8 /* n * k * 8, may be NULL */, void* hip_stream);
PT_API int  pt_nearest_k_host(PtScene* s, const float* h_points4, int64_t n, int32_t k, PtNearest* h_out, float* h_detail8 /* may be NULL */);
PT_API int  pt_count_within(PtScene* s, const float* d_points4, int64_t n, int32_t* d_count, void* hip_stream);
PT_API int  pt_count_within_host(PtScene* s, const float* h_points4, int64_t n, int32_t* h_count);

/* ----------------------------------------------------------------------------------
 * First K hits along a ray and hit counts (new: the reference keeps the closest hit only).  Opt-in: every call above is as it was.
 * pt_trace_rays returns one hit per ray; these return several, or their number (csrc/pt_rayhits.hip): what lies behind the first
 * surface (x-ray, thickness, multi-return range simulation, transmission through several walls), how many surfaces a segment
 * crosses (its parity is an inside / outside test), and what the back faces do, which every other ray entry point culls.
 *
 * Rays are RAY8 records exactly as pt_trace_rays takes them: org.xyz | dir.xyz | reserved (not read) | tmax; the direction is used as
 *   given, t is the parameter along it, the range is [0, tmax]; primitives are numbered triangles first, in the order of `tris`, then
 *   spheres.  flags is PT_HITS_FRONT (back faces culled, as everywhere else) or PT_HITS_BOTH_SIDES.
 * Arithmetic: IEEE float32, every operation below rounded once and none contracted, in the order written;
 *     dot(a, b)   = (ax*bx + ay*by) + az*bz
 *     cross(a, b) = (ay*bz - az*by, -(ax*bz - az*bx), ax*by - ay*bx)
 * Triangle k, V0 E1 E2 from its record (the PtTriangle fields v0, E1, E2), kEps = 1e-4f:
 *     T = org - V0;  P = cross(dir, E2);  Q = cross(T, E1)
 *     det = dot(P, E1);  t = dot(Q, E2) * (1 / det);  u = dot(P, T);  v = dot(Q, dir)
 *   FRONT acceptance (Triangle::hit's, operation for operation, facing +1):
 *     !(det < kEps)  &&  !(t < 0)  &&  !(t > tmax)  &&  !(u < 0 || u > det)  &&  !(v < 0 || v + u > det)
 *     && the ray passes the reference's slab test of the triangle's reference leaf box, uncut (the rule of the ray-query section;
 *        it passes always for a degenerate ray: one whose |(1/dx, 1/dy, 1/dz)| is not finite, i.e. a direction with a zero component).
 *   BACK acceptance (counted only under PT_HITS_BOTH_SIDES, facing -1): !(-det < kEps), the same t, and the same four range tests
 *     on -u, -v, -det (negation is exact); the same leaf-box condition.  No triangle is accepted on both sides.
 * Sphere j (prim = number of triangles + j), center c, radius rad:
 *     oc = org - c;  a = dot(dir, dir);  half_b = dot(oc, dir);  cc = dot(oc, oc) - rad * rad;  disc = half_b * half_b - a * cc
 *     disc < 0: no hit.  sq = sqrt(disc);  r1 = (-half_b - sq) / a;  r2 = (-half_b + sq) / a;  a root r is valid when !(r < 0) && !(tmax < r)
 *   PT_HITS_FRONT: the one root Sphere::hit returns for [0, tmax]: r1 if valid, else r2 if valid.
 *   PT_HITS_BOTH_SIDES: r1 if valid (entering, facing +1), and r2 if valid and r2 != r1 (leaving, facing -1).
 * H(ray) is the set of accepted (t, prim, facing) records; only a sphere under PT_HITS_BOTH_SIDES can contribute two records with one
 *   prim, and they differ in t.  Order: t ascending, compared as floats (-0 equals +0); among equal t the larger prim first — the tie
 *   rule of every ray entry point here.
 * pt_trace_rays_k: slot j of ray i, d_hits[i * k + j], is the j-th member of H(ray i) for j < min(k, |H|); every later slot is the miss
 *   record (0, -1).  1 <= k <= PT_RAY_HITS_KMAX.  t's bits are the float's own (a hit at -0.0 is reported as -0.0).  The definition
 *   names no tree: the result is the same bits before and after a refit or any rebuild and equals a brute-force evaluation over the
 *   scene's current positions.  With PT_HITS_FRONT slot 0 is bit for bit what pt_trace_rays(PT_QUERY_CLOSEST) writes for the same
 *   ray, and k = 1 is that call.  The known defect of the ray-query section (rays that Moeller-Trumbore accepts
 *   outside the boxes no tree lets them into) applies to every member of H as it does to the closest hit.
 * d_detail4 (may be NULL): 4 floats per slot, d_detail4[(i * k + j) * 4 ..]:  u * (1 / det) | v * (1 / det) | facing | 0, so that the
 *   hit point is approximately V0 + that * E1 + that * E2.  A sphere slot has 0 | 0 | facing | 0; a miss slot holds zeros.
 * pt_count_hits: d_count[i] = |H(ray i)|, uncapped, int32.  With pt_trace_rays_k it tells whether the K slots were all there is.
 * pt_trace_rays_k, pt_count_hits: d_rays8 (16-byte aligned), d_hits (8-byte aligned), d_detail4 and d_count (4-byte aligned) are DEVICE
 *   pointers on the scene's device holding n, n * k, n * k * 4 and n records.  Everything is enqueued on `hip_stream`: no host wait,
 *   nothing is read back, nothing is allocated (pt_scene_device_bytes stays what it was); batches of at most 2^30 rays go per launch.
 *   A query enqueued after pt_scene_update_vertices, pt_scene_rebuild_tree, pt_scene_rebuild_tree_ex or pt_scene_rebuild_tree_opt on
 *   the same stream sees their result.  The buffers must stay valid until the stream has passed the query.  A query leaves every render
 *   state alone: frames, pt_last_iterations, pt_last_counters, pt_last_render_ms.  Concurrency: ONE query, update or render at a time
 *   per scene.
 * pt_trace_rays_k_host, pt_count_hits_host: the same on HOST arrays: upload, query on the NULL stream, wait and download.  h_hits has
 *   n * k records.
 * NULL scene / rays / hits / count, n < 0, k < 1 or k > PT_RAY_HITS_KMAX, flags other than the two values and a misaligned device
 *   pointer return PT_ERR_INVALID before any HIP call, no pointer dereferenced, the message naming the entry point; n = 0 returns
 *   PT_OK without one.
 * A ray with a non-finite component or a zero direction: the result for THAT ray is unspecified (every prim stays in [-1, number of
 *   primitives), every count in [0, number of triangles + 2 * number of spheres]), the other rays of the batch are unaffected, and the
 *   call ends by the argument of quad_step (csrc/pt_trace.h).
 * Cost: k = 1 costs more than the lean closest-hit kernel — measured 1.16 to 1.33 times pt_trace_rays(PT_QUERY_CLOSEST) on 2 M rays
 *   (DESIGN.md section 34): for one hit per ray call pt_trace_rays.
 * Out of scope: k above 32 (every hit: pt_trace_rays_list, the next section), tmin other than 0, primitive masks, the 29-float surface
 * record per slot, a CLI option, a multi-GPU split.
 * -------------------------------------------------------------------------------- */
#define PT_RAY_HITS_KMAX   32
#define PT_HITS_FRONT      0
#define PT_HITS_BOTH_SIDES 1
PT_API int  pt_trace_rays_k(PtScene* s, const float* d_rays8, int64_t n, int32_t k, int32_t flags, PtRayHit* d_hits /* n * k */,
                            float* d_detail4 /* n * k * 4, may be NULL */, void* hip_stream);
PT_API int  pt_trace_rays_k_host(PtScene* s, const float* h_rays8, int64_t n, int32_t k, int32_t flags, PtRayHit* h_hits, float* h_detail4 /* may be NULL */);
PT_API int  pt_count_hits(PtScene* s, const float* d_rays8, int64_t n, int32_t flags, int32_t* d_count, void* hip_stream);
PT_API int  pt_count_hits_host(PtScene* s, const float* h_rays8, int64_t n, int32_t flags, int32_t* h_count);

/* ----------------------------------------------------------------------------------
 * Variable-length query results: all hits along a ray, all primitives in a radius (new: the reference has no such query).  Opt-in:
 * every call above is as it was.  pt_trace_rays_k and pt_nearest_k return at most 32 per query; these return every member, in CSR form
 * (csrc/pt_lists.hip, csrc/pt_rayhits.hip, csrc/pt_knearest.hip): the thickness of every wall a ray crosses, the full contact set of a
 * probe, every triangle inside a brush radius.  DESIGN.md section 37.
 *
 * The protocol, three device calls in stream order, none of which allocates, waits or reads back:
 *     pt_count_hits / pt_count_within     -> d_count[n]
 *     pt_list_offsets(d_count, n)         -> d_offsets[n + 1]      (the caller reads the 8-byte total d_offsets[n] back, at its own cost,
 *                                                                    and allocates)
 *     pt_trace_rays_list / pt_within_radius_list(..., d_offsets, cap, records)      -> every segment filled, sorted
 * pt_list_offsets: d_offsets[0] = 0 and d_offsets[i + 1] = d_offsets[i] + max(d_count[i], 0), in int64 (the sum does not wrap at 2^31).
 *   n = 0 writes the single 0.  The result depends only on the counts: the same bits on every run.  It needs no scene and runs on the
 *   current device.  d_scratch: pt_list_offsets_scratch_bytes(n) bytes of device memory (2 KB for any n > 0, 0 for n = 0; -1 for
 *   n < 0), 8-byte aligned, not read before it is written.  Three launches: per-span sums over at most 256 workgroups (a span is a whole
 *   number of 2,048-count chunks), one workgroup scanning those partials, a rescan of every span from its base; no workgroup waits on
 *   another.
 * pt_trace_rays_list: the segment of ray i is [b, e) with b = clamp(d_offsets[i], 0, cap) and e = clamp(d_offsets[i + 1], b, cap).  No
 *   other record of d_hits or d_detail4 is written, whatever the offsets hold: garbage offsets give garbage segments (overlapping ones
 *   among them), never a write outside [0, cap).  With m = e - b and H = H(ray i) under `flags`, exactly as pt_trace_rays_k defines it
 *   (acceptance, arithmetic, order, tie rule):
 *     m >= |H|: slots 0 .. |H| - 1 of the segment are the members of H in order; the later slots hold the miss record (0, -1).
 *     m < |H|:  the m slots hold m distinct members of H, sorted among themselves; which members is unspecified.
 *   Hence with offsets made from pt_count_hits of the same rays, flags and scene state, the records are the concatenation of every H,
 *   bit for bit: brute force over the scene's current positions, before and after a refit or any rebuild.  Slot 0 of a non-empty
 *   PT_HITS_FRONT list is pt_trace_rays(PT_QUERY_CLOSEST)'s record, and a ray with at most 32 hits has the slots pt_trace_rays_k(k = 32)
 *   gives it.  d_detail4 (may be NULL): pt_trace_rays_k's 4 floats per slot, d_detail4[s * 4 ..] for record s; miss slots hold zeros.
 * pt_within_radius_list: the same with C(p) and f of the section "K nearest and counts within a radius", its order (f ascending, among
 *   equal f the larger index first) and pt_nearest_k's 8-float detail record, d_detail8[s * 8 ..].  An infinite radius lists every
 *   primitive.
 * Stream order, concurrency, batching (at most 2^30 queries per launch) and the treatment of non-finite input are those of
 *   pt_trace_rays_k / pt_nearest_k (a query whose list is unspecified keeps every prim in [-1, number of primitives) and writes its own
 *   segment only); the known defect of DESIGN.md section 33 applies unchanged.  Alignment: d_rays8 and d_points4 16 bytes; records,
 *   offsets and scratch 8 bytes; counts and detail 4 bytes.  pt_scene_device_bytes stays what it was.
 * NULL scene / rays / points / offsets / records / count, n < 0, cap < 0, unknown flags, a NULL scratch for n > 0 and a misaligned
 *   device pointer return PT_ERR_INVALID before any HIP call, no pointer dereferenced, the message naming the entry point.  n = 0 returns
 *   PT_OK without a HIP call, pt_list_offsets after writing its one 0.
 * pt_trace_rays_list_host, pt_within_radius_list_host: upload, count, scan and fill on the NULL stream, wait and download.  h_offsets
 *   (n + 1 records) is always written.  With the records pointer NULL the call stops after the offsets: the sizing call.  With
 *   cap < h_offsets[n] it returns PT_ERR_INVALID, the offsets written.  The records of every segment go to h_hits / h_out [0, h_offsets[n]).
 * Cost (measured on an MI355X, 69,576 triangles): the fill walks the tree again, so count + offsets + fill costs
 *   1.7 to 2.3 times the count alone on 2 M rays (0.55 / 1.79 / 1.69 ms on camera / bounce / segment rays) and 2.7 times on 2 M points at
 *   a median of 8 members (9.2 ms), 0.58 to 0.86 times count + pt_trace_rays_k / pt_nearest_k (k = 32).  Lists of the whole scene for
 *   4,096 points (285 M records) take 248 ms, 3.7 times the count.  A segment smaller than its list still walks the whole tree.
 * Out of scope: a defined choice of members for an undersized segment, tmin, primitive masks, the 29-float surface record per slot, a
 * per-slot owner array, a CLI option, a multi-GPU split.
 * -------------------------------------------------------------------------------- */
PT_API int64_t pt_list_offsets_scratch_bytes(int64_t n);                 /* or -1 (n < 0) */
PT_API int  pt_list_offsets(const int32_t* d_count, int64_t n, int64_t* d_offsets /* n + 1 */, void* d_scratch, void* hip_stream);
PT_API int  pt_trace_rays_list(PtScene* s, const float* d_rays8, int64_t n, int32_t flags, const int64_t* d_offsets /* n + 1 */,
                               int64_t cap, PtRayHit* d_hits /* cap */, float* d_detail4 /* cap * 4, may be NULL */, void* hip_stream);
PT_API int  pt_within_radius_list(PtScene* s, const float* d_points4, int64_t n, const int64_t* d_offsets /* n + 1 */,
                                  int64_t cap, PtNearest* d_out /* cap */, float* d_detail8 /* cap * 8, may be NULL */, void* hip_stream);
PT_API int  pt_trace_rays_list_host(PtScene* s, const float* h_rays8, int64_t n, int32_t flags, int64_t* h_offsets /* n + 1, written */,
                                    int64_t cap, PtRayHit* h_hits /* may be NULL */, float* h_detail4 /* may be NULL */);
PT_API int  pt_within_radius_list_host(PtScene* s, const float* h_points4, int64_t n, int64_t* h_offsets, int64_t cap,
                                       PtNearest* h_out /* may be NULL */, float* h_detail8 /* may be NULL */);

/* ----------------------------------------------------------------------------------
 * Query filters (new: the reference has no such query).  Opt-in: every call above is as it was.
 * Each of the eight device queries above answers over every primitive and from t = 0.  These are the same eight over a SUBSET
 * (csrc/pt_lists.h: Filtered): visibility between surface points (a ray that ignores the primitive it starts on), the nearest OTHER
 * triangle from a mesh vertex, collision probes against "the moving mesh but not the room", range simulation through a window.
 * DESIGN.md section 40.
 *
 * PtQueryFilter is a HOST struct, read during the call; its three pointers are DEVICE pointers on the scene's device, 4-byte aligned,
 *   read by the kernels in stream order (they must stay valid, and unchanged, until the stream has passed the query):
 *     d_prim_bits   one word per primitive, in primitive order: triangles in the order of `tris`, then spheres (number of triangles +
 *                   number of spheres words).  NULL: all 32 bits for every primitive.
 *     d_query_bits  one word per ray / point.  NULL: `bits` for every query.
 *     d_skip_prim   one int per ray / point: that primitive is no member for that query.  Any value outside [0, number of primitives)
 *                   skips none.  NULL: none.
 *     bits          the mask of every query when d_query_bits is NULL.
 *     flags         0 or PT_FILTER_TMIN.  PT_FILTER_TMIN (ray queries only): the 7th float of the RAY8 record, the oracle's tmin, which
 *                   every other call does not read, is the ray's near bound.
 *   pt_query_filter_default writes NULL, NULL, NULL, 0xFFFFFFFF, 0: the neutral filter.  A NULL `filter` argument is the neutral filter.
 *   The filter is stateless: the scene stores nothing, nothing is allocated, pt_scene_device_bytes stays what it was, a caller may keep
 *   several groupings of one scene, and vertex updates, material updates and the three rebuilds cannot interact with it — primitive
 *   numbers survive them.
 * Definition, without reference to any tree.  Let H(i) be the set the matching section above defines for query i: for a ray query the
 *   (t, prim, facing) records in [0, tmax] under the call's `flags` (pt_trace_rays_f: PT_HITS_FRONT); for a point query the (f, prim)
 *   with f <= r2.  With m_i = d_query_bits ? d_query_bits[i] : bits and skip_i = d_skip_prim ? d_skip_prim[i] : -1, the filtered set
 *   H'(i) holds the members of H(i) for which ALL of
 *     (prim_bits[prim] & m_i) != 0
 *     prim != skip_i
 *     with PT_FILTER_TMIN:  !(t < tmin_i), compared as floats — a member at exactly tmin is kept
 *   hold.  H' is a pure selection from H: tmin does not change which root of a sphere the front-face rule picks for [0, tmax] (a sphere
 *   whose entering root lies in [0, tmin) has no member under PT_HITS_FRONT; under PT_HITS_BOTH_SIDES its leaving root remains).  A tmin
 *   that is negative or not finite leaves THAT ray's result unspecified, as a bad ray does.
 * Every filtered call returns for H' exactly what its twin returns for H: the same order, the same tie rule (larger prim first), the
 *   same miss record (0, -1), the same bits of t and f, the same detail and surface records.
 *     pt_trace_rays_f           pt_trace_rays:  PT_QUERY_CLOSEST returns the first member of H'; PT_QUERY_ANY returns prim >= 0 exactly when
 *                               H' is not empty, and then some member of H'.  d_surface29 as in the twin.
 *     pt_trace_rays_k_f         pt_trace_rays_k        pt_count_hits_f      pt_count_hits      pt_trace_rays_list_f      pt_trace_rays_list
 *     pt_closest_points_f       pt_closest_points:  closest and any-within, d_detail8 as in the twin.
 *     pt_nearest_k_f            pt_nearest_k           pt_count_within_f    pt_count_within    pt_within_radius_list_f   pt_within_radius_list
 *   Each takes its twin's arguments and `filter` before the outputs.  Hence column 0 of pt_trace_rays_k_f (PT_HITS_FRONT) is
 *   pt_trace_rays_f's closest record, and every filtered result equals the selection, on the host, of the unfiltered list of the same
 *   query.  The CSR route is pt_count_*_f, pt_list_offsets, pt_*_list_f with the SAME filter: the fill's members are the count's.
 *   A filter that keeps everything — NULL, or no array, bits 0xFFFFFFFF and flags 0 — enqueues the twin's own kernels.
 * Device pointers, the caller's stream, no host wait, nothing read back, nothing allocated, batches of at most 2^30 queries, stream
 *   order, concurrency and the treatment of non-finite input: the twin's.  The known defect of DESIGN.md section 33 applies unchanged.
 * Argument checks: the twin's, in the twin's order; after them unknown filter flags, PT_FILTER_TMIN on a point query, and a filter array
 *   that is not 4-byte aligned return PT_ERR_INVALID — all before any HIP call, no device pointer dereferenced, the message naming the
 *   entry point.  n = 0 returns PT_OK without a HIP call.
 * Cost: only a candidate the query would take pays the filter — one 4-byte gather of d_prim_bits[prim] after a
 *   test on registers —, but a filtered-out primitive never tightens a bound, so a selective filter makes the walk visit what an
 *   unfiltered walk would have culled behind it.  Measured on an MI355X (69,576 triangles, 2 M rays or points): with nothing filtered out
 *   the K, count and list calls cost 1.02 to 1.09 times their twins, the closest and any forms 1.01 to 1.20 times; with half of the
 *   primitives masked the closest forms cost 1.12 to 1.85 times the unfiltered closest query, the K, count and list calls 0.90 to 1.34
 *   times.  An any form stops at its first MEMBER, so a selective mask costs it most: up to 5.6 times on camera rays with half masked
 *   (0.21 ms for 2 M rays: the filtered closest hit's cost).  Every filtered call is cheaper than listing every member
 *   (pt_trace_rays_list, pt_within_radius_list) and selecting on the host.
 * Out of scope: node-level mask culling (an OR of the masks below every node of both trees, kept up by every set, refit and rebuild:
 *   the follow-up once a selective mask's cost is known), masks in renders and in pt_aov_rays, _host variants (the shared host staging
 *   takes one input array; Python stages numpy input through torch), hit callbacks, a multi-GPU split, a CLI option.
 * -------------------------------------------------------------------------------- */
#define PT_FILTER_TMIN 1u
typedef struct PtQueryFilter {
    const uint32_t* d_prim_bits;
    const uint32_t* d_query_bits;
    const int32_t*  d_skip_prim;
    uint32_t bits;
    uint32_t flags;
} PtQueryFilter;                                                     /* 32 bytes */
PT_API void pt_query_filter_default(PtQueryFilter* f);
PT_API int  pt_trace_rays_f(PtScene* s, const float* d_rays8, int64_t n, int32_t mode, const PtQueryFilter* filter, PtRayHit* d_hits,
                            float* d_surface29 /* may be NULL */, void* hip_stream);
PT_API int  pt_trace_rays_k_f(PtScene* s, const float* d_rays8, int64_t n, int32_t k, int32_t flags, const PtQueryFilter* filter,
                              PtRayHit* d_hits /* n * k */, float* d_detail4 /* n * k * 4, may be NULL */, void* hip_stream);
PT_API int  pt_count_hits_f(PtScene* s, const float* d_rays8, int64_t n, int32_t flags, const PtQueryFilter* filter, int32_t* d_count, void* hip_stream);
PT_API int  pt_trace_rays_list_f(PtScene* s, const float* d_rays8, int64_t n, int32_t flags, const int64_t* d_offsets /* n + 1 */, int64_t cap,
                                 const PtQueryFilter* filter, PtRayHit* d_hits /* cap */, float* d_detail4 /* cap * 4, may be NULL */, void* hip_stream);
PT_API int  pt_closest_points_f(PtScene* s, const float* d_points4, int64_t n, int32_t mode, const PtQueryFilter* filter, PtNearest* d_out,
                                float* d_detail8 /* may be NULL */, void* hip_stream);
PT_API int  pt_nearest_k_f(PtScene* s, const float* d_points4, int64_t n, int32_t k, const PtQueryFilter* filter, PtNearest* d_out /* n * k */,
                           float* d_detail8 /* n * k * 8, may be NULL */, void* hip_stream);
PT_API int  pt_count_within_f(PtScene* s, const float* d_points4, int64_t n, const PtQueryFilter* filter, int32_t* d_count, void* hip_stream);
PT_API int  pt_within_radius_list_f(PtScene* s, const float* d_points4, int64_t n, const int64_t* d_offsets /* n + 1 */, int64_t cap,
                                    const PtQueryFilter* filter, PtNearest* d_out /* cap */, float* d_detail8 /* cap * 8, may be NULL */, void* hip_stream);

/* ----------------------------------------------------------------------------------
 * Box queries (new: the reference has no such query).  Opt-in: every call above is as it was.
 * The third shape of a BVH query set: after what lies along a RAY and what lies near a POINT, what lies in a REGION, an axis-aligned
 * box of the caller's (csrc/pt_box.hip, csrc/pt_box.h): voxelising the resident (and moving) scene into an occupancy grid, selecting
 * every triangle in a box or above a plane, the broad phase "does anything reach into this cell".  DESIGN.md section 41.
 *
 * Boxes are BOX8 records: lo.xyz | reserved | hi.xyz | reserved, 32 bytes, 16-byte aligned; the two reserved floats are not read.
 *   Primitives are numbered as in pt_trace_rays: triangles first, in the order of `tris`, spheres after them.
 * Arithmetic: IEEE float32, every operation below rounded once and none contracted, in the order written; dot, cross, min, max and
 *   boxdist2 are those of the section "Closest-point queries".
 * The class key g(Q, k) of box Q = (lo, hi) and primitive k takes one of three values: 0 = inside, 1 = touching, +inf = no member.
 *   valid = lo.x <= hi.x && lo.y <= hi.y && lo.z <= hi.z.  An invalid box has no member: g = +inf for every k.  That covers an inverted
 *   box and any NaN coordinate (a comparison with NaN is false).  lo == hi on an axis is allowed: a slice, a point.
 * g(Q, k) for triangle k, V0 E1 E2 as in the closest-point section:  a = V0, ab = E1, ac = E2, b = a + ab, c = a + ac
 *     1. tlo, thi = component-wise min(min(a, b), c), max(max(a, b), c)      (exactly the box f's last line computes)
 *     2. unless tlo <= hi && thi >= lo on every axis:  g = +inf
 *     3. if tlo >= lo && thi <= hi on every axis:  g = 0
 *     4. if any of the six coordinates of Q is infinite:  g = 1, and step 5 is skipped.  A box bounded on ONE axis only — a half-space,
 *        a slab — is then answered exactly (a triangle's extent on one axis is an interval).  A box that is bounded on two or three
 *        axes and infinite elsewhere — a COLUMN, infinite on one axis only; a quadrant — is answered CONSERVATIVELY: a triangle whose
 *        own box overlaps Q but which passes Q by diagonally is reported as touching.
 *     5. the separating axes, with bc = ac - ab:
 *          ctr = (lo + hi) * 0.5;  h = max(hi - ctr, ctr - lo) per axis;  v0 = a - ctr, v1 = b - ctr, v2 = c - ctr
 *          plane:  n = cross(ab, ac);  d = dot(n, v0);  r = (h.x*|n.x| + h.y*|n.y|) + h.z*|n.z|;  separates when |d| > r
 *          edges:  for e in the order ab, ac, bc and for axis i in x, y, z, with (j, k) the next two axes cyclically:
 *                    p_m = v_m[k]*e[j] - v_m[j]*e[k]  for m = 0, 1, 2;   rr = h[j]*|e[k]| + h[k]*|e[j]|
 *                    separates when min(min(p0, p1), p2) > rr || max(max(p0, p1), p2) < -rr
 *          g = +inf if any of the ten separates, else 1
 *   Every comparison is inclusive: touching counts.  A zero-area triangle has n = 0, so its plane never separates: it is judged by
 *   the boxes and the edge axes.  Step 2 is a FLOOR, as the last line of f is: a member's own box overlaps Q, compared without any
 *   rounding in between, and every widened box of either tree contains the boxes of the records below it — so
 *   a walk that culls by the same per-axis overlap test never disagrees with this definition, and the answer is the same bits before
 *   and after a refit or any rebuild.
 * g(Q, k) for sphere j (k = number of triangles + j), center c, radius rad; membership refers to the sphere's SURFACE, as
 *   pt_closest_points measures to the surface:
 *     if c - rad >= lo && c + rad <= hi on every axis:  g = 0
 *     else  near2 = boxdist2(c, lo, hi);  far2 = (gx*gx + gy*gy) + gz*gz with g_axis = max(|lo - c|, |hi - c|);  rr = rad * rad
 *           g = 1 if near2 <= rr && far2 >= rr, else +inf      (a box strictly inside the ball touches no surface)
 * Members: B(Q) = { k : g(Q, k) <= bound }, bound = 1 for PT_BOX_TOUCHING (flags 0: inside or touching), 0 for PT_BOX_INSIDE (flags 1).
 *   Order: g ascending — inside first —, among equal g the larger primitive index first: the one order of the lists above.
 * Overflow: coordinates so large that a product or sum of step 5 overflows float32 leave THAT pair's class unspecified; every prim
 *   stays in [-1, number of primitives) and every count in [0, number of primitives].
 * pt_box_count: d_count[i] = |B(Q_i)|.
 * pt_box_any:   d_out[i].prim >= 0 exactly when pt_box_count of the same box, flags and filter is above 0; the record is then SOME
 *   member, (g(Q, prim), prim) with its own cls bits; which member is unspecified and may change between versions (the walk stops at
 *   the first).  No member: the miss record (0, -1).
 * pt_box_list:  the segment of box i is [b, e) with b = clamp(d_offsets[i], 0, cap) and e = clamp(d_offsets[i + 1], b, cap), as
 *   pt_trace_rays_list states it: no record outside the segments is written, whatever the offsets hold, never one outside [0, cap).
 *   With m = e - b:  m >= |B|: slots 0 .. |B| - 1 hold B in order, the later slots the miss record (0, -1);  m < |B|: the m slots hold
 *   m distinct members of B, sorted among themselves; which members is unspecified.
 *   The CSR route: pt_box_count, pt_list_offsets, pt_box_list with the SAME flags and filter — the records are then the concatenation
 *   of every B, bit for bit brute force over the scene's current positions.
 * filter (may be NULL): a PtQueryFilter exactly as the section above takes it — primitive masks, per-query masks, one skipped
 *   primitive per box; a filtered-out primitive is no member.  PT_FILTER_TMIN does not apply.  A filter that keeps everything runs the
 *   unfiltered kernels.
 * pt_box_count, pt_box_any, pt_box_list: d_boxes8 (16-byte aligned), d_out (8-byte aligned), d_offsets (8-byte aligned) and d_count
 *   (4-byte aligned) are DEVICE pointers on the scene's device.  Everything is enqueued on `hip_stream`: no host wait, nothing is read
 *   back, nothing is allocated (pt_scene_device_bytes stays what it was); batches of at most 2^30 boxes go per launch.  A query
 *   enqueued after pt_scene_update_vertices, pt_scene_rebuild_tree, pt_scene_rebuild_tree_ex or pt_scene_rebuild_tree_opt on the same
 *   stream sees their result.  The buffers must stay valid until the stream has passed the query.  A query leaves every render state
 *   alone: frames, pt_last_iterations, pt_last_counters, pt_last_render_ms.  Concurrency: ONE query, update or render at a time per
 *   scene.
 * pt_box_count_host, pt_box_any_host, pt_box_list_host: the same on HOST arrays, without a filter (as the section above rules for
 *   _host variants): upload, query on the NULL stream, wait and download.  pt_box_list_host follows pt_within_radius_list_host:
 *   h_offsets (n + 1) is always written; with h_out NULL the call stops there (the sizing call); with cap < h_offsets[n] it returns
 *   PT_ERR_INVALID, the offsets written.
 * Argument checks, in the order of every query: NULL scene / boxes / offsets / out / count, n < 0, cap < 0, unknown flags, then the
 *   alignments, then the filter's (unknown filter flags, PT_FILTER_TMIN, a misaligned filter array) return PT_ERR_INVALID before any
 *   HIP call, no pointer dereferenced, the message naming the entry point.  n = 0 returns PT_OK without a HIP call.
 * The walk ends whatever the floats are, by the argument of quad_step (csrc/pt_trace.h): depth-first over a finite tree, its stack
 *   bounded by the depth of the tree.
 * Cost: a box's cost is the number of tree nodes its box overlaps plus one key per triangle below an
 *   overlapping leaf; every lane walks alone, so one box that holds thousands of primitives holds its wave for that long — the
 *   caller's cost, as an infinite radius is.  A box query is the right call when the region IS a box (a voxel, a cell, a selection
 *   rectangle, a half-space): pt_count_within on the bounding ball over-reports by the ball's corners, overlaps more of the tree and
 *   needs a host pass to tell; when the region is a ball, pt_count_within is.  Measured on an MI355X (69,576 triangles, 2 M boxes): the
 *   voxels of a 128^3 grid over the scene, 95 % of them empty, count in 0.52 ms (pt_count_within on their bounding balls: 0.68 ms, and
 *   1.65 times as many primitives reported), any in 0.12 ms, count + offsets + fill in 1.3 ms; voxel-sized boxes ON the surface, 21
 *   members each, count in 3.7 ms, any in 0.30 ms, count + offsets + fill (45 M records) in 12.4 ms.
 * Out of scope: oriented boxes, frusta and general convex regions (the next section); detail records per member; a wave-cooperative walk for boxes that
 *   hold thousands of members; node-level mask culling; _host variants with filters; a multi-GPU split; a CLI option.
 * -------------------------------------------------------------------------------- */
typedef struct PtBoxMember { float cls; int32_t prim; } PtBoxMember;   /* 8 bytes; a miss is (0, -1) */
#define PT_BOX_TOUCHING 0
#define PT_BOX_INSIDE   1
PT_API int  pt_box_count(PtScene* s, const float* d_boxes8, int64_t n, int32_t flags, const PtQueryFilter* filter /* may be NULL */,
                         int32_t* d_count, void* hip_stream);
PT_API int  pt_box_any(PtScene* s, const float* d_boxes8, int64_t n, int32_t flags, const PtQueryFilter* filter /* may be NULL */,
                       PtBoxMember* d_out /* n */, void* hip_stream);
PT_API int  pt_box_list(PtScene* s, const float* d_boxes8, int64_t n, int32_t flags, const int64_t* d_offsets /* n + 1 */, int64_t cap,
                        const PtQueryFilter* filter /* may be NULL */, PtBoxMember* d_out /* cap */, void* hip_stream);
PT_API int  pt_box_count_host(PtScene* s, const float* h_boxes8, int64_t n, int32_t flags, int32_t* h_count);
PT_API int  pt_box_any_host(PtScene* s, const float* h_boxes8, int64_t n, int32_t flags, PtBoxMember* h_out);
PT_API int  pt_box_list_host(PtScene* s, const float* h_boxes8, int64_t n, int32_t flags, int64_t* h_offsets /* n + 1, written */, int64_t cap,
                             PtBoxMember* h_out /* may be NULL */);

/* ----------------------------------------------------------------------------------
 * Convex-region queries (new: the reference has no such query).  Opt-in: every call above is as it was.
 * The regions a caller who also renders actually has: the frustum of a pixel window of a camera (a marquee selection, view-frustum
 * culling of the resident, moving scene per camera, per 8 x 8 tile, per view of a batch), an oriented bounding box of a tool, a
 * vehicle or a sensor, a light's or a portal's pyramid (csrc/pt_convex.hip, csrc/pt_convex.h).  DESIGN.md section 42.
 *
 * A region is the intersection of m half-spaces, m = n_planes, ONE value per call in 1 .. PT_CONVEX_MAX_PLANES (8).  Region i reads m
 *   PLANE4 records n.xyz | d at d_planes4 + (i * m + j) * 4 floats, j = 0 .. m - 1; the array is 16-byte aligned.  A point x is inside
 *   plane j when s_j(x) <= d_j with  s_j(x) = (n.x*x.x + n.y*x.y) + n.z*x.z.
 *   Primitives are numbered as in pt_trace_rays: triangles first, in the order of `tris`, spheres after them.
 * Arithmetic: IEEE float32, every operation below rounded once and none contracted, in the order written.
 * Normals need not be unit.  A plane (0, 0, 0, d >= 0) is neutral (a region of fewer planes is padded with it), as is d = +inf;
 *   (0, 0, 0, d < 0) and d = -inf make the region empty.
 *   valid = every normal component of the region's m planes is finite.  An invalid region has no member: h = +inf for every k.  A NaN d
 *   needs no rule: s <= NaN is false, so everything is outside.
 * The class key h(Q, k) of region Q and primitive k takes one of three values: 0 = inside, 1 = touching, +inf = no member.
 * h(Q, k) for triangle k, V0 E1 E2 as in the closest-point section:  a = V0, b = a + E1, c = a + E2 (the record's own floats, exactly
 *   as the box section forms them);  in_j(v) = s_j(v) <= d_j
 *     1. if some j has none of in_j(a), in_j(b), in_j(c):  h = +inf
 *     2. else if every j has all three:  h = 0
 *     3. else h = 1
 * h(Q, k) for sphere j (k = number of triangles + j), center c, radius rad; membership refers to the sphere's SURFACE:
 *     len_j = sqrtf((n.x*n.x + n.y*n.y) + n.z*n.z);  r_j = rad * len_j;  sc_j = s_j(c)
 *     1. if some j has !(sc_j - r_j <= d_j):  h = +inf
 *     2. else if every j has sc_j + r_j <= d_j:  h = 0
 *     3. else h = 1
 *   Class 1 is CONSERVATIVE: a triangle that straddles two planes near an edge or a corner of the region, yet passes the region by,
 *   is reported as touching (no plane of the region separates it; an edge-edge axis would), and a region wholly inside a ball is
 *   reported as touching that sphere — as the box section's column case over-reports.  Class 0 is exact.  A region of one plane (a
 *   half-space) or of two parallel planes (a slab) is answered exactly.  DESIGN.md section 42 has the measured share of over-reports.
 *   Rule 1 is a FLOOR: s_j at the corner of a box that minimises it — per axis lo where n >= 0, hi otherwise — is, in float32 and with
 *   no slack, at most s_j of every float point of the box, because rounding to nearest is monotone; every widened box of either tree
 *   contains the boxes of the records below it.  So a walk that culls a node by that corner never disagrees
 *   with this definition, and the answer is the same bits before and after a refit or any rebuild.
 * Members: C(Q) = { k : h(Q, k) <= bound }, bound = 1 for PT_CONVEX_TOUCHING (flags 0: inside or touching), 0 for PT_CONVEX_INSIDE
 *   (flags 1).  Order: h ascending — inside first —, among equal h the larger primitive index first: the one order of the lists above.
 *   Records are PtBoxMember.
 * Overflow: coordinates so large that a product or sum overflows float32 leave THAT pair's class unspecified; every prim stays in
 *   [-1, number of primitives) and every count in [0, number of primitives].
 * pt_convex_count: d_count[i] = |C(Q_i)|.
 * pt_convex_any:   d_out[i].prim >= 0 exactly when pt_convex_count of the same region, flags and filter is above 0; the record is then
 *   SOME member, (h(Q, prim), prim) with its own cls bits; which member is unspecified and may change between versions (the walk stops
 *   at the first).  No member: the miss record (0, -1).
 * pt_convex_list:  the segment of region i is [b, e) with b = clamp(d_offsets[i], 0, cap) and e = clamp(d_offsets[i + 1], b, cap), as
 *   pt_trace_rays_list states it: no record outside the segments is written, whatever the offsets hold, never one outside [0, cap).
 *   With len = e - b:  len >= |C|: slots 0 .. |C| - 1 hold C in order, the later slots the miss record (0, -1);  len < |C|: the len
 *   slots hold len distinct members of C, sorted among themselves; which members is unspecified.
 *   The CSR route: pt_convex_count, pt_list_offsets, pt_convex_list with the SAME n_planes, flags and filter — the records are then the
 *   concatenation of every C, bit for bit brute force over the scene's current positions.
 * filter (may be NULL): a PtQueryFilter exactly as the section "Query filters" takes it — primitive masks, per-query masks, one skipped
 *   primitive per region; a filtered-out primitive is no member.  PT_FILTER_TMIN does not apply.  A filter that keeps everything runs
 *   the unfiltered kernels.
 * pt_convex_count, pt_convex_any, pt_convex_list: d_planes4 (16-byte aligned), d_out (8-byte aligned), d_offsets (8-byte aligned) and
 *   d_count (4-byte aligned) are DEVICE pointers on the scene's device.  Everything is enqueued on `hip_stream`: no host wait, nothing is
 *   read back, nothing is allocated (pt_scene_device_bytes stays what it was); batches of at most 2^30 regions go per launch.  A query
 *   enqueued after pt_scene_update_vertices, pt_scene_rebuild_tree, pt_scene_rebuild_tree_ex or pt_scene_rebuild_tree_opt on the same
 *   stream sees their result.  The buffers must stay valid until the stream has passed the query.  A query leaves every render state
 *   alone: frames, pt_last_iterations, pt_last_counters, pt_last_render_ms.  Concurrency: ONE query, update or render at a time per
 *   scene.
 * pt_convex_count_host, pt_convex_any_host, pt_convex_list_host: the same on HOST arrays, without a filter (as the _host variants of
 *   the box section): upload, query on the NULL stream, wait and download.  pt_convex_list_host follows pt_box_list_host: h_offsets
 *   (n + 1) is always written; with h_out NULL the call stops there (the sizing call); with cap < h_offsets[n] it returns
 *   PT_ERR_INVALID, the offsets written.
 * Argument checks, in the order of every query: NULL scene / planes / offsets / out / count, n < 0, cap < 0, n_planes outside 1 .. 8,
 *   unknown flags, then the alignments (planes 16, offsets 8, out 8, count 4), then the filter's (unknown filter flags,
 *   PT_FILTER_TMIN, a misaligned filter array) return PT_ERR_INVALID before any HIP call, no pointer dereferenced, the message naming
 *   the entry point.  n = 0 returns PT_OK without a HIP call, but does not excuse a NULL.
 * The walk ends whatever the floats are, by the argument of quad_step (csrc/pt_trace.h): depth-first over a finite tree, its stack
 *   bounded by the depth of the tree.
 * pt_camera_frustum (host only, no HIP call): the six planes of the half-open pixel window [x0, x1) x [y0, y1) of `cam`, in the order
 *   left, right, top, bottom, near, far, as 24 floats for n_planes = 6.  0 <= x0 < x1 <= W and 0 <= y0 < y1 <= H; the four are floats, so
 *   that a caller can widen a window by a fraction of a pixel; the sample of pixel (px, py) at offset (u1, u2) is the screen position
 *   (px + u1, py + u2).  Computed in float64 from the camera's float32 fields and rounded once to float32:
 *     the direction at screen position (fx, fy) is  F + (2 (fx/(W-1) - 0.5) tx) R + (-2 (fy/(H-1) - 0.5) ty) U  with tx, ty the float32
 *     half-angle tangents of a render of `cam` (the device's pixel_direction uses the same); a side plane contains cam->pos and the two
 *     corner directions of its side, its normal (not unit) oriented so that the direction at the window's centre is inside,
 *     d = n . pos; near is (-F^, -(F^ . pos + near)) and far (F^, F^ . pos + far) with F^ = F / |F|; near < 0 or far = +inf gives the
 *     neutral plane (0, 0, 0, +inf) in that place.
 *   Two windows that share a side (x1 of one is x0 of the other, the same y0, y1) get that plane with the same bits up to sign.
 *   PT_ERR_INVALID: a NULL, a bad window, W or H below 2, a NaN near or far, near > far, a camera field that is not finite, a zero
 *   forward vector, a degenerate side.
 * Cost: as a box's — the nodes the region may reach plus one key per triangle below such a leaf —, a node test
 *   and a key each costing m plane evaluations; every lane walks alone, so one region that holds thousands of primitives holds its
 *   wave for that long: the whole-frame frustum is a query for one lane, the caller's cost.  Measured on an MI355X (69,576
 *   triangles): the 32,400 frusta of the 8 x 8 tiles of a 1080p camera count in 2.05 ms, any in 0.14 ms, count + offsets + fill
 *   (196,147 records) in 4.4 ms; the 2 M voxels of a 128^3 grid as six planes each count in 0.68 ms, where pt_box_count of the same
 *   boxes takes 0.50 ms and reports 0.69 times as many members (when the region IS an axis-aligned box, pt_box_count is the call);
 *   2 M voxel-sized oriented boxes on the surface, 25 members each, count in 7.7 ms, any in 1.2 ms, count + offsets + fill (52.5 M
 *   records) in 22.5 ms.
 * Out of scope: an exact class 1 (clipping the triangle against the region, or the remaining separating axes); more than 8 planes; a
 *   per-query plane count; non-convex regions; detail records per member; a wave-cooperative walk for regions that hold thousands of
 *   members; node-level mask culling; _host variants with filters; a multi-GPU split; a ptrender option.
 * -------------------------------------------------------------------------------- */
#define PT_CONVEX_TOUCHING   0
#define PT_CONVEX_INSIDE     1
#define PT_CONVEX_MAX_PLANES 8
PT_API int  pt_convex_count(PtScene* s, const float* d_planes4, int64_t n, int32_t n_planes, int32_t flags, const PtQueryFilter* filter /* may be NULL */,
                            int32_t* d_count, void* hip_stream);
PT_API int  pt_convex_any(PtScene* s, const float* d_planes4, int64_t n, int32_t n_planes, int32_t flags, const PtQueryFilter* filter /* may be NULL */,
                          PtBoxMember* d_out /* n */, void* hip_stream);
PT_API int  pt_convex_list(PtScene* s, const float* d_planes4, int64_t n, int32_t n_planes, int32_t flags, const int64_t* d_offsets /* n + 1 */,
                           int64_t cap, const PtQueryFilter* filter /* may be NULL */, PtBoxMember* d_out /* cap */, void* hip_stream);
PT_API int  pt_convex_count_host(PtScene* s, const float* h_planes4, int64_t n, int32_t n_planes, int32_t flags, int32_t* h_count);
PT_API int  pt_convex_any_host(PtScene* s, const float* h_planes4, int64_t n, int32_t n_planes, int32_t flags, PtBoxMember* h_out);
PT_API int  pt_convex_list_host(PtScene* s, const float* h_planes4, int64_t n, int32_t n_planes, int32_t flags, int64_t* h_offsets /* n + 1, written */,
                                int64_t cap, PtBoxMember* h_out /* may be NULL */);
PT_API int  pt_camera_frustum(const PtCamera* cam, float x0, float y0, float x1, float y1, float near_dist, float far_dist, float* planes24 /* 24, written */);

/* ----------------------------------------------------------------------------------
 * Sphere casts (new: the reference has no such query).  Opt-in: every call above is as it was.
 * The query a collision user needs first: how far a body of some size can travel before it touches the scene (csrc/pt_sweep.hip,
 * csrc/pt_sweep.h) — the end cap of a character's capsule, a camera boom, a tool tip, a LiDAR beam with divergence, clearance along a
 * path — against a mesh that pt_scene_update_vertices moves.  A ray has no thickness, pt_closest_points no motion, and points stepped
 * along the segment tunnel through thin geometry.  DESIGN.md section 43.
 *
 * Sweeps are SWEEP8 records: org.xyz | radius | dir.xyz | tmax, 32 bytes, the array 16-byte aligned.  The sphere of that radius has its
 *   centre at o + t d for t in [0, tmax]; the direction is used as given and is NOT normalised, t is the parameter along it.
 *   radius >= 0, and 0 is a two-sided thin ray; tmax >= 0, +inf allowed.  A zero direction is a sphere that stands still: only the
 *   overlap rule (step 1) can make a member.  Results are PtRayHit (t, prim); primitives are numbered as in pt_trace_rays: triangles
 *   first, in the order of `tris`, spheres after them; a miss is (0, -1).  Nothing is culled by facing, and the reference's leaf boxes
 *   play no part.
 * Arithmetic: IEEE float32, every operation below rounded once and none contracted, in the order written.  dot, cross, f, sphere_f
 *   (the f of a sphere) and boxdist2 are those of the section "Closest-point queries".  min and max are selects,
 *     min(a, b) = (b < a) ? b : a      max(a, b) = (b > a) ? b : a
 *   with several arguments from the left, min(min(a, b), c): one answer for a NaN and for zeros of either sign.
 *   o, d, r, tmax are the record's fields, r2 = r * r, NOW = 2^-126 (the smallest positive normal float).
 * first(m, dv, R2): the first touch of the line m + t dv with the ball of squared radius R2 about 0, by the closest approach:
 *     A = dot(dv, dv);  t0 = -dot(m, dv) / A;  w = m + t0 * dv;  k = R2 - dot(w, w);  t = t0 - sqrt(k / A)
 *     first = max(NOW, t) when A > 0 && k >= 0 && t0 >= 0, else +inf
 *   (Not the textbook b^2 - a c form: in float32 that left a residual |dist - r| of 3 * 10^-4 at coordinates of magnitude 4 and radius
 *   0.01, this form 1.6 * 10^-6.)  A line that is inside the ball already by these floats and still approaches its middle touches NOW.
 * tau(S, k) for triangle k, V0 E1 E2 as in the closest-point section:  a = V0, ab = E1, ac = E2, b = a + ab, c = a + ac, bc = ac - ab
 *     1. Overlap.  If f(o, k) <= r2:  tau = 0, and steps 2 to 4 play no part.  So tau = 0 for exactly the primitives pt_count_within
 *        counts for the point (o, r), bit for bit — and for no other: every contact below is at NOW or later.
 *     2. Floor.  tlo, thi = the record's own box as f's last line forms it; lo' = tlo - r, hi' = thi + r.  Per axis with d != 0:
 *        inv = 1 / d, t1 = (lo' - o) * inv, t2 = (hi' - o) * inv, near = min(t1, t2), far = max(t1, t2).  An axis with d == 0 passes
 *        iff lo' <= o && o <= hi' and has no near or far.  tn = max(0, near_x, near_y, near_z), tf = min(tmax, far_x, far_y, far_z)
 *        over the axes that have them.  Unless every d == 0 axis passes and tn <= tf:  tau = +inf.
 *     3. Candidates.
 *        Face:  n = cross(ab, ac), nn = dot(n, n), h = dot(o - a, n), dn = dot(d, n), s = (h >= 0) ? 1 : -1, ln = sqrt(nn),
 *          g = s*h - r*ln.  When nn > 0 && s*dn < 0:  t = max(NOW, g > 0 ? g / -(s*dn) : 0),  q = (o + t*d) - ((s*r)/ln) * n; the
 *          candidate t is taken if q passes the three edge-function tests >= 0 of f's `inside` (ap = q - a).  Only the near face:
 *          a sphere that starts outside cannot reach the far offset face without first passing an edge cylinder.
 *        Edges:  for (v, e) in (a, ab), (a, ac), (b, bc) with ee = dot(e, e) > 0:  m = o - v, um = dot(m, e) / ee, ud = dot(d, e) / ee,
 *          t = first(m - um*e, d - ud*e, r2); taken if 0 <= um + t*ud && um + t*ud <= 1.
 *        Vertices:  for v in a, b, c:  first(o - v, d, r2).
 *        tau_raw = min over the at most seven, in this order from +inf.
 *     4. tau = max(tau_raw, tn) when that is <= tmax, else +inf.
 *   The floor only moves tau towards the true value: the centre at true contact lies inside the inflated box.  It is what lets a tree
 *   walk prune without ever disagreeing with this definition (below).
 * tau(S, k) for sphere j (k = number of triangles + j), center ctr, radius rad:  pc = o - ctr, l = sqrt(dot(pc, pc)), g = l - rad
 *     if g * g <= r2:  tau = 0 (contact with the SURFACE, as everywhere; this is sphere_f <= r2)
 *     else if l > rad:  R = rad + r;  tau = first(pc, d, R * R)
 *     else (deep inside the ball):  R = rad - r;  A, t0, k of first(pc, d, R * R);  tau = max(NOW, t0 + sqrt(k / A)) when A > 0 && k >= 0,
 *       else +inf
 *     tau = +inf when it exceeds tmax.
 *   tau = +inf is no member, also when tmax = +inf.
 * PT_SWEEP_CLOSEST: defined without reference to any tree.  Among the primitives k with tau(S_i, k) <= tmax, d_hits[i] = (tau, k) of the
 *   smallest tau; among equal tau the largest k (ties at tau = 0 are ordinary).  No such primitive: a miss, (0, -1).  The result is
 *   therefore bit for bit the same before and after a refit or any rebuild, and equals a brute-force evaluation over the scene's
 *   current positions.
 *   d_detail8 (may be NULL): the 8-float record of the closest-point section, c.xyz | v | w | side | feature | 0, for the winning
 *   primitive and the point  centre = o + tau * d  (one multiply and one add per axis, float32): the sphere's centre at contact.
 *   A miss gives zeros.  The contact normal is centre - c, for the caller to normalise.
 * PT_SWEEP_ANY: prim >= 0 exactly when the closest form of the same record (and filter) hits.  The record is SOME member k with
 *   tau(S, k) <= tmax and t = tau(S, k) bit for bit; which member is unspecified and may change between versions (the walk stops at
 *   the first).  d_detail8 must be NULL.
 * Why a tree walk is exact: a child box (lo, hi), decoded and widened as the closest-point walks widen it, is entered iff
 *   boxdist2(o, lo, hi) <= r2, or the test of step 2 on [lo - r, hi + r] passes with its tn not above the best tau so far (strictly:
 *   an equal tn may hide a tie).  Every operation of both is monotone in lo and hi under rounding to nearest, for fixed o, inv and r,
 *   and every widened box contains the boxes of the records below it: a parent's interval contains a child's
 *   with no slack, and a culled node holds no member that could win or tie.
 * filter (may be NULL): a PtQueryFilter exactly as the section "Query filters" takes it — primitive masks, per-query masks, one skipped
 *   primitive per sweep (the body's own triangle, say); a filtered-out primitive is no member.  PT_FILTER_TMIN does not apply and is
 *   rejected.  A filter that keeps everything runs the unfiltered kernels.
 * pt_sweep_spheres: d_sweeps8 (16-byte aligned), d_hits (8-byte aligned) and d_detail8 (4-byte aligned) are DEVICE pointers on the
 *   scene's device holding n records.  Everything is enqueued on `hip_stream`: no host wait, nothing is read back, nothing is allocated
 *   (pt_scene_device_bytes stays what it was); batches of at most 2^30 sweeps go per launch.  A query enqueued after
 *   pt_scene_update_vertices, pt_scene_rebuild_tree, pt_scene_rebuild_tree_ex or pt_scene_rebuild_tree_opt on the same stream sees
 *   their result.  The buffers must stay valid until the stream has passed the query.  A query leaves every render state alone:
 *   frames, pt_last_iterations, pt_last_counters, pt_last_render_ms.  Concurrency: ONE query, update or render at a time per scene.
 * pt_sweep_spheres_host: the same on HOST arrays, without a filter: uploads, queries on the NULL stream, waits and downloads.
 * Argument checks, in the order of every query: NULL scene / sweeps / hits, n < 0, an unknown mode, a detail buffer given with
 *   PT_SWEEP_ANY, then the alignments (sweeps 16, hits 8, detail 4), then the filter's (unknown filter flags, PT_FILTER_TMIN, a
 *   misaligned filter array) return PT_ERR_INVALID before any HIP call, no pointer dereferenced, the message naming the entry point.
 *   n = 0 returns PT_OK without a HIP call, but does not excuse a NULL.
 * A record with a non-finite coordinate, a negative or NaN radius or tmax, or a direction component that is denormal (its inverse
 *   overflows): the result for THAT record is unspecified (prim stays in [-1, number of primitives)), the other records of the batch are
 *   unaffected, and the call ends by the argument of quad_step (csrc/pt_trace.h): a depth-first walk over a finite tree, its stack
 *   bounded by the depth of the tree whatever the floats are.
 * Known limit: on a needle triangle the float32 normal is tilted (the kappa of the ray section's note), and the face candidate with
 *   it; the error of tau grows with kappa as f's does.  DESIGN.md section 43 has the measured bound per family.
 * Out of scope: contact counts, lists and the first K contacts along a sweep; capsule and box sweeps; rotation; a scene that moves
 *   during the sweep; sorting sweeps for coherence; a wave-cooperative walk; a multi-GPU split; a ptrender option.
 * -------------------------------------------------------------------------------- */
#define PT_SWEEP_CLOSEST 0
#define PT_SWEEP_ANY     1
PT_API int  pt_sweep_spheres(PtScene* s, const float* d_sweeps8, int64_t n, int32_t mode, const PtQueryFilter* filter /* may be NULL */,
                             PtRayHit* d_hits, float* d_detail8 /* may be NULL */, void* hip_stream);
PT_API int  pt_sweep_spheres_host(PtScene* s, const float* h_sweeps8, int64_t n, int32_t mode, PtRayHit* h_hits, float* h_detail8 /* may be NULL */);

/* ----------------------------------------------------------------------------------
 * Triangle queries (new: the reference has no such query).  Opt-in: every call above is as it was.
 * The fourth shape of a query: after rays, points and regions, the caller's own TRIANGLES (csrc/pt_tri.hip, csrc/pt_tri.h): which
 * primitives of the resident, moving scene the triangles of a tool, a robot link or a character mesh actually cut, and along which
 * segments — the contact curve; and the plane section of the scene (a slicer layer, a floor plan, a section view) as the segments cut
 * by a large quad of two query triangles.  pt_convex_count on a triangle written as five half-spaces is conservative near its edges
 * and returns no geometry; this is exact triangle against triangle, and returns the segments.  DESIGN.md section 44.
 *
 * Queries are TRI12 records: a.xyz | - | b.xyz | - | c.xyz | -, 48 bytes, the array 16-byte aligned; the three reserved floats are not
 *   read.  Primitives are numbered as in pt_trace_rays: triangles first, in the order of `tris`, spheres after them.  Results are
 *   PtBoxMember records (cls, prim): every member's cls is 1, a miss is (0, -1).
 * Arithmetic: IEEE float32, every operation below rounded once and none contracted, in the order written.  dot and cross are those of
 *   the section "Closest-point queries"; min and max are the selects of the section "Sphere casts", several arguments from the left.
 * Of the query T = (qa, qb, qc):  n = cross(qb - qa, qc - qa);  qlo, qhi = component-wise min(min(qa, qb), qc), max(max(qa, qb), qc);
 *   the plane function  d(v) = (n.x*(v.x - qa.x) + n.y*(v.y - qa.y)) + n.z*(v.z - qa.z);  the inward edge normals
 *   m0 = cross(n, qb - qa), m1 = cross(n, qc - qb), m2 = cross(n, qa - qc) and the edge functions
 *   w0(x) = dot(m0, x - qa), w1(x) = dot(m1, x - qb), w2(x) = dot(m2, x - qa)      (edges 0 and 2 pass through qa, edge 1 through qb).
 * Membership of triangle k, V0 E1 E2 as in the closest-point section:  a = V0, b = a + E1, c = a + E2 (the record's own floats)
 *     1. Box floor.  tlo, thi = component-wise min(min(a, b), c), max(max(a, b), c).  Unless tlo <= qhi && thi >= qlo on every axis:
 *        no member.
 *     2. Plane floor.  da = d(a), db = d(b), dc = d(c); a vertex is ABOVE when its d >= 0 (half-open: a vertex on the plane is above).
 *        Unless one vertex is above and one is not: no member.
 *     3. Section.  The lone vertex L is the one whose side differs from the other two's; (v1, v2) are the other two in cyclic order:
 *        L = a: (b, c), L = b: (c, a), L = c: (a, b).  t1 = d(L) / (d(L) - d(v1)), t2 = d(L) / (d(L) - d(v2));
 *        P = L + t1*(v1 - L), Q = L + t2*(v2 - L)      (the subtraction, then one multiply and one add per axis).
 *     4. Clip.  [s0, s1] = [0, 1].  For i = 0, 1, 2 in order:  wp = w_i(P), wq = w_i(Q).  If neither is >= 0: no member.  If exactly
 *        one is:  s = wp / (wp - wq);  wp >= 0: s1 = min(s1, s), else s0 = max(s0, s).  After the three: member iff s0 <= s1, and then
 *        PQ = Q - P,  p = P + s0*PQ,  q = P + s1*PQ,  kind = 1.
 *   Consequences of the half-open rule: a triangle lying in T's plane has every vertex above and is no member (coplanar overlap is not
 *   reported); a zero-area query has n = 0, every d = 0, every vertex above: no triangle member; a query with a NaN has every d NaN,
 *   no vertex above: no triangle member, and the other records of the batch are unaffected.  A zero-area scene triangle that pierces
 *   T is a member with p == q.  In real arithmetic steps 2 to 4 are exactly T intersected with triangle k for pairs that are not
 *   coplanar: symmetric in the two triangles, not conservative.  The section points of an edge that two scene triangles share agree
 *   within rounding, NOT bit for bit: a record stores a, E1, E2, and a + E1 is rounded, so the two records hold the shared vertices
 *   with different last bits and walk the edge from different ends.
 * Membership of sphere j (k = number of triangles + j), centre ctr, radius rad, by the SURFACE as everywhere:  with f and its closest
 *   point c of the closest-point section (the detail record's c) taken for the point ctr and the triangle (qa, qb - qa, qc - qa), min
 *   and max as selects;  far2 = max(max(|qa - ctr|^2, |qb - ctr|^2), |qc - ctr|^2), each dot(v, v);  rr = rad * rad:
 *     member iff f <= rr && far2 >= rr      (T comes within rad of the centre and is not wholly inside the ball);  p = q = c, kind = 2.
 * Members: M(T) = the members above.  Order: the larger primitive index first (every key is 1: the one order of the lists above).
 * Overflow: coordinates so large that a product or sum overflows float32 leave THAT pair unspecified; every prim stays in
 *   [-1, number of primitives) and every count in [0, number of primitives].
 * pt_tri_count: d_count[i] = |M(T_i)|.
 * pt_tri_any:   d_out[i].prim >= 0 exactly when pt_tri_count of the same record and filter is above 0; the record is then SOME member,
 *   (1, prim); which member is unspecified and may change between versions (the walk stops at the first).  No member: (0, -1).
 * pt_tri_list:  the segment of query i is [b, e) with b = clamp(d_offsets[i], 0, cap) and e = clamp(d_offsets[i + 1], b, cap), as
 *   pt_box_list states it: no record outside the segments is written, whatever the offsets hold, never one outside [0, cap).  With
 *   m = e - b:  m >= |M|: slots 0 .. |M| - 1 hold M in order, the later slots the miss record (0, -1);  m < |M|: the m slots hold m
 *   distinct members, sorted among themselves; which members is unspecified.
 *   d_detail8 (may be NULL): 8 floats per slot of every segment, p.xyz | q.xyz | kind | 0, for the member in that slot; a miss slot
 *   holds zeros.  Written by a second pass over the filled slots that evaluates the same function on the scene's current records:
 *   the same bits.  Slots outside the segments are not written.
 *   The CSR route: pt_tri_count, pt_list_offsets, pt_tri_list with the SAME filter — the records are then the concatenation of every
 *   M, bit for bit brute force over the scene's current positions.
 * Why a tree walk is exact: a child box (lo, hi), decoded and widened as the box walks widen it, is entered iff it overlaps (qlo, qhi)
 *   on every axis (inclusive) AND straddles the plane: d at the corner that minimises it — per axis lo where n >= 0, hi otherwise — is
 *   < 0 and d at the opposite corner is >= 0.  d's subtraction, three products and two sums are monotone in each coordinate under
 *   rounding to nearest; a record's vertices lie in its box; every widened box contains the boxes of the records below it (DESIGN.md
 *   section 29).  So a culled node holds no member, and the answer is the same bits before and after a refit or any rebuild.  The
 *   plane test makes a large slanted triangle — a slicing quad — walk a slab of the tree, not its whole bounding box.
 * filter (may be NULL): a PtQueryFilter exactly as the section "Query filters" takes it — primitive masks, per-query masks, one skipped
 *   primitive per query (the body's own triangle, say); a filtered-out primitive is no member.  PT_FILTER_TMIN does not apply and is
 *   rejected.  A filter that keeps everything runs the unfiltered kernels.
 * pt_tri_count, pt_tri_any, pt_tri_list: d_tris12 (16-byte aligned), d_out (8-byte aligned), d_offsets (8-byte aligned), d_count and
 *   d_detail8 (4-byte aligned) are DEVICE pointers on the scene's device.  Everything is enqueued on `hip_stream`: no host wait, nothing
 *   is read back, nothing is allocated (pt_scene_device_bytes stays what it was); batches of at most 2^30 queries go per launch.  A
 *   query enqueued after pt_scene_update_vertices, pt_scene_rebuild_tree, pt_scene_rebuild_tree_ex or pt_scene_rebuild_tree_opt on the
 *   same stream sees their result.  The buffers must stay valid until the stream has passed the query.  A query leaves every render
 *   state alone: frames, pt_last_iterations, pt_last_counters, pt_last_render_ms.  Concurrency: ONE query, update or render at a time
 *   per scene.
 * pt_tri_count_host, pt_tri_any_host, pt_tri_list_host: the same on HOST arrays, without a filter: upload, query on the NULL stream,
 *   wait and download.  pt_tri_list_host follows pt_box_list_host: h_offsets (n + 1) is always written; with h_out NULL the call stops
 *   there (the sizing call); with cap < h_offsets[n] it returns PT_ERR_INVALID, the offsets written.  h_detail8 (may be NULL): cap * 8
 *   floats, of which h_offsets[n] * 8 are written.
 * Argument checks, in the order of every query: NULL scene / tris / offsets / out / count, n < 0, cap < 0, then the alignments (tris
 *   16, offsets 8, out 8, count 4, detail 4), then the filter's (unknown filter flags, PT_FILTER_TMIN, a misaligned filter array)
 *   return PT_ERR_INVALID before any HIP call, no pointer dereferenced, the message naming the entry point.  n = 0 returns PT_OK
 *   without a HIP call, but does not excuse a NULL.  Only pt_tri_list and pt_tri_list_host take a detail buffer.
 * The walk ends whatever the floats are, by the argument of quad_step (csrc/pt_trace.h): depth-first over a finite tree, its stack
 *   bounded by the depth of the tree.
 * Cost: the tree nodes whose boxes the query's box overlaps and its plane crosses, plus one key per triangle
 *   below such a leaf; every lane walks alone, so one large query — a slicing quad through the whole scene — holds its wave for as
 *   long as its slab of the tree takes: the caller's cost, as a whole-frame frustum is.
 * Out of scope: self-intersection of the scene's own mesh (neighbours share edges: it needs an adjacency-aware rule); coplanar
 *   overlap; the circle of a sphere section; K-limited lists; a wave-cooperative walk; _host variants with filters; a multi-GPU
 *   split; a CLI option.
 * -------------------------------------------------------------------------------- */
PT_API int  pt_tri_count(PtScene* s, const float* d_tris12, int64_t n, const PtQueryFilter* filter /* may be NULL */, int32_t* d_count, void* hip_stream);
PT_API int  pt_tri_any(PtScene* s, const float* d_tris12, int64_t n, const PtQueryFilter* filter /* may be NULL */, PtBoxMember* d_out /* n */,
                       void* hip_stream);
PT_API int  pt_tri_list(PtScene* s, const float* d_tris12, int64_t n, const int64_t* d_offsets /* n + 1 */, int64_t cap,
                        const PtQueryFilter* filter /* may be NULL */, PtBoxMember* d_out /* cap */, float* d_detail8 /* cap * 8, may be NULL */,
                        void* hip_stream);
PT_API int  pt_tri_count_host(PtScene* s, const float* h_tris12, int64_t n, int32_t* h_count);
PT_API int  pt_tri_any_host(PtScene* s, const float* h_tris12, int64_t n, PtBoxMember* h_out);
PT_API int  pt_tri_list_host(PtScene* s, const float* h_tris12, int64_t n, int64_t* h_offsets /* n + 1, written */, int64_t cap,
                             PtBoxMember* h_out /* may be NULL */, float* h_detail8 /* may be NULL */);

/* ----------------------------------------------------------------------------------
 * Radiance along the caller's own rays (new: the reference reaches its integrator through a pinhole camera only).
 * Opt-in: every call above is as it was.  pt_trace_rays opened the geometry of an uploaded scene to the caller's rays; this opens
 * the light transport: a panorama, fisheye, orthographic or thin-lens camera, a light probe at a point, a lightmap texel, the
 * radiance arriving at a sensor in a scene that pt_scene_update_vertices moves — the caller makes the rays (csrc/pt_rays.hip).
 *
 * Rays are RAY8 records as in pt_trace_rays: org.xyz | dir.xyz | reserved (must be 0, not read) | tmax.  The direction must have
 *   unit length and is used as given.  tmax bounds the PRIMARY ray only (it takes the place of the camera path's 999999); the rays
 *   of later bounces are the integrator's own.
 * Definition: ray i takes the place of a pixel.  For each pass k = prm->first_pass .. first_pass + passes - 1 one stream runs
 *   exactly what StartRender runs for a pixel and a pass (srcs/pathtracer.cu:70-81):
 *     1. the RNG is seeded with (uint64_t)(int64_t)(int32_t)(seed_i + k * seed_stride), the sum taken in wrapping uint32 arithmetic;
 *        seed_i = d_seed[i], or i when d_seed is NULL;
 *     2. two uniform draws are made and discarded — the jitter draws: with them a ray taken from a camera pixel (direction of
 *        pt_dbg_pixel_dir, seed py * W + px, stride W * H) reproduces that pixel of pt_render bit for bit;
 *     3. spp_per_pass paths all start down the ray; the primary ray is traced once and its hit shared;
 *     4. the pass mean is pixelColor / spp_per_pass.
 *   The same ray serves every pass of a call: a caller who wants a newly jittered ray per pass calls once per pass and folds with
 *   the moments calls.  A primary ray with no hit in [0, tmax] gets what a pixel that looks past the scene gets: the ambient term
 *   for every sample, no draws, no rays.
 * pt_render_rays: d_rays8 (16-byte aligned, n_rays records), d_seed (NULL or n_rays int32), d_rgb (16-byte aligned) and d_work are
 *   DEVICE pointers on the scene's device.  d_rgb[3 * i + c] = the sum over the call's passes, in pass order starting from 0, of
 *   the per-pass means of ray i.  The buffer holds pt_rays_floats(n_rays) floats: rays are rendered in groups of 64, and the
 *   padding rays of the last group are exactly +0.
 *   Work buffer: d_work is scratch of pt_rays_work_bytes() bytes, and the contract of the moments section holds for it — after the
 *   call its start holds the per-pass means, prm->passes x pt_rays_floats(n_rays) float32, pass-major, each pass in the layout of
 *   d_rgb, valid until d_work is next written.  pt_accumulate_passes folds that slab when it is described to it by a camera of
 *   W = 8 * ceil(n_rays / 64), H = 8 pixels (as many 8x8 tiles as there are groups of 64 rays; the moments come out in ray order
 *   like d_rgb) and the prm of the call with first_pass = 0 — its seed limit then reads 64 * ceil(n / 64) * passes <= 2^31 - 1.
 *   Checked on the host before any HIP call, else PT_ERR_INVALID: a NULL scene, rays, params, rgb or work; n_rays < 1;
 *   seed_stride < 0; prm->rank != 0 || prm->world != 1; the parameter ranges of pt_render_tiles; d_rays8 or d_rgb not 16-byte
 *   aligned; ceil(n_rays / 64) x passes work units beyond pt_render_tiles' own limit, or 64 x that not below 2^31.
 *   Otherwise pt_render_tile_list's contract: BLOCKING as mode 1 is, one render, update or query at a time per scene, all GPU work
 *   on `hip_stream`, always the queue-driven pipeline (pt_set_mode(0), pt_enable_counters, pt_enable_trace_timing and the PTAMD_TSTAT
 *   diagnostics do not apply and are left as set for the next pt_render_tiles); pt_last_render_ms and pt_last_iterations report it.
 *   pt_set_shade_rounds, pt_set_drain_threshold and pt_set_early_shade act on the stream count (64 * ceil(n / 64) * passes) as on
 *   a frame's.  A ray render enqueued after pt_scene_update_vertices on the same stream sees the moved geometry.  The rays (and
 *   seeds) are read where they are for as long as the call blocks — a sample that restarts at the shared first hit reads its origin
 *   from d_rays8 —, so nothing is copied and nothing is allocated in the scene (pt_scene_device_bytes stays what it was).
 * pt_rays_floats: 192 * ceil(n_rays / 64), or -1 (n_rays < 1 or beyond 2^31).
 * pt_rays_work_bytes: pt_work_bytes of any frame that has ceil(n_rays / 64) tiles with the same prm, as pt_tile_list_work_bytes
 *   is: the pipeline's need depends on the number of work units only.  -1 for arguments pt_render_rays would reject.
 * pt_render_rays_host: the same on HOST arrays (h_seed may be NULL): uploads, renders on the NULL stream, waits and downloads
 *   h_rgb[n_rays * 3] — no padding.
 * Rays with a non-finite component or a zero direction: the result for THAT ray is unspecified, the other rays are unaffected, and
 *   the call ends, by the argument of the ray-query section (a depth-first search over a finite tree) and the path-length limits.
 * Feature buffers of a ray batch: pt_aov_rays above; with the caller's W x H grid of rays they are what pt_denoise takes.
 * Out of scope: a tile-split or multi-GPU ray render, rays x views, a per-pass ray set inside one call, non-unit directions, tmin,
 * mode 0, a CLI option.
 * -------------------------------------------------------------------------------- */
PT_API int64_t pt_rays_floats(int64_t n_rays);                                    /* 192 * ceil(n / 64), or -1 */
PT_API int64_t pt_rays_work_bytes(const PtParams* prm, int64_t n_rays);           /* or -1 */
PT_API int  pt_render_rays(PtScene* s, const float* d_rays8, const int32_t* d_seed, int64_t n_rays, int32_t seed_stride,
                           const PtParams* prm, float* d_rgb, void* d_work, void* hip_stream);
PT_API int  pt_render_rays_host(PtScene* s, const float* h_rays8, const int32_t* h_seed, int64_t n_rays, int32_t seed_stride,
                                const PtParams* prm, float* h_rgb /* n_rays * 3 */);

/* ----------------------------------------------------------------------------------
 * Adaptive sampling: every tile rendered until ITS error estimate is met (new: the reference gives every pixel the same passes).
 * Opt-in: every call above is as it was.  pt_render_converge stops the whole frame on one figure; here the moments calls meet
 * pt_render_tile_list, so the passes go where the noise is (csrc/pt_stats.hip).
 *
 * "Frame tile layout" below = the layout of pt_render_tiles with rank 0 of world 1: tile t (row-major over the full frame) owns
 *   floats 192 t .. 192 t + 191, pt_tiles_floats(cam, world 1) floats in all.  The float buffers of pt_accumulate_tile_list (d_work,
 *   d_sum, d_m2) and of pt_finish_tiles (d_sum, d_m2, d_mean, d_var) must be 16-byte aligned: their kernels move float4 only.
 *   pt_tile_errors takes 4-byte aligned moments and writes d_err 8-byte aligned; int32 buffers are 4-byte aligned.
 * pt_accumulate_tile_list: the list variant of pt_accumulate_passes.  d_work is the work buffer a pt_render_tile_list(cam, prm, list of
 *   n_tiles) left behind (prm->passes x n_tiles x 192 means, pass-major, list order); entry i is folded into tile d_list[i] of d_sum /
 *   d_m2 (frame tile layout), per float exactly the fold of pt_accumulate_passes with k = n_before + 1, ...: a tile's result is bit for
 *   bit what pt_accumulate_passes gives it after a full-frame render of the same passes.  n_before = passes every LISTED tile holds so
 *   far (0: the listed tiles are overwritten, not read); tiles not listed are not touched.  d_tile_passes (may be NULL): int32 per tile
 *   of the frame, d_tile_passes[d_list[i]] = n_before + prm->passes.
 * pt_tile_errors: one PtTileError per list entry (d_list NULL: tiles 0 .. n_tiles - 1 in order) from frame-layout moments of n_passes
 *   passes.  A pixel is used if it lies inside W x H and its S and M2 are all finite; an in-frame pixel that is not used counts as
 *   skipped.  Per used pixel, float32 as written: v_c = max(M2_c, 0) * n / (n - 1);
 *     term = sqrt((v_r + v_g) + v_b) / (((|S_r| + |S_g|) + |S_b|) + 0.03f * n)      (the mean_rel_se term of pt_error_estimate)
 *   The 64 terms of a tile (0.0 for a pixel not used), widened to float64, are summed in a fixed tree: for o = 32, 16, 8, 4, 2, 1,
 *   pixel l < o adds pixel l + o (pixel = ty * 8 + tx).  mean_rel_se = sum / pixels in float64, 0 when pixels == 0.  No atomics: two
 *   calls return the same bits.
 * pt_finish_tiles: the frame of tiles with unequal pass counts.  Per float of the frame tile layout, n = d_tile_passes[tile], IEEE
 *   float32, n converted to float once:  d_mean = S / n;  d_var = (max(M2, 0) * n) / (n - 1) (a NaN M2 stays NaN; n == 1 gives what
 *   the formula gives).  A tile with n == 0 gets +0 in both.  Either output may be NULL, not both.
 * The three calls take DEVICE pointers, are asynchronous on `hip_stream`, allocate nothing and read nothing back.  Checked before the
 *   first HIP call, else PT_ERR_INVALID: NULL pointers, a buffer short of the alignment above, n_tiles < 1 or more than the frame has, n_before < 0, n_passes < 2,
 *   prm->rank != 0 || prm->world != 1, a camera or params that pt_tiles_floats rejects, both outputs of pt_finish_tiles NULL.
 *   The ENTRIES of d_list are the caller's responsibility, as the contents of any device buffer are: each must be a tile of the frame
 *   and none may appear twice (an entry outside the frame is skipped by the fold and yields a zero record; a tile listed twice is
 *   written by two threads).
 *
 * pt_render_adaptive: host convenience like pt_render_converge (whole frame, world = 1, synchronous).  The rule, in this order:
 *   batch = prm->passes (>= 1, clamped to max_passes); min_passes is raised to 2; 2 <= min_passes <= max_passes, target >= 0 (not NaN)
 *   and the seed limit of pt_render for prm->first_pass + max_passes are required.  The active list starts as all tiles, ascending;
 *   done = 0.  Each round renders b = min(batch, max_passes - done) passes of the active list (pt_render_tile_list with first_pass =
 *   prm->first_pass + done — every active tile holds exactly `done` passes), folds them (pt_accumulate_tile_list, n_before = done),
 *   done += b; once done >= min_passes it takes pt_tile_errors of the active list for n_passes = done and drops every tile whose
 *   mean_rel_se <= target (a NaN stays active), keeping the order.  It stops when the list is empty or done == max_passes.
 *   h_accum_rgb[H*W*3] = S: every tile is bit for bit that tile of pt_render with passes = h_tile_passes[t] and the same first_pass.
 *   h_mean_rgb (may be NULL) = the pt_finish_tiles mean, the frame to show: pt_tonemap_u8(mean, n, 1) and pt_denoise(..., sample_cnt = 1,
 *   ...) take it as it is.  h_var_rgb (may be NULL) = the variance of S with each tile's own n.  h_tile_passes[tiles] (required) and
 *   h_tile_err[tiles] (may be NULL; the error at the tile's last check) are row-major over the tile grid.
 *   Deterministic: a tile's passes, seeds and fold do not depend on which other tiles are active, and the error of a tile is a fixed
 *   tree over its own pixels, so the pass map is a function of the scene, the camera and the arguments alone.
 *   A late round holds few tiles and is bound by launch latency (the pt_render_views section): the time saved trails the tile-passes
 *   saved (the adaptive section, has the measurement).
 * Out of scope: a tile-split or multi-GPU version, growing batches, dilating the active set to neighbours, adaptive views or rays,
 * mode 0 (a list is always rendered by the queue-driven pipeline).
 * -------------------------------------------------------------------------------- */
typedef struct PtTileError { double mean_rel_se; int32_t pixels, skipped; } PtTileError;   /* 16 bytes */
typedef struct PtAdaptiveReport {
    int32_t rounds;                 /* list renders done */
    int32_t tiles, tiles_converged; /* tiles of the frame; tiles that met the target (the rest stopped at max_passes) */
    int64_t tile_passes;            /* sum over tiles of their passes: the work done, in tile-passes */
    double  max_tile_err;           /* largest mean_rel_se over all tiles at their last check */
} PtAdaptiveReport;

PT_API int  pt_accumulate_tile_list(const void* d_work, const PtCamera* cam, const PtParams* prm, const int32_t* d_list, int32_t n_tiles,
                                    int32_t n_before, float* d_sum, float* d_m2, int32_t* d_tile_passes /* may be NULL */, void* hip_stream);
PT_API int  pt_tile_errors(const float* d_sum, const float* d_m2, const PtCamera* cam, const int32_t* d_list /* NULL: all */, int32_t n_tiles,
                           int32_t n_passes, PtTileError* d_err, void* hip_stream);
PT_API int  pt_finish_tiles(const float* d_sum, const float* d_m2, const int32_t* d_tile_passes, const PtCamera* cam,
                            float* d_mean, float* d_var, void* hip_stream);
PT_API int  pt_render_adaptive(PtScene* s, const PtCamera* cam, const PtParams* prm, double target, int32_t min_passes, int32_t max_passes,
                               float* h_accum_rgb, float* h_mean_rgb, float* h_var_rgb, int32_t* h_tile_passes, double* h_tile_err,
                               PtAdaptiveReport* report);

/* ----------------------------------------------------------------------------------
 * (a12,a13) Output + camera helpers (host).
 * pt_tonemap_u8 = exportImage (srcs/pathtracer.cu:94-112): /SampleCnt, ACESFilm
 *   (include/CudaUtil.cuh:383-391), ConverToUint8 (include/image.h:5-8).
 * pt_write_png  = Image::WriteTo (srcs/image.cpp:22-25), RGB8.
 * pt_camera_basis = Camera::SetRotation + GetRight (srcs/camera.cpp:32-66).
 * -------------------------------------------------------------------------------- */
PT_API int  pt_tonemap_u8(const float* raw_rgb, int64_t n_pixels, int32_t sample_cnt, uint8_t* rgb8);
PT_API int  pt_convert_u8(const float* values, int64_t n, uint8_t* out);      /* ConverToUint8, include/image.h:5-8, element-wise */
PT_API int  pt_write_png(const char* path, const uint8_t* data, int32_t W, int32_t H, int32_t channels);
PT_API void pt_camera_basis(const float rot_deg[3], float forward[3], float up[3], float right[3]);

/* ----------------------------------------------------------------------------------
 * Synthetic scenes (the reference ships none: .gitignore:365, renderer.cpp:102-115 load
 * absolute Windows paths).  Geometry exactly as SURVEY.md Appendix A.
 *   kind 0: Cornell box (12 tris)                      kind 1: + 1 stand-in mesh (69,564 tris)
 *   kind 2: + 4 instanced stand-ins (278,256 tris)
 * lat_lon: tessellation of the stand-in (187 in the configs; smaller for tests).
 * Returns the number of primitives; writes at most `cap` of them when prims != NULL.
 * -------------------------------------------------------------------------------- */
PT_API int32_t pt_scene_gen(int32_t kind, int32_t lat_lon, PtPrimitive* prims, int32_t cap);
/* Minimal Wavefront OBJ(+MTL) reader producing the Vertex data Model::processMesh would
 * (include/model.h:120-207) with BVH::AddModel's matrix bake (srcs/bvh.cpp:153-189):
 * uniform `scale` then `translate`.  Same count/cap convention as pt_scene_gen. */
PT_API int32_t pt_load_obj(const char* path, float scale, const float translate[3],
                           PtPrimitive* prims, int32_t cap);

/* ----------------------------------------------------------------------------------
 * Parity hooks: run single device functions of the integrator on the GPU so tests can
 * compare them with the oracle record by record (host pointers in and out).
 * Record layouts are those of oracle/pt_oracle.h (RAY8, HIT(29 f), BXDF in 28 f / out 12 f).
 * The HIT record's u and v (floats 2, 3) are HitResult::u / v of the reference: the triangle's vertex u, v (PtTriangle u0 .. v2)
 * under the barycentric weights of the shading frame, 0 for a sphere.  (They were 0 for every hit before scenes kept the vertex u, v
 * on the device; the same holds for the surface records of pt_trace_rays.)
 * -------------------------------------------------------------------------------- */
PT_API int  pt_dbg_raycast(PtScene* s, const float* rays8, int32_t n, float* out_hits29, int32_t* out_prim);
PT_API int  pt_dbg_bxdf(int32_t device, int32_t lobe, const float* in28, int32_t n, float* out12);
PT_API int  pt_dbg_rng(int32_t device, uint64_t seed, int32_t n, uint32_t* raw_out, float* uniform_out);
PT_API int  pt_dbg_math(int32_t device, const float* in, int32_t n, float* out8);
/* The sin / cos pair of the BxDF samplers (pathtrace-on-cuda_amd/csrc/pt_sincos.h; angles in [0, 2 pi], include/Bxdf.cuh:23-41,140-150):
 * out2 = sin cos per input, to be compared with (float)sin((double)x), (float)cos((double)x) bit for bit. */
PT_API int  pt_dbg_sincos(int32_t device, const float* in, int32_t n, float* out2);
/* The per-ray set-up of the traversal kernel (csrc/pt_trace.h: ray_setup) on n directions (3 floats each): out5 = the reference's
 * Normalize(inv(dir)) (include/CudaUtil.cuh:60-63, :70) x, y, z | the kernel's cull scale | 1.0 for a degenerate direction; the
 * test compares it with IEEE arithmetic bit for bit. */
PT_API int  pt_dbg_ray_setup(int32_t device, const float* dir3, int32_t n, float* out5);
/* StartRender's prologue + GetPixelDirection (srcs/pathtracer.cu:33-40,70-74) for n rows (px, py, pass) of int32:
 * out8 = u1 u2 | dir.xyz (after the Ray constructor's second normalisation) | the RNG's next uniform draw | 0 0. */
PT_API int  pt_dbg_pixel_dir(int32_t device, const PtCamera* cam, const int32_t* pxpypass, int32_t n, float* out8);
/* One NEE sample + its visibility (include/CudaUtil.cuh:235-245, SamplePrimitive :38-48, GetLightColor :150-166) per row.
 * in5 = surface point p.xyz | RNG seed low, high (uint32 bits); out12 = light index (int bits) | sampled point xyz | pdfLight |
 * cosA | shadow ray t_max | closest-hit primitive of the shadow ray (int bits) | GetLightColor rgb | the RNG's next draw. */
PT_API int  pt_dbg_nee(PtScene* s, const float* in5, int32_t n, float* out12);
/* Measurement aid: stream triad a = b + s*c over three float4 arrays of `bytes_per_array`
 * each, `iters` times; *gb_per_s = bytes moved (2 reads + 1 write per element) / time of the timed launches. */
PT_API int  pt_dbg_triad(int32_t device, int64_t bytes_per_array, int32_t iters, double* gb_per_s);
/* Measurement aid: the chip's vector-ALU issue rate, measured — every wave runs a long stream of independent
 * instructions of one kind out of registers (op: 0 v_fma_f32, 1 v_pk_fma_f32, 2 v_max3_f32, 3 v_cvt_f32_ubyte1,
 * 4 v_add_u32, 5 v_fma_f64, 6 v_cndmask_b32, 7 v_pk_mul_f32, 8 v_fma_mix_f32, 9 v_cvt_f32_f16, 10 v_perm_b32, 11 v_min_f32,
 * 12 v_cvt_f32_u32, 13 v_ldexp_f32, 14 v_cmp_le_f32, 15 v_bfe_u32; +16 = lanes 32..63 masked off) at `waves_per_simd`
 * waves per SIMD (1..8).  *wave_insts_per_s = wave-instructions retired per second chip-wide; *clock_ghz = shader
 * clock during the run.  This is the denominator of bench.py's VALU roofline for the traversal kernel. */
PT_API int  pt_dbg_valu_rate(int32_t device, int32_t op, int32_t waves_per_simd, int32_t iters,
                             double* wave_insts_per_s, double* clock_ghz);
/* Work counters of the last pt_render_tiles on this scene (int64 x 8):
 * [0] rays [1] node records fetched [2] triangle tests [3] sphere tests [4] rays with hit
 * [5] camera paths [6] loop trips of the wave scheduler [7] lane-trips with an active ray */
PT_API int  pt_last_counters(PtScene* s, int64_t* out8);
/* Diagnostic (environment PTAMD_TSTAT=1 only): per wf_trace launch of the last render, in 100 MHz ticks:
 * ~(earliest wave start), ~(earliest time a wave found the ray queue empty; 0 = never), latest wave exit.
 * With PTAMD_TSTAT=1 pt_last_counters returns wf_trace's trip counters instead of the work counters.
 * n_launches = 0: out3n receives 32 int64 instead — the histogram of wave lifetimes in 32-microsecond bins.
 * n_launches = -n: out3n receives n int64 — the number of rays each of the first n launches traced.
 * n_launches = -3000 / -3001 / -3002 (PTAMD_TSTAT=1): 64 int64 histogram of node steps per ray (bins of 4) / 32 int64 histogram of
 * the stack depth after a node step / 5 int64 shader clocks summed over waves per section of the loop (refill, vote, node step,
 * triangle step, ray epilogue). */
PT_API int  pt_dbg_trace_timeline(PtScene* s, int64_t* out3n, int32_t n_launches);
/* Render path: 1 = queue-driven wavefront pipeline (default: traversal and shading are
 * separate kernels, lanes refill from a ray queue), 0 = the one-kernel state machine.
 * Both produce bit-identical frames.  Environment PTAMD_MODE overrides the default.
 * pt_last_iterations: bounce iterations the pipeline launched for the last render.  The host reads the live-stream count every 16 to 64
 * iterations (with wf_drain off: every 16), so this is the first such poll at or after the iteration that retired the last stream
 * or handed the rest to wf_drain: with wf_drain off at most 15 more than the render needed. */
PT_API int  pt_set_mode(PtScene* s, int32_t mode);
/* Per-launch timing of the two pipeline kernels (mode 1): pt_enable_trace_timing makes every following render record HIP
 * events, on the launch stream, before and after each of its first max_launches wf_trace launches and after the wf_shade
 * launch that follows it (0 = off); pt_trace_timing / pt_shade_timing return the summed and maximum duration in ms of the
 * wf_trace / wf_shade launches so bracketed, and how many were timed in the last render. */
PT_API int  pt_enable_trace_timing(PtScene* s, int32_t max_launches);
PT_API int  pt_trace_timing(PtScene* s, double* sum_ms, int32_t* launches, double* max_ms);
PT_API int  pt_shade_timing(PtScene* s, double* sum_ms, int32_t* launches, double* max_ms);
PT_API int  pt_last_iterations(PtScene* s);
/* Mode 1 hands the last streams of a render to one run-to-completion launch (wf_drain) once at
 * most `live_streams` are still alive (0 = never; default 80,000: the launch, its streams spread over every SIMD,
 * replaces the last ~200 latency-bound iterations of a render — +5 % for one rank of an 8-way split, +1 % on one GPU).
 * Result-neutral. */
PT_API int  pt_set_drain_threshold(PtScene* s, int32_t live_streams);
/* Mode 1, early shade: in a render call of at most `max_streams` streams (pixels of this rank x passes of the call) the shade step of
 * every iteration starts on a second HIP stream beside the draining traversal kernel (streams whose rays are all back are shaded at
 * once, the others — and all list appends — follow when the traversal has finished); renders of fewer than max_streams / 8 streams are
 * left alone too (launch-latency bound); 0 = never, default 2,500,000: on for one rank of
 * an 8-way tile split of 1080p x 8 passes (-6.5 % time), off for a full frame (whose launches are large next to the traversal's
 * ~0.3 ms launch tail).  Result-neutral: every stream goes through the same step (pathtrace-on-cuda_amd/csrc/pt_wavefront.hip:
 * wf_shade PHASE 1 / 2).  Environment PTAMD_EARLY overrides the default. */
PT_API int  pt_set_early_shade(PtScene* s, int32_t max_streams);
/* Mode 1, shading schedule: 1 = a stream whose path ends starts its next sample in the same step (bounces - 1 steps per sample,
 * two bounce evaluations per step), 0 = one bounce evaluation per step (bounces steps per sample, a shorter step), -1 = 0 while
 * more than 4 M streams are alive, 1 below.  Default: -1 for scenes whose surface table fits in L2 (<= 2 MB: +10 % on
 * the Cornell room), 1 otherwise (with the bunny one bounce per step is neutral on a full frame and costs 6 % for one rank of an
 * 8-way split).  Result-neutral: a stream goes through the same operations in the same order either way
 * (pathtrace-on-cuda_amd/csrc/pt_stream.h: shade_step_t). */
PT_API int  pt_set_shade_rounds(PtScene* s, int32_t mode);
/* Run the counting build of the kernel on the next pt_render_tiles calls (slower; mode 0). */
PT_API int  pt_enable_counters(PtScene* s, int32_t on);

#ifdef __cplusplus
}
#endif
#endif /* PT_API_H */
