// ref_surface.h — the reference's C++ host surface, re-declared on top of the C-ABI.
//
// For users of WaterPlease/PathTrace-on-CUDA who have no viewer to drop the library behind:
// the same class names, public members and call sequence as include/camera.h, include/bvh.h
// (SAH path), include/CudaPrimitive.cuh (host-visible parts), include/image.h and
// include/pathtracer.cuh, with glm::vec3 replaced by a plain 3-float struct and all GL members
// removed.  Everything forwards to include/pt_api.h; nothing here computes radiance.
#pragma once
#include <string>
#include <vector>
#include "../../include/pt_api.h"

struct vec3f { float x, y, z; vec3f() : x(0), y(0), z(0) {} vec3f(float a, float b, float c) : x(a), y(b), z(c) {} };

// include/camera.h:9-40
class Camera {
public:
    Camera();                               // fovy 45, aspect 16/9, rotation (0,90,0), pos 0 (srcs/camera.cpp:7-15)
    explicit Camera(vec3f _pos);
    vec3f pos;
    unsigned int Screen_W = 1920, Screen_H = 1080;
    float fovy, aspect, near, far;
    const vec3f GetForward() { return forward; }
    const vec3f GetUp() { return up; }
    const vec3f GetRight() { return right; }
    const Camera& AddRotation(vec3f deltaRotation);
    const Camera& SetRotation(vec3f _rotation);   // (roll, pitch, yaw) in degrees (srcs/camera.cpp:42-66)
private:
    vec3f rotation, forward, up, right;
};

// include/mesh.h:11-37, include/bvh.h:8-13 — byte-identical to the C-ABI mirrors
typedef PtMaterialOnCPU MaterialOnCPU;
typedef PtVertex Vertex;
typedef PtPrimitive Primitive;

// include/CudaPrimitive.cuh:15-23, 237-247, 249-323 (data members)
typedef PtMaterial Material;
typedef PtBVHNode CudaBVHNode;
typedef PtTriangle Triangle;
struct Sphere : PtSphere {
    Sphere() { memset_zero(); }
    Sphere(float x, float y, float z, float r, Material m) { center[0] = x; center[1] = y; center[2] = z; rad = r; mat = m; }
private:
    void memset_zero();
};

// include/bvh.h:39-77,123-131 (SAH path; GL members dropped)
class BVH {
public:
    std::vector<Primitive> primitives;
    virtual ~BVH();
    virtual void GenBVHTree();              // build + flatten (the reference keeps a pointer tree in rootBVH; here the flat arrays)
    void AddPrimitives(const Primitive* p, size_t n) { primitives.insert(primitives.end(), p, p + n); }
    bool AddOBJ(const std::string& path, float scale, vec3f translation);   // Model + BVH::AddModel (srcs/bvh.cpp:153-189)
    unsigned int primCnt() const { return (unsigned int)primitives.size(); }
    PtFlatBVH* flat = nullptr;
};
class SAHBVH : public BVH {};

// include/CudaPrimitive.cuh:325-337
extern std::vector<CudaBVHNode> CudaBVH;
extern std::vector<Triangle> CudaPrims;
extern std::vector<Sphere> CudaSpheres;
void LoadFromBVH(BVH* bvh);

// include/image.h
typedef unsigned char Pixel;
inline unsigned char ConverToUint8(float value) { return (unsigned char)(value * 255.99f); }
class Image {
public:
    Image(int W, int H, int C);
    ~Image();
    bool WriteTo(const char* path);
    unsigned char* GetData() noexcept { return data; }
    int GetWidth() noexcept { return width; }
    int GetHeight() noexcept { return height; }
    int GetNrChannels() noexcept { return nrChannels; }
private:
    unsigned char* data = nullptr;
    int width, height, nrChannels;
};

// include/pathtracer.cuh + the compile-time tunables of include/CudaUtil.cuh:15-19 as members
class PathTracer {
public:
    PtParams params;                        // defaults = the reference's #defines
    int device = 0;
    bool progressive = true;                // rewrite temp.png after every pass (srcs/pathtracer.cu:245)
    PathTracer() { pt_params_default(&params); pt_denoise_params_default(&denoise_params); }
    void Render(Camera& camera, BVH* bvh);  // writes temp.png / result.png in the CWD; GPU error -> message + exit(99)
    double last_render_ms = 0.0;            // kernel time of the last Render (sum over passes)
    // Viewer hook (new; the reference's viewer only sees temp.png, srcs/renderer.cpp:283-293): when non-empty, the float accumulation
    // buffer (W*H*3 float32, row-major, sum of per-pass means so far) is written to this path after every pass and at the end,
    // atomically (temporary name + rename) — point it at /dev/shm and a viewer can map the frame while the render goes on.
    std::string raw_path;
    // Tile split over several processes, one per GPU (new; the reference is single-device): this process renders tiles
    // t % world == rank; the ranks meet through `id_file` (pt_comm_create_from_file_tagged: `job_tag` is any value the ranks of one
    // job share and other jobs do not) and rank 0 assembles and exports the frame.  If any rank fails, every rank exits 99.
    int rank = 0, world = 1;
    std::string id_file;
    unsigned long long job_tag = 0;
    // Feature buffers and denoiser (new; include/pt_api.h: pt_render_aov, pt_denoise), rank 0 only, after the final frame: when
    // non-empty, the first-hit AOVs of the call's passes are taken and `denoise_path` receives the denoised frame, tone-mapped
    // like result.png; `aov_path` receives the raw AOV buffer (W*H*8 float32, row-major).  Empty: nothing changes.
    std::string denoise_path, aov_path;
    PtDenoiseParams denoise_params;
    // Render to a target (new; include/pt_api.h: pt_render_converge), single process only: when target_error > 0 the frame is
    // rendered in batches of params.passes passes until the estimated relative RMS error is <= target_error or max_passes
    // (0 = 8 batches) are in; one line reports the passes used and both estimates, `variance_path` (when non-empty) receives
    // the per-pixel variance of the frame (W*H*3 float32, row-major), and result.png / the denoiser use passes_done.
    double target_error = 0.0;
    int max_passes = 0;
    std::string variance_path;
    int passes_done = 0;                    // passes in the frame of the last Render
    // Adaptive sampling (new; include/pt_api.h: pt_render_adaptive), single process only and without a target_error, a window or views:
    // when `adaptive` is set every 8x8 tile is rendered in batches of params.passes passes until ITS error estimate is <= adaptive_target
    // (checked once min_passes are in) or max_passes (0 = 8 batches) are in.  result.png and the denoiser show the mean frame (each
    // tile divided by its own passes); raw_path receives the sums, variance_path the per-pixel variance of them (W*H*3 float32 each) and
    // pass_map_path the passes of every tile (tiles_y x tiles_x int32, row-major); one line reports the rounds and the work done.
    bool adaptive = false;
    double adaptive_target = 0.0;
    int min_passes = 0;
    std::string pass_map_path;
    long long tile_passes_done = 0;         // tile-passes rendered by the last adaptive Render
    // Render region (new; include/pt_api.h: pt_render_window), single process only and without the denoiser, the AOVs or a target:
    // when window_x1 > window_x0 only the half-open pixel window is rendered (the 8x8 tiles that overlap it, not the frame) and
    // temp.png, result.png and raw_path hold the window — the pixels are those of the full frame's render, bit for bit.
    int window_x0 = 0, window_y0 = 0, window_x1 = 0, window_y1 = 0;
    // A batch of views (new; include/pt_api.h: pt_render_views), single process only and without a window, a target, the denoiser or
    // the AOVs: when non-empty, Render renders these cameras (pos, rotation and fovy of each; screen size and aspect are those of
    // the camera Render is given) in ONE pipeline run and writes result_000.png, result_001.png, ... (and raw_path + "_000", ...)
    // instead of result.png — each bit for bit what a Render of that camera alone writes.  view_first_pass: one first pass per
    // view, or empty for params.first_pass.
    std::vector<Camera> view_cameras;
    std::vector<int> view_first_pass;
};
