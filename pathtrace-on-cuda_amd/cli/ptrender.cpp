// ptrender — headless command line for the path tracer (the reference has no CLI: its window size
// is a compile-time constant and rendering starts on key P, srcs/main.cpp:15-16, srcs/renderer.cpp:283-293).
// Uses only the reference-shaped host surface (host/ref_surface.h).
#include <unistd.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <string>
#include <vector>
#include "../host/ref_surface.h"

static void usage()
{
    std::cout <<
        "usage: ptrender [--scene cornell|standin|standin4] [--obj FILE --obj-scale S --obj-translate X,Y,Z]\n"
        "                [--glass-sphere] [--width W] [--height H] [--passes N] [--spp N] [--depth N]\n"
        "                [--lat-lon N] [--device D] [--no-progressive] [--raw FILE] [--denoise FILE.png] [--aov FILE]\n"
        "                [--target-error E [--max-passes N] [--variance FILE]] [--window X0,Y0,X1,Y1]\n"
        "                [--adaptive E [--min-passes M] [--max-passes N] [--pass-map FILE] [--variance FILE]]\n"
        "                [--cam-pos X,Y,Z] [--cam-rot RX,RY,RZ] [--fov DEG] [--views FILE]\n"
        "                [--world N --rank R --id-file PATH [--job-tag T]]   (one process per GPU; rank 0 writes the frame;\n"
        "                 T = a number the ranks of this job share and other jobs do not, default: the parent process id)\n"
        "Writes temp.png (per pass) and result.png in the current directory, like PathTracer::Render.\n"
        "--raw FILE: also writes the float accumulation buffer (W*H*3 float32) there after every pass (viewer hook).\n"
        "--denoise FILE.png: also writes the frame denoised with the first-hit feature buffers (rank 0, after the final frame).\n"
        "--aov FILE: also writes those feature buffers (W*H*8 float32: albedo.rgb normal.xyz depth coverage) there.\n"
        "--target-error E: renders batches of --passes passes until the frame's estimated relative RMS error is <= E or --max-passes\n"
        "  (default 8 batches) are in, prints the passes used and the estimates; --variance FILE: the per-pixel variance of the frame\n"
        "  (W*H*3 float32).  Single process only; result.png and --denoise use the passes actually rendered.\n"
        "--window X0,Y0,X1,Y1: renders only the half-open pixel window [X0, X1) x [Y0, Y1) of the frame (the 8x8 tiles that overlap it);\n"
        "  temp.png, result.png and --raw are the window, pixel for pixel the crop of the full frame's.  Single process, and not with\n"
        "  --denoise, --aov or --target-error.\n"
        "--adaptive E: renders every 8x8 tile in batches of --passes passes until the tile's own error estimate (the mean over its pixels of\n"
        "  the relative standard error) is <= E, checked once --min-passes (default 2) are in, or --max-passes (default 8 batches) are in;\n"
        "  prints the rounds and the tile-passes used.  result.png and --denoise show the mean frame (every tile divided by its own passes);\n"
        "  --raw FILE: the sums, --variance FILE: their per-pixel variance (W*H*3 float32 each), --pass-map FILE: the passes of every tile\n"
        "  (tiles_y x tiles_x int32).  Single process, and not with --target-error, --window or --views.\n"
        "--cam-pos X,Y,Z, --cam-rot RX,RY,RZ (degrees, as Camera::SetRotation), --fov DEG (vertical): the camera; defaults 0,20,60 /\n"
        "  0,90,0 / 45, the reference application's.\n"
        "--views FILE: renders a batch of cameras in one pipeline run.  Each line of FILE is `px py pz rx ry rz fov [first_pass]`\n"
        "  (# starts a comment); writes result_000.png, result_001.png, ... (and with --raw FILE the float frames FILE_000, ...), each\n"
        "  what a run with that line's --cam-pos / --cam-rot / --fov writes as result.png.  Single process, and not with --window,\n"
        "  --target-error, --denoise or --aov.\n"
        "Defaults: scene cornell, 1920x1080, 8 passes x 64 spp, depth 8.\n";
}

// --views FILE: one camera per line, `px py pz rx ry rz fov [first_pass]`; false (with a message that names the line) for a malformed one
static bool read_views(const std::string& path, std::vector<Camera>& cams, std::vector<int>& first, int defaultFirst)
{
    FILE* f = fopen(path.c_str(), "r");
    if (!f) { std::cerr << "--views: cannot read " << path << "\n"; return false; }
    char line[1024];
    bool ok = true;
    for (int no = 1; ok && fgets(line, sizeof line, f); no++) {
        if (char* h = strchr(line, '#')) *h = 0;
        if (strspn(line, " \t\r\n") == strlen(line)) continue;
        float v[7]; int fp = defaultFirst, used = 0;
        const int n = sscanf(line, "%f %f %f %f %f %f %f %n%d %n", &v[0], &v[1], &v[2], &v[3], &v[4], &v[5], &v[6], &used, &fp, &used);
        if (n < 7 || line[used] != 0 || !(v[6] > 0.f && v[6] < 180.f) || fp < 0) {
            std::cerr << "--views " << path << ": line " << no << " is not `px py pz rx ry rz fov [first_pass]` (0 < fov < 180, first_pass >= 0)\n";
            ok = false;
            break;
        }
        Camera c(vec3f(v[0], v[1], v[2]));
        c.SetRotation(vec3f(v[3], v[4], v[5]));
        c.fovy = v[6];
        cams.push_back(c); first.push_back(fp);
    }
    fclose(f);
    if (ok && cams.empty()) { std::cerr << "--views " << path << ": no camera in it\n"; ok = false; }
    return ok;
}

int main(int argc, char** argv)
{
    std::string scene = "cornell", obj, rawPath, denoisePath, aovPath, variancePath;
    double targetError = 0.0; int maxPasses = 0;
    bool adaptive = false; double adaptiveTarget = 0.0; int minPasses = 0; std::string passMapPath;
    float objScale = 1.f; float objT[3] = {0, 0, 0};
    int W = 1920, H = 1080, passes = 8, spp = 64, depth = 8, latlon = 187, device = 0;
    bool glass = false, progressive = true;
    int win[4] = {0, 0, 0, 0}; bool windowed = false;
    float camPos[3] = {0.f, 20.f, 60.f}, camRot[3] = {0.f, 90.f, 0.f}, fov = 45.f; std::string viewsPath;      // the reference app's camera (srcs/renderer.cpp:28-30)
    int rank = 0, world = 1; std::string idFile; unsigned long long jobTag = (unsigned long long)getppid();
    for (int i = 1; i < argc; i++) {
        const std::string a = argv[i];
        auto next = [&]() -> const char* { if (i + 1 >= argc) { usage(); exit(2); } return argv[++i]; };
        if (a == "--scene") scene = next();
        else if (a == "--obj") obj = next();
        else if (a == "--obj-scale") objScale = (float)atof(next());
        else if (a == "--obj-translate") { if (sscanf(next(), "%f,%f,%f", &objT[0], &objT[1], &objT[2]) != 3) { usage(); return 2; } }
        else if (a == "--glass-sphere") glass = true;
        else if (a == "--width") W = atoi(next());
        else if (a == "--height") H = atoi(next());
        else if (a == "--passes") passes = atoi(next());
        else if (a == "--spp") spp = atoi(next());
        else if (a == "--depth") depth = atoi(next());
        else if (a == "--lat-lon") latlon = atoi(next());
        else if (a == "--device") device = atoi(next());
        else if (a == "--no-progressive") progressive = false;
        else if (a == "--raw") rawPath = next();
        else if (a == "--denoise") denoisePath = next();
        else if (a == "--aov") aovPath = next();
        else if (a == "--target-error") targetError = atof(next());
        else if (a == "--max-passes") maxPasses = atoi(next());
        else if (a == "--adaptive") { adaptive = true; adaptiveTarget = atof(next()); }
        else if (a == "--min-passes") minPasses = atoi(next());
        else if (a == "--pass-map") passMapPath = next();
        else if (a == "--variance") variancePath = next();
        else if (a == "--window") { if (sscanf(next(), "%d,%d,%d,%d", &win[0], &win[1], &win[2], &win[3]) != 4) { usage(); return 2; } windowed = true; }
        else if (a == "--cam-pos") { if (sscanf(next(), "%f,%f,%f", &camPos[0], &camPos[1], &camPos[2]) != 3) { usage(); return 2; } }
        else if (a == "--cam-rot") { if (sscanf(next(), "%f,%f,%f", &camRot[0], &camRot[1], &camRot[2]) != 3) { usage(); return 2; } }
        else if (a == "--fov") fov = (float)atof(next());
        else if (a == "--views") viewsPath = next();
        else if (a == "--world") world = atoi(next());
        else if (a == "--rank") rank = atoi(next());
        else if (a == "--id-file") idFile = next();
        else if (a == "--job-tag") jobTag = strtoull(next(), nullptr, 10);
        else if (a == "--help" || a == "-h") { usage(); return 0; }
        else { std::cerr << "unknown option " << a << "\n"; usage(); return 2; }
    }
    if (world < 1 || rank < 0 || rank >= world || (world > 1 && idFile.empty())) { std::cerr << "--world N needs 0 <= --rank < N and --id-file PATH\n"; return 2; }
    if (adaptive && (world > 1 || targetError > 0.0 || windowed || !viewsPath.empty())) { std::cerr << "--adaptive is single-process and does not go with --target-error, --window or --views\n"; return 2; }
    if (adaptive && (!(adaptiveTarget >= 0.0) || minPasses < 0 || (maxPasses != 0 && (maxPasses < 2 || maxPasses < minPasses)))) { std::cerr << "--adaptive E needs E >= 0 and 2 <= --min-passes <= --max-passes\n"; return 2; }
    if (!adaptive && (minPasses != 0 || !passMapPath.empty())) { std::cerr << "--min-passes and --pass-map need --adaptive E\n"; return 2; }
    if (!adaptive && (maxPasses != 0 || !variancePath.empty()) && !(targetError > 0.0)) { std::cerr << "--max-passes and --variance need --target-error E > 0\n"; return 2; }
    if (targetError > 0.0 && (world > 1 || (maxPasses != 0 && maxPasses < 2))) { std::cerr << "--target-error is single-process and needs --max-passes >= 2\n"; return 2; }
    if (windowed && (world > 1 || !denoisePath.empty() || !aovPath.empty() || targetError > 0.0)) { std::cerr << "--window is single-process and does not go with --denoise, --aov or --target-error\n"; return 2; }
    if (windowed && (win[0] < 0 || win[1] < 0 || win[2] > W || win[3] > H || win[0] >= win[2] || win[1] >= win[3])) { std::cerr << "--window X0,Y0,X1,Y1 needs 0 <= X0 < X1 <= width and 0 <= Y0 < Y1 <= height\n"; return 2; }
    if (!(fov > 0.f && fov < 180.f)) { std::cerr << "--fov DEG needs 0 < DEG < 180\n"; return 2; }
    if (!viewsPath.empty() && (windowed || world > 1 || targetError > 0.0 || !denoisePath.empty() || !aovPath.empty())) { std::cerr << "--views is single-process and does not go with --window, --target-error, --denoise or --aov\n"; return 2; }
    std::vector<Camera> viewCams; std::vector<int> viewFirst;
    if (!viewsPath.empty() && !read_views(viewsPath, viewCams, viewFirst, 0)) return 2;
    const int kind = scene == "cornell" ? 0 : scene == "standin" ? 1 : scene == "standin4" ? 2 : -1;
    if (kind < 0) { std::cerr << "unknown scene " << scene << "\n"; return 2; }

    // the reference app's setup unless told otherwise: camera at (0,20,60), rotation (0,90,0), fovy 45, aspect W/H (srcs/renderer.cpp:28-30,47-53)
    Camera camera(vec3f(camPos[0], camPos[1], camPos[2]));
    camera.SetRotation(vec3f(camRot[0], camRot[1], camRot[2]));
    camera.fovy = fov;
    camera.Screen_W = (unsigned)W; camera.Screen_H = (unsigned)H; camera.aspect = (float)W / (float)H;

    SAHBVH bvh;
    const int n = pt_scene_gen(kind, latlon, nullptr, 0);
    if (n < 0) { std::cerr << pt_last_error() << "\n"; return 2; }
    bvh.primitives.resize((size_t)n);
    pt_scene_gen(kind, latlon, bvh.primitives.data(), n);
    if (!obj.empty() && !bvh.AddOBJ(obj, objScale, vec3f(objT[0], objT[1], objT[2]))) return 2;
    if (glass) {   // BASELINE.json configs[3]: glass sphere r=6 at (10,6,8), opacity 0, roughness 0
        Material m; memset(&m, 0, sizeof(m));
        m.albedo[0] = m.albedo[1] = m.albedo[2] = 1.f; m.specular[0] = m.specular[1] = m.specular[2] = 0.04f;
        CudaSpheres.push_back(Sphere(10.f, 6.f, 8.f, 6.f, m));
    }
    std::cout << "Build BVH" << std::endl;
    bvh.GenBVHTree();
    std::cout << "Pre process done : Primitive CNT = " << bvh.primCnt() << std::endl;

    PathTracer tracer;
    tracer.params.passes = passes; tracer.params.spp_per_pass = spp; tracer.params.max_bounce = depth;
    tracer.device = device; tracer.progressive = progressive; tracer.raw_path = rawPath;
    tracer.denoise_path = denoisePath; tracer.aov_path = aovPath;
    tracer.target_error = targetError; tracer.max_passes = maxPasses; tracer.variance_path = variancePath;
    tracer.adaptive = adaptive; tracer.adaptive_target = adaptiveTarget; tracer.min_passes = minPasses; tracer.pass_map_path = passMapPath;
    if (windowed) { tracer.window_x0 = win[0]; tracer.window_y0 = win[1]; tracer.window_x1 = win[2]; tracer.window_y1 = win[3]; }
    tracer.view_cameras = viewCams; tracer.view_first_pass = viewFirst;
    tracer.rank = rank; tracer.world = world; tracer.id_file = idFile; tracer.job_tag = jobTag;
    tracer.Render(camera, &bvh);
    if (adaptive) {               // kernel_ms below would be the last round only
        std::cout << "{\"tile_passes_done\": " << tracer.tile_passes_done << "}" << std::endl;
        return 0;
    }
    if (targetError > 0.0) {      // kernel_ms below would be the last batch only
        std::cout << "{\"passes_done\": " << tracer.passes_done << "}" << std::endl;
        return 0;
    }
    const double samples = (windowed ? (double)(win[2] - win[0]) * (win[3] - win[1]) : (double)W * H) * passes * spp * (viewCams.empty() ? 1.0 : (double)viewCams.size());
    std::cout << "{\"msamples_per_s_kernel\": " << samples / (tracer.last_render_ms * 1e-3) / 1e6 << ", \"kernel_ms\": " << tracer.last_render_ms << "}" << std::endl;
    return 0;
}
