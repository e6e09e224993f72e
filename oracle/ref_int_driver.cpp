// TEST INFRASTRUCTURE ONLY (oracle/): driver for oracle/_ref/ptref_int, a build of the reference's INTEGRATOR.
//
// What it is: a small command-line program, written for this repository, that includes the reference's own unmodified
// headers where they lie in the reference tree (REF of oracle/Makefile)
//   include/CudaUtil.cuh   (intersectionAABB, RayCast, SamplePrimitive, GetLightColor, GetColor_iter, ACESFilm)
//   include/Bxdf.cuh       (the four lobes: eval_*, sample_*, sample_*_pdf, and everything below them)
//   include/CudaPrimitive.cuh, CudaVector.cuh, CudaRay.cuh (Triangle::Copy/hit, Sphere::hit, vec3)
// and calls them as host C++.  <cuda_runtime.h> and <device_launch_parameters.h> are the REAL headers bundled with this
// image's triton wheel.  <curand_kernel.h> is oracle/curand_shim.h (this repository's RNG contract; see that file) and
// <curand.h> is empty; oracle/Makefile puts both into oracle/_ref/fwd/ for the build.  -DNDEBUG as in the reference's
// Release configuration (PathTrace_GPGPU.vcxproj:142), so the asserts of GetColor_iter are compiled out.
//
// What is restated here, because srcs/pathtracer.cu itself cannot be compiled (<<<>>> launches, managed memory): the
// ten-line pixel loop of StartRender (srcs/pathtracer.cu:76-81), the light list (:164-174), and the one line of
// GetColor_iter that divides SamplePrimitive's pdf by the light count (include/CudaUtil.cuh:235-237) for `nee`.  The
// reference's compile-time MAX_BOUNCE 8, RUSSIAN_ROULETTE_BOUNCE 3 and PROB_STOP_BOUNCE 0.5 apply to `paths`.
//
// libm switch (first argument): `glibc` = the float functions of this machine's libm, `contract` = correctly rounded
// float results through double, (float)f((double)x) — the two modes of o_set_libm (oracle/pt_oracle.h).  The reference is
// not touched for this: the program is compiled with -fno-builtin and defines the seven functions of
// oracle/pt_oracle.cpp:51-57 (sinf cosf tanf atanf atan2f powf expf) itself; each either goes through double or calls the
// libm function found with dlsym(RTLD_NEXT).  Transcendentals the reference's headers reach: sinf, cosf, atanf
// (Bxdf.cuh:30-31,145-148), powf (Bxdf.cuh:86 as powf; :264,:313 as pow(float, 2.0f), which <math.h> resolves to the float
// overload and the compiler may turn into a multiplication: x * x is the correctly rounded square in either mode), expf
// (Bxdf.cuh:103, the non-GGX branch, never taken).  tanf / atan2f are used by srcs/pathtracer.cu only, which is not part
// of this program; they are defined all the same.  sqrtf / fabsf are exact in IEEE arithmetic and stay libm's.
//
// Record layouts are those of oracle/pt_oracle.h (TRI 88 f, SPH 16 f, RAY8, HIT 29 f, NODE 40 B), so outputs compare
// byte for byte with the oracle's.  Output goes where the caller says; the binary itself lives in oracle/_ref/ (git-ignored).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <cstdint>
#include <string>
#include <vector>

#include <dlfcn.h>

#include "CudaUtil.cuh"         // reference header: pulls CudaVector / CudaRay / CudaPrimitive / Bxdf

// ---------------------------------------------------------------------------------
// libm switch
// ---------------------------------------------------------------------------------
static int g_contract = 1;
template <class F> static F next_sym(const char* name)
{
    void* p = dlsym(RTLD_NEXT, name);
    if (!p) { fprintf(stderr, "ptref_int: libm has no %s\n", name); exit(2); }
    return (F)p;
}
typedef float (*f1_t)(float);
typedef float (*f2_t)(float, float);
#define LIBM1(name, dname) \
    extern "C" float name(float x) noexcept { \
        if (g_contract) return (float)dname((double)x); \
        static f1_t f = next_sym<f1_t>(#name); return f(x); }
#define LIBM2(name, dname) \
    extern "C" float name(float x, float y) noexcept { \
        if (g_contract) return (float)dname((double)x, (double)y); \
        static f2_t f = next_sym<f2_t>(#name); return f(x, y); }
LIBM1(sinf, sin)
LIBM1(cosf, cos)
LIBM1(tanf, tan)
LIBM1(atanf, atan)
LIBM1(expf, exp)
LIBM2(atan2f, atan2)
LIBM2(powf, pow)

// ---------------------------------------------------------------------------------
// files and records
// ---------------------------------------------------------------------------------
static std::vector<unsigned char> slurp(const char* path)
{
    FILE* f = fopen(path, "rb");
    if (!f) { fprintf(stderr, "ptref_int: cannot open %s\n", path); exit(2); }
    fseek(f, 0, SEEK_END); long n = ftell(f); fseek(f, 0, SEEK_SET);
    std::vector<unsigned char> b((size_t)n);
    if (n && fread(b.data(), 1, (size_t)n, f) != (size_t)n) { fprintf(stderr, "ptref_int: short read %s\n", path); exit(2); }
    fclose(f);
    return b;
}
static void spit(const char* path, const void* p, size_t n)
{
    FILE* f = fopen(path, "wb");
    if (!f) { fprintf(stderr, "ptref_int: cannot write %s\n", path); exit(2); }
    if (n && fwrite(p, 1, n, f) != n) { fprintf(stderr, "ptref_int: short write %s\n", path); exit(2); }
    fclose(f);
}
static vec3 get3(const float* f) { return vec3(f[0], f[1], f[2]); }
static void put3(std::vector<float>& o, const vec3& v) { o.push_back(v[0]); o.push_back(v[1]); o.push_back(v[2]); }
static Material getm(const float* f)
{
    Material m; m.emittance = get3(f); m.albedo = get3(f + 3); m.specular = get3(f + 6);
    m.opacity = f[9]; m.roughness = f[10]; m.metallic = f[11]; return m;
}
static void putm(std::vector<float>& o, const Material& m)
{
    put3(o, m.emittance); put3(o, m.albedo); put3(o, m.specular);
    o.push_back(m.opacity); o.push_back(m.roughness); o.push_back(m.metallic);
}
static const int TRI_FLOATS = 88, HIT_FLOATS = 29;
static void put_hit(std::vector<float>& o, bool hit, const HitResult& h)
{
    if (!hit) { for (int i = 0; i < HIT_FLOATS; i++) o.push_back(0.f); return; }
    o.push_back(1.f); o.push_back(h.t); o.push_back(h.u); o.push_back(h.v); o.push_back(h.bFrontFace ? 1.f : 0.f);
    put3(o, h.p); put3(o, h.normal); put3(o, h.tangent); put3(o, h.bitangent);
    putm(o, h.mat);
}
static uint32_t u32(const float* f) { uint32_t u; memcpy(&u, f, 4); return u; }

// The world as PathTracer::Render uploads it (srcs/pathtracer.cu:142-187): triangles through Triangle::Copy, the light list, spheres, nodes.
struct World {
    std::vector<CudaBVHNode> nodes;
    std::vector<Triangle> tris, lights;
    std::vector<Sphere> spheres;
    int Nl = 0;
};
static void load_world(World& w, const char* nodes_path, const char* tris_path, const char* sph_path)
{
    auto nb = slurp(nodes_path), tb = slurp(tris_path), sb = slurp(sph_path);
    static_assert(sizeof(CudaBVHNode) == 40, "NODE record is the reference's CudaBVHNode");
    w.nodes.resize(nb.size() / sizeof(CudaBVHNode));
    memcpy((void*)w.nodes.data(), nb.data(), w.nodes.size() * sizeof(CudaBVHNode));
    const size_t n = tb.size() / (TRI_FLOATS * 4);
    w.tris.resize(n); w.lights.resize(n);
    for (size_t i = 0; i < n; i++) {
        const float* f = (const float*)tb.data() + i * TRI_FLOATS;
        // TRI record: V0 V1 V2 | T0 T1 T2 | B0 B1 B2 | N0 N1 N2 | normal E1 E2 (recomputed by Copy) | u0 v0 u1 v1 u2 v2 | mat0 mat1 mat2 | area
        Triangle src;
        src.Copy(get3(f), get3(f + 3), get3(f + 6), get3(f + 9), get3(f + 12), get3(f + 15), get3(f + 18), get3(f + 21), get3(f + 24),
                 get3(f + 27), get3(f + 30), get3(f + 33), getm(f + 51), getm(f + 63), getm(f + 75),
                 f[45], f[47], f[49], f[46], f[48], f[50]);
        w.tris[i].Copy(src);                                                     // srcs/pathtracer.cu:166
        if (src.mat0.emittance.length() > EPS || src.mat1.emittance.length() > EPS || src.mat2.emittance.length() > EPS)
            w.lights[w.Nl++].Copy(src);                                          // :167-173
    }
    const size_t ns = sb.size() / (16 * 4);
    w.spheres.resize(ns);
    for (size_t i = 0; i < ns; i++) {
        const float* f = (const float*)sb.data() + i * 16;
        w.spheres[i].Copy(Sphere(f[0], f[1], f[2], f[3], getm(f + 4)));          // :177-180
    }
}

// ---------------------------------------------------------------------------------
// rng SEED N : N lines "raw uniform-bits" of curand / curand_uniform after curand_init(SEED, 0, 0)
static int cmd_rng(int argc, char** argv)
{
    if (argc != 4) return 1;
    const unsigned long long seed = strtoull(argv[2], nullptr, 10);
    const int n = atoi(argv[3]);
    curandState a, b;
    curand_init(seed, 0, 0, &a); curand_init(seed, 0, 0, &b);
    for (int i = 0; i < n; i++) {
        const unsigned int raw = curand(&a);
        const float u = curand_uniform(&b);
        printf("%u %u\n", raw, u32(&u));
    }
    return (a.draws == n && b.draws == n) ? 0 : 3;
}

// bxdf LOBE in28 out12 : the arguments and columns of o_bxdf (oracle/pt_oracle.h)
static int cmd_bxdf(int argc, char** argv)
{
    if (argc != 5) return 1;
    const int lobe = atoi(argv[2]);
    auto ib = slurp(argv[3]);
    const size_t n = ib.size() / (28 * 4);
    std::vector<float> out; out.reserve(n * 12);
    for (size_t r = 0; r < n; r++) {
        const float* f = (const float*)ib.data() + r * 28;
        HitResult h; memset((void*)&h, 0, sizeof(h));
        h.normal = get3(f); h.tangent = get3(f + 3); h.bitangent = get3(f + 6); h.bFrontFace = f[9] != 0.f;
        const vec3 albedo = get3(f + 10), specular = get3(f + 13);
        const float roughness = f[16], metallic = f[17];
        const vec3 wo = get3(f + 18), wi = get3(f + 21);
        curandState s;
        curand_init(((unsigned long long)u32(f + 25) << 32) | u32(f + 24), 0, 0, &s);
        const vec3 ior = reflectivity_to_eta(specular);                          // CudaUtil.cuh:231
        vec3 e, ws, es; float p, ps;
        switch (lobe) {
        case 0:
            e = eval_gltfpbr(albedo, specular, roughness, metallic, h, wo, wi);
            p = sample_gltfpbr_pdf(albedo, specular, roughness, metallic, h, wo, wi);
            ws = sample_gltfpbr(albedo, specular, roughness, metallic, h, wo, &s);
            es = eval_gltfpbr(albedo, specular, roughness, metallic, h, wo, ws);
            ps = sample_gltfpbr_pdf(albedo, specular, roughness, metallic, h, wo, ws);
            break;
        case 1:
            e = eval_reflective(albedo, specular, roughness, metallic, h, wo, wi);
            p = sample_reflective_pdf(albedo, h.normal, wo, wi);
            ws = sample_reflective(albedo, h.normal, wo);
            es = eval_reflective(albedo, specular, roughness, metallic, h, wo, ws);
            ps = sample_reflective_pdf(albedo, h.normal, wo, ws);
            break;
        case 2:
            e = eval_refractive(albedo, ior[0], roughness, h, wo, wi);
            p = sample_refractive_pdf(albedo, ior[0], roughness, h, wo, wi);
            ws = sample_refractive(albedo, ior[0], roughness, h, wo, &s);
            es = eval_refractive(albedo, ior[0], roughness, h, wo, ws);
            ps = sample_refractive_pdf(albedo, ior[0], roughness, h, wo, ws);
            break;
        default:
            e = eval_pure_refractive(albedo, ior[0], h, wo, wi);
            p = sample_pure_refractive_pdf(albedo, ior[0], h, wo, wi);
            ws = sample_pure_refractive(albedo, ior[0], h, wo, &s);
            es = eval_pure_refractive(albedo, ior[0], h, wo, ws);
            ps = sample_pure_refractive_pdf(albedo, ior[0], h, wo, ws);
            break;
        }
        put3(out, e); out.push_back(p); put3(out, ws); put3(out, es); out.push_back(ps); out.push_back((float)s.draws);
    }
    spit(argv[4], out.data(), out.size() * 4);
    return 0;
}

// raycast nodes tris88 sph16 rays8 hits29 : the reference's RayCast per RAY8 row (direction used as given)
static int cmd_raycast(int argc, char** argv)
{
    if (argc != 7) return 1;
    World w; load_world(w, argv[2], argv[3], argv[4]);
    auto rb = slurp(argv[5]);
    const size_t R = rb.size() / (8 * 4);
    std::vector<float> out; out.reserve(R * HIT_FLOATS);
    for (size_t r = 0; r < R; r++) {
        const float* f = (const float*)rb.data() + r * 8;
        Ray ray; ray.org = get3(f); ray.dir = get3(f + 3);
        HitResult h; memset((void*)&h, 0, sizeof(h));
        const bool hit = RayCast(ray, w.tris.data(), (int)w.tris.size(), w.nodes.data(), (int)w.nodes.size(),
                                 w.spheres.data(), (int)w.spheres.size(), h, f[6], f[7]);
        put_hit(out, hit, h);
    }
    spit(argv[6], out.data(), out.size() * 4);
    return 0;
}

// nee nodes tris88 sph16 in5 out12 : per row of o_nee's in5 (point, seed lo, seed hi) one `curand(s) % Nl`, SamplePrimitive and
// GetLightColor (CudaUtil.cuh:235-239).  Columns written are those these functions return — 0 light index (int32 bits), 1-3 point,
// 4 pdf, 8-10 light colour, 11 the next uniform draw; 5-7 (cosA, tmax, the shadow ray's primitive: the oracle's own) stay 0.
static int cmd_nee(int argc, char** argv)
{
    if (argc != 7) return 1;
    World w; load_world(w, argv[2], argv[3], argv[4]);
    if (w.Nl == 0) { fprintf(stderr, "ptref_int: no light\n"); return 2; }
    auto ib = slurp(argv[5]);
    const size_t n = ib.size() / (5 * 4);
    std::vector<float> out(n * 12, 0.f);
    const int Nl = w.Nl;
    Triangle* lights = w.lights.data();
    for (size_t i = 0; i < n; i++) {
        const float* f = (const float*)ib.data() + i * 5;
        const vec3 p = get3(f);
        curandState st; curandState* s = &st;
        curand_init(((unsigned long long)u32(f + 4) << 32) | u32(f + 3), 0, 0, s);
        int lightIdx = curand(s) % Nl;
        vec3 SampledPoint;
        float pdfLight = SamplePrimitive(s, SampledPoint, lights[lightIdx]) / ((float)Nl);
        Color lightColor = GetLightColor(p, SampledPoint, w.tris.data(), (int)w.tris.size(), w.nodes.data(), (int)w.nodes.size(),
                                         w.spheres.data(), (int)w.spheres.size());
        float* o = out.data() + i * 12;
        memcpy(o, &lightIdx, 4);
        o[1] = SampledPoint[0]; o[2] = SampledPoint[1]; o[3] = SampledPoint[2]; o[4] = pdfLight;
        o[8] = lightColor[0]; o[9] = lightColor[1]; o[10] = lightColor[2]; o[11] = curand_uniform(s);
    }
    spit(argv[6], out.data(), out.size() * 4);
    return 0;
}

// paths nodes tris88 sph16 rows out : one row = one pixel of one pass, 10 x 4 bytes: camera position (3 f), direction (3 f), seed low and
// high word, draws to skip (what GetPixelDirection consumed), spp (uint32 each).  out = 3 f per row: pixelColor / (float)spp, summed in
// float32 in path order (srcs/pathtracer.cu:76-81).
static int cmd_paths(int argc, char** argv)
{
    if (argc != 7) return 1;
    World w; load_world(w, argv[2], argv[3], argv[4]);
    if (w.Nl == 0) { fprintf(stderr, "ptref_int: no light\n"); return 2; }
    auto ib = slurp(argv[5]);
    const size_t n = ib.size() / (10 * 4);
    std::vector<float> out(n * 3);
    for (size_t r = 0; r < n; r++) {
        const float* f = (const float*)ib.data() + r * 10;
        const vec3 CameraPos = get3(f), direction = get3(f + 3);
        curandState s;
        curand_init(((unsigned long long)u32(f + 7) << 32) | u32(f + 6), 0, 0, &s);
        for (uint32_t k = 0; k < u32(f + 8); k++) curand(&s);
        const int spp = (int)u32(f + 9);
        Color pixelColor(0.f, 0.f, 0.f);
        for (int i = 0; i < spp; i++)
        {
            pixelColor += GetColor_iter(Ray(CameraPos, direction), w.tris.data(), (int)w.tris.size(), w.nodes.data(), (int)w.nodes.size(),
                                        w.lights.data(), w.Nl, w.spheres.data(), (int)w.spheres.size(), &s);
        }
        const Color c = pixelColor / (float)(spp);
        out[3 * r] = c[0]; out[3 * r + 1] = c[1]; out[3 * r + 2] = c[2];
    }
    spit(argv[6], out.data(), out.size() * 4);
    return 0;
}

// aces in out : 3 f per row through ACESFilm (CudaUtil.cuh:383-391)
static int cmd_aces(int argc, char** argv)
{
    if (argc != 4) return 1;
    auto ib = slurp(argv[2]);
    const size_t n = ib.size() / 12;
    std::vector<float> out(n * 3);
    for (size_t i = 0; i < n; i++) {
        const Color c = ACESFilm(get3((const float*)ib.data() + 3 * i));
        out[3 * i] = c[0]; out[3 * i + 1] = c[1]; out[3 * i + 2] = c[2];
    }
    spit(argv[3], out.data(), out.size() * 4);
    return 0;
}

int main(int argc, char** argv)
{
    int rc = 1;
    if (argc >= 3 && (!strcmp(argv[1], "glibc") || !strcmp(argv[1], "contract"))) {
        g_contract = !strcmp(argv[1], "contract");
        argc--; argv++;
        std::string c = argv[1];
        if (c == "rng") rc = cmd_rng(argc, argv);
        else if (c == "bxdf") rc = cmd_bxdf(argc, argv);
        else if (c == "raycast") rc = cmd_raycast(argc, argv);
        else if (c == "nee") rc = cmd_nee(argc, argv);
        else if (c == "paths") rc = cmd_paths(argc, argv);
        else if (c == "aces") rc = cmd_aces(argc, argv);
    }
    if (rc == 1) fprintf(stderr, "usage: ptref_int glibc|contract rng|bxdf|raycast|nee|paths|aces ...\n");
    return rc;
}
