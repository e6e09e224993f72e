// tree_lab.cpp — host-only: the traversal tree the upload builds (host/accel_build.cpp), the size-aware one (default) against
// the centroid-SAH one (PTAMD_TREE=0), on one ray set.  Builds a config scene, both quantised 4-wide trees exactly as the upload
// does, shoots camera rays, two generations of cosine-weighted bounce rays and a shadow ray towards the light from every hit
// (traced on the old tree, so both trees see the same rays) and walks every ray through each tree one ray at a time with the
// kernel's slab test on the dequantised boxes (far side cut at the closest hit, children nearest first), counting node steps
// and leaf visits.  Weighted cost per ray = node steps + 3.1 x leaf visits (a pair-record test costs about three node trips,
// DESIGN 5.3).  Ray classes: path / shadow rays whose segment misses or crosses the "core box" (the box of the triangles
// smaller than 1/8 of the scene diagonal: the mesh).
//   g++ -std=c++17 -O2 -I include tools/tree_lab.cpp pathtrace-on-cuda_amd/build/{accel_build,bvh_build,scenes,pt_host,obj_loader}.o -pthread -o /tmp/tree_lab
//   /tmp/tree_lab [kind=1] [lat_lon=187] [pixels=60000]
// The last line per tree is machine-readable: "TREE <0|1> kind <k> nodes <n> children <c> depth <d> bdepth <b> steps <s> leaves <l> weighted <w>".
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>
#include "../include/pt_api.h"
#include "../pathtrace-on-cuda_amd/host/accel_build.h"

struct V { float x, y, z; };
static V operator+(V a, V b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
static V operator-(V a, V b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
static V operator*(V a, float s) { return {a.x * s, a.y * s, a.z * s}; }
static float dot(V a, V b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
static V cross(V a, V b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
static V norm(V a) { return a * (1.f / std::sqrt(dot(a, a))); }

static constexpr double kLeafTrip = 3.1;
struct Ray { V o, d; float tmax; bool any; };
struct Cnt { double nodes = 0, leaves = 0, rays = 0; };

static bool tri_hit(const PtAccel& A, int q, const Ray& r, float& best, V* nrm)
{
    const float* t = &A.tri[(size_t)q * 12];
    const V v0{t[0], t[1], t[2]}, e1{t[4], t[5], t[6]}, e2{t[8], t[9], t[10]};
    const V T = r.o - v0, P = cross(r.d, e2), Q = cross(T, e1);
    const float det = dot(P, e1);
    if (det < 1e-4f) return false;
    const float inv = 1.f / det, tt = dot(Q, e2) * inv;
    if (tt < 0.f || tt > best) return false;
    const float u = dot(P, T), v = dot(Q, r.d);
    if (u < 0.f || u > det || v < 0.f || u + v > det) return false;
    best = tt;
    if (nrm) *nrm = norm(cross(e1, e2));
    return true;
}

static void child_box(const uint32_t* d, int k, float* lo, float* hi)
{
    float org[3]; memcpy(org, d, 12);
    for (int a = 0; a < 3; a++) {
        float sc; memcpy(&sc, &d[a == 0 ? 3 : 13 + a], 4);
        lo[a] = org[a] + sc * (float)((d[8 + a] >> (8 * k)) & 0xff);
        hi[a] = org[a] + sc * (float)((d[11 + a] >> (8 * k)) & 0xff);
    }
}

// returns the primitive hit or -1; counts into c
static int trace(const PtAccel& A, const Ray& r, Cnt& c, float& tHit, V* nrm)
{
    const V inv{1.f / r.d.x, 1.f / r.d.y, 1.f / r.d.z};
    float best = r.tmax; int prim = -1;
    int stack[256]; int sp = 0; int cur = 0;
    c.rays++;
    for (;;) {
        if (cur >= 0) {
            c.nodes++;
            const uint32_t* d = &A.quad[(size_t)cur * 16];
            float tn[4]; bool hit[4];
            for (int k = 0; k < 4; k++) {
                hit[k] = false; tn[k] = 1e30f;
                if ((int32_t)d[4 + k] == ~0) continue;
                float lo[3], hi[3]; child_box(d, k, lo, hi);
                float t0 = 0.f, t1 = best;
                const float o[3] = {r.o.x, r.o.y, r.o.z}, iv[3] = {inv.x, inv.y, inv.z};
                for (int a = 0; a < 3; a++) {
                    float a0 = (lo[a] - o[a]) * iv[a], a1 = (hi[a] - o[a]) * iv[a];
                    if (a0 > a1) std::swap(a0, a1);
                    t0 = std::max(t0, a0); t1 = std::min(t1, a1);
                }
                if (t0 <= t1 * 1.00001f + 1e-6f) { hit[k] = true; tn[k] = t0; }
            }
            int idx[4] = {0, 1, 2, 3}, order[4], nh = 0;
            std::stable_sort(idx, idx + 4, [&](int a, int b) { return tn[a] < tn[b]; });
            for (int k = 0; k < 4; k++) if (hit[idx[k]]) order[nh++] = idx[k];
            if (nh == 0) { if (sp == 0) break; cur = stack[--sp]; continue; }
            for (int k = nh - 1; k >= 1; k--) stack[sp++] = (int32_t)d[4 + order[k]];
            cur = (int32_t)d[4 + order[0]];
        } else {
            c.leaves++;
            const int code = ~cur, first = code >> 3, cnt = code & 7;
            bool stop = false;
            for (int k = 0; k < cnt; k++)
                if (tri_hit(A, first + k, r, best, nrm)) { int p; memcpy(&p, &A.tri[(size_t)(first + k) * 12 + 3], 4); prim = p; if (r.any) stop = true; }
            if (stop || sp == 0) break;
            cur = stack[--sp];
        }
    }
    tHit = best;
    return prim;
}

static void build(int tree, PtFlatBVH* bvh, PtAccel& acc, double& ms)
{
    setenv("PTAMD_TREE", tree ? "1" : "0", 1);
    const auto t0 = std::chrono::steady_clock::now();
    pt_build_accel(pt_bvh_nodes(bvh), pt_bvh_num_nodes(bvh), pt_bvh_tris(bvh), pt_bvh_num_tris(bvh), acc);
    ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    unsetenv("PTAMD_TREE");
}

int main(int argc, char** argv)
{
    const int kind = argc > 1 ? atoi(argv[1]) : 1, ll = argc > 2 ? atoi(argv[2]) : 187, npix = argc > 3 ? atoi(argv[3]) : 60000;
    const int n = pt_scene_gen(kind, ll, nullptr, 0);
    std::vector<PtPrimitive> prims((size_t)n);
    pt_scene_gen(kind, ll, prims.data(), n);
    PtFlatBVH* bvh = nullptr;
    if (pt_bvh_build_sah(prims.data(), n, &bvh)) { printf("bvh build failed\n"); return 1; }
    PtAccel acc[2]; double ms[2];
    build(0, bvh, acc[0], ms[0]);
    build(1, bvh, acc[1], ms[1]);
    printf("scene kind %d lat_lon %d: %d triangles\n", kind, ll, pt_bvh_num_tris(bvh));

    // the ray set, traced on the old tree
    std::mt19937 rng(12345);
    std::uniform_real_distribution<float> U(0.f, 1.f);
    std::vector<Ray> rays, gen;
    const V cam{0.f, 20.f, 60.f};
    const float th = std::tan(0.5f * 45.f * 3.14159265f / 180.f), aspect = 16.f / 9.f;
    for (int i = 0; i < npix; i++) {
        const float sx = (2.f * U(rng) - 1.f) * th * aspect, sy = (2.f * U(rng) - 1.f) * th;
        gen.push_back({cam, norm(V{sx, sy, -1.f}), 1e30f, false});
    }
    for (int g = 0; g < 3; g++) {
        std::vector<Ray> next;
        for (const Ray& r : gen) {
            rays.push_back(r);
            Cnt dummy; float t; V nrm{0, 1, 0};
            if (trace(acc[0], r, dummy, t, &nrm) < 0) continue;
            const V p = r.o + r.d * t;
            if (dot(nrm, r.d) > 0.f) nrm = nrm * -1.f;
            const V lp{-5.f + 10.f * U(rng), 39.98f, -5.f + 10.f * U(rng)};
            const V tl = lp - p; const float dl = std::sqrt(dot(tl, tl));
            if (dl > 1e-3f) rays.push_back({p + nrm * 1e-3f, tl * (1.f / dl), dl - 2e-3f, true});
            const float u1 = U(rng), u2 = U(rng), rr = std::sqrt(u1), ph = 6.2831853f * u2;
            V tng = std::fabs(nrm.x) > 0.5f ? V{0, 1, 0} : V{1, 0, 0};
            const V bt = norm(cross(nrm, tng)); tng = cross(bt, nrm);
            const V d = norm(tng * (rr * std::cos(ph)) + bt * (rr * std::sin(ph)) + nrm * std::sqrt(1.f - u1));
            next.push_back({p + nrm * 1e-3f, d, 1e30f, false});
        }
        gen.swap(next);
    }
    printf("%zu rays (camera, 2 bounce generations, shadow)\n", rays.size());

    // ray classes by the core box
    const PtTriangle* T = pt_bvh_tris(bvh);
    const int nT = pt_bvh_num_tris(bvh);
    float smn[3] = {1e30f, 1e30f, 1e30f}, smx[3] = {-1e30f, -1e30f, -1e30f};
    for (int i = 0; i < nT; i++) for (int a = 0; a < 3; a++) for (float x : {T[i].V0[a], T[i].V1[a], T[i].V2[a]}) { smn[a] = std::min(smn[a], x); smx[a] = std::max(smx[a], x); }
    float sd2 = 0.f;
    for (int a = 0; a < 3; a++) sd2 += (smx[a] - smn[a]) * (smx[a] - smn[a]);
    float cmn[3] = {1e30f, 1e30f, 1e30f}, cmx[3] = {-1e30f, -1e30f, -1e30f};
    for (int i = 0; i < nT; i++) {
        float mn[3], mx[3], d2 = 0.f;
        for (int a = 0; a < 3; a++) { mn[a] = std::min(T[i].V0[a], std::min(T[i].V1[a], T[i].V2[a])); mx[a] = std::max(T[i].V0[a], std::max(T[i].V1[a], T[i].V2[a])); d2 += (mx[a] - mn[a]) * (mx[a] - mn[a]); }
        if (d2 * 64.f < sd2) for (int a = 0; a < 3; a++) { cmn[a] = std::min(cmn[a], mn[a]); cmx[a] = std::max(cmx[a], mx[a]); }
    }
    std::vector<int> cls(rays.size());
    for (size_t i = 0; i < rays.size(); i++) {
        const Ray& r = rays[i];
        float t0 = 0.f, t1 = r.tmax;
        const float o[3] = {r.o.x, r.o.y, r.o.z}, d[3] = {r.d.x, r.d.y, r.d.z};
        for (int a = 0; a < 3; a++) { const float iv = 1.f / d[a]; float a0 = (cmn[a] - o[a]) * iv, a1 = (cmx[a] - o[a]) * iv; if (a0 > a1) std::swap(a0, a1); t0 = std::fmax(t0, a0); t1 = std::fmin(t1, a1); }
        cls[i] = (r.any ? 2 : 0) + (t0 <= t1 ? 1 : 0);
    }
    static const char* cname[4] = {"path, missing the core box", "path, through the core box", "shadow, missing the core box", "shadow, through the core box"};

    double w[2] = {0, 0};
    for (int tree = 0; tree < 2; tree++) {
        const PtAccel& A = acc[tree];
        double kids = 0;
        for (int q = 0; q < A.n_quad; q++) for (int k = 0; k < 4; k++) kids += (int32_t)A.quad[(size_t)q * 16 + 4 + k] != ~0;
        printf("\n%s tree (PTAMD_TREE=%d): %d quad nodes, %.2f children per node, quad depth %d, binary depth %d, built in %.0f ms\n",
               tree ? "size-aware" : "centroid-SAH", tree, A.n_quad, kids / A.n_quad, A.quad_depth, A.depth, ms[tree]);
        Cnt all, per[4];
        for (size_t i = 0; i < rays.size(); i++) {
            Cnt c; float t; trace(A, rays[i], c, t, nullptr);
            all.nodes += c.nodes; all.leaves += c.leaves; all.rays++;
            per[cls[i]].nodes += c.nodes; per[cls[i]].leaves += c.leaves; per[cls[i]].rays++;
        }
        for (int k = 0; k < 4; k++)
            printf("  %-30s %7.0f rays: node steps/ray %6.3f  leaf visits/ray %6.3f  trips/ray %6.2f  weighted %6.2f\n", cname[k], per[k].rays,
                   per[k].nodes / std::max(1.0, per[k].rays), per[k].leaves / std::max(1.0, per[k].rays), (per[k].nodes + per[k].leaves) / std::max(1.0, per[k].rays),
                   (per[k].nodes + kLeafTrip * per[k].leaves) / std::max(1.0, per[k].rays));
        w[tree] = (all.nodes + kLeafTrip * all.leaves) / all.rays;
        printf("  %-30s %7.0f rays: node steps/ray %6.3f  leaf visits/ray %6.3f  trips/ray %6.2f  weighted %6.2f\n", "all", all.rays,
               all.nodes / all.rays, all.leaves / all.rays, (all.nodes + all.leaves) / all.rays, w[tree]);
        printf("TREE %d kind %d nodes %d children %.3f depth %d bdepth %d steps %.4f leaves %.4f weighted %.4f\n", tree, kind, A.n_quad, kids / A.n_quad,
               A.quad_depth, A.depth, all.nodes / all.rays, all.leaves / all.rays, w[tree]);
    }
    printf("\nweighted cost per ray, size-aware / centroid-SAH: %.3f\n", w[1] / w[0]);
    pt_bvh_free(bvh);
    return 0;
}
