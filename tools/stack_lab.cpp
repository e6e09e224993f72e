// stack_lab.cpp — host-only, a sibling of tree_lab.cpp: how full does a ray's traversal stack get on the caller's triangles?
// Reads triangle positions (n x 9 float32: V0 V1 V2) and rays (m x 8 float32 RAY8: org.xyz dir.xyz 0 tmax) from two binary files,
// runs pt_bvh_build_sah and pt_build_accel exactly as the upload does (PTAMD_TREE is honoured as there) and walks every ray through
// the quantised 4-wide tree one ray at a time: children nearest first, far side cut at the closest hit, up to three pushes per node.
// Counted per ray: node steps and the deepest stack; over all rays: the node steps taken with at least kLds entries on the stack
// (wf_trace keeps 16 entries per lane in LDS, csrc/pt_wavefront.hip: kWfLdsStack; the rest goes to global memory).
// child_box, the slab test and the triangle test are tree_lab.cpp's: they APPROXIMATE the kernel's arithmetic (no conservative
// widening of the boxes, no reference leaf box, no parked leaves), so the figures are those of the tree, not of the kernel to the step.
//   g++ -std=c++17 -O2 -I include tools/stack_lab.cpp pathtrace-on-cuda_amd/build/{accel_build,bvh_build,scenes,pt_host,obj_loader}.o -pthread -o /tmp/stack_lab
//   /tmp/stack_lab positions.bin rays.bin
// The last line is machine-readable:
//   "STACK tris <n> rays <m> bdepth <b> depth <d> over_lds <share of rays whose deepest stack > 16> over_budget <share of rays with > 256
//    node steps> n_over_budget <their number> max_stack <k> max_steps <s> deep_share <share of node steps taken at stack depth >= 16>"
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../include/pt_api.h"
#include "../pathtrace-on-cuda_amd/host/accel_build.h"

struct V { float x, y, z; };
static V operator-(V a, V b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
static float dot(V a, V b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
static V cross(V a, V b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }

static constexpr int kLds = 16, kBudget = 256, kStack = 256;
struct Ray { V o, d; float tmax; };
struct Walk { long steps = 0, deepSteps = 0; int maxStack = 0; };

static bool tri_hit(const PtAccel& A, int q, const Ray& r, float& best)
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

static Walk walk(const PtAccel& A, const Ray& r)
{
    Walk w;
    const float o[3] = {r.o.x, r.o.y, r.o.z}, iv[3] = {1.f / r.d.x, 1.f / r.d.y, 1.f / r.d.z};
    float best = r.tmax;
    int stack[kStack]; int sp = 0; int cur = 0;
    for (;;) {
        if (cur >= 0) {
            const uint32_t* d = &A.quad[(size_t)cur * 16];
            float tn[4]; bool hit[4];
            for (int k = 0; k < 4; k++) {
                hit[k] = false; tn[k] = 1e30f;
                if ((int32_t)d[4 + k] == ~0) continue;
                float lo[3], hi[3]; child_box(d, k, lo, hi);
                float t0 = 0.f, t1 = best;
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
            bool done = false;
            if (nh == 0) { if (sp == 0) done = true; else cur = stack[--sp]; }
            else {
                for (int k = nh - 1; k >= 1; k--) { if (sp >= kStack) { fprintf(stderr, "stack_lab: stack of %d entries is full\n", kStack); exit(2); } stack[sp++] = (int32_t)d[4 + order[k]]; }
                w.maxStack = std::max(w.maxStack, sp);
                cur = (int32_t)d[4 + order[0]];
            }
            // the stack depth after this node step: what wf_trace's diagnostic build puts into its histogram
            w.steps++;
            if (sp >= kLds) w.deepSteps++;
            if (done) break;
        } else {
            const int code = ~cur, first = code >> 3, cnt = code & 7;
            for (int k = 0; k < cnt; k++) tri_hit(A, first + k, r, best);
            if (sp == 0) break;
            cur = stack[--sp];
        }
    }
    return w;
}

static std::vector<float> read_floats(const char* path, int per)
{
    FILE* f = fopen(path, "rb");
    if (!f) { fprintf(stderr, "stack_lab: cannot open %s\n", path); exit(2); }
    fseek(f, 0, SEEK_END); const long bytes = ftell(f); fseek(f, 0, SEEK_SET);
    if (bytes <= 0 || bytes % (4 * per)) { fprintf(stderr, "stack_lab: %s is not rows of %d float32\n", path, per); exit(2); }
    std::vector<float> v((size_t)bytes / 4);
    if (fread(v.data(), 4, v.size(), f) != v.size()) { fprintf(stderr, "stack_lab: short read of %s\n", path); exit(2); }
    fclose(f);
    return v;
}

int main(int argc, char** argv)
{
    if (argc < 3) { fprintf(stderr, "usage: stack_lab positions.bin rays.bin\n"); return 2; }
    const std::vector<float> pos = read_floats(argv[1], 9), rr = read_floats(argv[2], 8);
    const int n = (int)(pos.size() / 9), m = (int)(rr.size() / 8);
    // positions only: the tree depends on nothing else (flat unit frames and a grey material fill the records)
    std::vector<PtPrimitive> prims((size_t)n);
    memset(prims.data(), 0, prims.size() * sizeof(PtPrimitive));
    for (int i = 0; i < n; i++) {
        PtVertex* vs[3] = {&prims[i].v1, &prims[i].v2, &prims[i].v3};
        for (int k = 0; k < 3; k++) {
            const float* p = &pos[(size_t)i * 9 + 3 * k];
            vs[k]->Position = {p[0], p[1], p[2]};
            vs[k]->Normal = {0.f, 1.f, 0.f}; vs[k]->Tangent = {1.f, 0.f, 0.f}; vs[k]->Bitangent = {0.f, 0.f, 1.f};
        }
    }
    PtFlatBVH* bvh = nullptr;
    if (pt_bvh_build_sah(prims.data(), n, &bvh)) { printf("bvh build failed\n"); return 1; }
    PtAccel acc;
    pt_build_accel(pt_bvh_nodes(bvh), pt_bvh_num_nodes(bvh), pt_bvh_tris(bvh), pt_bvh_num_tris(bvh), acc);

    long steps = 0, deep = 0, maxSteps = 0, overLds = 0, overBudget = 0;
    int maxStack = 0;
    for (int i = 0; i < m; i++) {
        const float* q = &rr[(size_t)i * 8];
        const Walk w = walk(acc, Ray{{q[0], q[1], q[2]}, {q[3], q[4], q[5]}, q[7]});
        steps += w.steps; deep += w.deepSteps;
        maxSteps = std::max(maxSteps, w.steps); maxStack = std::max(maxStack, w.maxStack);
        overLds += w.maxStack > kLds; overBudget += w.steps > kBudget;
    }
    printf("%d triangles, %d quad nodes, %d rays, %.1f node steps per ray\n", pt_bvh_num_tris(bvh), acc.n_quad, m, (double)steps / std::max(1, m));
    printf("STACK tris %d rays %d bdepth %d depth %d over_lds %.4f over_budget %.4f n_over_budget %ld max_stack %d max_steps %ld deep_share %.5f\n",
           pt_bvh_num_tris(bvh), m, acc.depth, acc.quad_depth, (double)overLds / std::max(1, m), (double)overBudget / std::max(1, m), overBudget, maxStack, maxSteps,
           steps ? (double)deep / (double)steps : 0.0);
    pt_bvh_free(bvh);
    return 0;
}
