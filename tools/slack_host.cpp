// slack_host.cpp — quad_order and box_test of csrc/pt_trace.h compiled for the host, so that the numpy models of tests/slack_ref.py can be
// held against the kernels' own arithmetic bit for bit without a GPU (tests/test_slack.py).  The two functions are plain inline C++ once
// PT_DEV is defined away and the bit casts are supplied; the test copies their text out of the header into slack_kernel_fns.inc, with
// quad_order's slack constant replaced by PT_TEST_KSL, and compiles this file with -ffp-contract=off next to it:
//   g++ -std=c++17 -O2 -ffp-contract=off -I <dir of slack_kernel_fns.inc> -DPT_TEST_KSL=9.5367431640625e-7f tools/slack_host.cpp -o slack_host
//   slack_host <in> <out>
// in:  int32 n_quad, n_nodes, n_queries | quad records (16 dwords) | binary records (16 floats) |
//      per query 9 dwords: quad node, binary node, org.xyz, inv.xyz, cull
// out: per query 12 dwords: k0 k1 k2 k3 r0 r1 r2 r3 of quad_order (cullT = cull) | okL tnL okR tnR of box_test on the two children (cullB = cull)
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#define PT_DEV static inline
struct f3 { float x, y, z; };
struct uint4 { uint32_t x, y, z, w; };
static inline float __uint_as_float(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }
static inline int __float_as_int(float f) { int i; memcpy(&i, &f, 4); return i; }
constexpr int kQuadMiss = 0x7fffffff;
#include "slack_kernel_fns.inc"

int main(int argc, char** argv)
{
    if (argc < 3) { fprintf(stderr, "usage: slack_host <in> <out>\n"); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 1;
    int32_t head[3];
    if (fread(head, 4, 3, f) != 3 || head[0] < 1 || head[1] < 1 || head[2] < 0) return 1;
    std::vector<uint32_t> quad((size_t)head[0] * 16), query((size_t)head[2] * 9), out((size_t)head[2] * 12);
    std::vector<float> nodes((size_t)head[1] * 16);
    if (fread(quad.data(), 4, quad.size(), f) != quad.size() || fread(nodes.data(), 4, nodes.size(), f) != nodes.size() ||
        fread(query.data(), 4, query.size(), f) != query.size()) return 1;
    fclose(f);
    for (int i = 0; i < head[2]; i++) {
        const uint32_t* q = &query[(size_t)i * 9];
        if (q[0] >= (uint32_t)head[0] || q[1] >= (uint32_t)head[1]) return 1;
        float v[7];
        memcpy(v, q + 2, 28);
        const f3 org{v[0], v[1], v[2]}, inv{v[3], v[4], v[5]};
        const uint32_t* n = &quad[(size_t)q[0] * 16];
        const uint4 n0{n[0], n[1], n[2], n[3]}, n1{n[4], n[5], n[6], n[7]}, n2{n[8], n[9], n[10], n[11]}, n3{n[12], n[13], n[14], n[15]};
        int k[4], r[4];
        quad_order(n0, n1, n2, n3, org, inv, v[6], k[0], k[1], k[2], k[3], r[0], r[1], r[2], r[3]);
        uint32_t* o = &out[(size_t)i * 12];
        memcpy(o, k, 16);
        memcpy(o + 4, r, 16);
        const float* b = &nodes[(size_t)q[1] * 16];
        float tnL, tnR;
        o[8] = box_test(b[0], b[1], b[2], b[3], b[4], b[5], org, inv, v[6], tnL) ? 1u : 0u;
        o[10] = box_test(b[6], b[7], b[8], b[9], b[10], b[11], org, inv, v[6], tnR) ? 1u : 0u;
        memcpy(o + 9, &tnL, 4);
        memcpy(o + 11, &tnR, 4);
    }
    f = fopen(argv[2], "wb");
    if (!f) return 1;
    const bool ok = fwrite(out.data(), 4, out.size(), f) == out.size();
    return fclose(f) == 0 && ok ? 0 : 1;
}
