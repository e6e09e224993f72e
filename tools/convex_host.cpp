// convex_host.cpp — convex_tri_key, convex_sphere_key and convex_overlaps of csrc/pt_convex.h compiled for the host, so that the numpy
// restatement of tests/convex_ref.py can be held against the kernels' own arithmetic bit for bit without a GPU
// (tests/test_convex_queries.py).  The three functions are plain inline C++ once PT_DEV is defined away; the test copies their text out
// of the header into convex_kernel_fns.inc and compiles this file with the library's numerics flags next to it:
//   g++ -std=c++17 -O2 -ffp-contract=off -fno-fast-math -I <dir of convex_kernel_fns.inc> tools/convex_host.cpp -o convex_host
//   convex_host <in> <out>
// in:  int32 m, n_tri, n_sph, n_box | n_tri pairs of 4 m + 9 floats: m planes n.xyz d, a.xyz ab.xyz ac.xyz | n_sph pairs of 4 m + 4 floats:
//      m planes, c.xyz rad | n_box pairs of 4 m + 6 floats: m planes, lo.xyz hi.xyz of a node's box
// out: n_tri + n_sph + n_box floats: the class key of every pair; for a box pair 1 if convex_overlaps holds, else 0
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#define PT_DEV static inline
struct f3 { float x, y, z; };
struct float4 { float x, y, z, w; };
#include "convex_kernel_fns.inc"

int main(int argc, char** argv)
{
    if (argc < 3) { fprintf(stderr, "usage: convex_host <in> <out>\n"); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 1;
    int32_t head[4];
    if (fread(head, 4, 4, f) != 4 || head[0] < 1 || head[0] > 8 || head[1] < 0 || head[2] < 0 || head[3] < 0) return 1;
    const int m = head[0];
    const size_t nt = (size_t)head[1], ns = (size_t)head[2], nb = (size_t)head[3], wt = 4 * m + 9, ws = 4 * m + 4, wb = 4 * m + 6;
    std::vector<float> tri(nt * wt), sph(ns * ws), box(nb * wb), out(nt + ns + nb);
    if (fread(tri.data(), 4, tri.size(), f) != tri.size() || fread(sph.data(), 4, sph.size(), f) != sph.size() ||
        fread(box.data(), 4, box.size(), f) != box.size())
        return 1;
    fclose(f);
    float4 pl[8];
    for (size_t i = 0; i < nt; i++) {
        const float* p = &tri[i * wt];
        memcpy(pl, p, 16 * m);
        p += 4 * m;
        out[i] = convex_tri_key(pl, m, f3{p[0], p[1], p[2]}, f3{p[3], p[4], p[5]}, f3{p[6], p[7], p[8]});
    }
    for (size_t i = 0; i < ns; i++) {
        const float* p = &sph[i * ws];
        memcpy(pl, p, 16 * m);
        p += 4 * m;
        out[nt + i] = convex_sphere_key(pl, m, float4{p[0], p[1], p[2], p[3]});
    }
    for (size_t i = 0; i < nb; i++) {
        const float* p = &box[i * wb];
        memcpy(pl, p, 16 * m);
        p += 4 * m;
        out[nt + ns + i] = convex_overlaps(f3{p[0], p[1], p[2]}, f3{p[3], p[4], p[5]}, pl, m) ? 1.f : 0.f;
    }
    f = fopen(argv[2], "wb");
    if (!f) return 1;
    const bool ok = fwrite(out.data(), 4, out.size(), f) == out.size();
    return fclose(f) == 0 && ok ? 0 : 1;
}
