// box_host.cpp — box_tri_key and box_sphere_key of csrc/pt_box.h compiled for the host, so that the numpy restatement of tests/box_ref.py
// can be held against the kernels' own arithmetic bit for bit without a GPU (tests/test_box_queries.py).  The two functions are plain
// inline C++ once PT_DEV is defined away; the test copies their text out of the header into box_kernel_fns.inc and compiles this file
// with the library's numerics flags next to it:
//   g++ -std=c++17 -O2 -ffp-contract=off -fno-fast-math -I <dir of box_kernel_fns.inc> tools/box_host.cpp -o box_host
//   box_host <in> <out>
// in:  int32 n_tri, n_sph | n_tri pairs of 15 floats: lo.xyz hi.xyz a.xyz ab.xyz ac.xyz | n_sph pairs of 10 floats: lo.xyz hi.xyz c.xyz rad
// out: n_tri + n_sph floats: the class key of every pair
#include <cstdint>
#include <cstdio>
#include <vector>

#define PT_DEV static inline
struct f3 { float x, y, z; };
struct float4 { float x, y, z, w; };
#include "box_kernel_fns.inc"

int main(int argc, char** argv)
{
    if (argc < 3) { fprintf(stderr, "usage: box_host <in> <out>\n"); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 1;
    int32_t head[2];
    if (fread(head, 4, 2, f) != 2 || head[0] < 0 || head[1] < 0) return 1;
    std::vector<float> tri((size_t)head[0] * 15), sph((size_t)head[1] * 10), out((size_t)head[0] + (size_t)head[1]);
    if (fread(tri.data(), 4, tri.size(), f) != tri.size() || fread(sph.data(), 4, sph.size(), f) != sph.size()) return 1;
    fclose(f);
    for (size_t i = 0; i < (size_t)head[0]; i++) {
        const float* p = &tri[i * 15];
        out[i] = box_tri_key(f3{p[0], p[1], p[2]}, f3{p[3], p[4], p[5]}, f3{p[6], p[7], p[8]}, f3{p[9], p[10], p[11]}, f3{p[12], p[13], p[14]});
    }
    for (size_t i = 0; i < (size_t)head[1]; i++) {
        const float* p = &sph[i * 10];
        out[(size_t)head[0] + i] = box_sphere_key(f3{p[0], p[1], p[2]}, f3{p[3], p[4], p[5]}, float4{p[6], p[7], p[8], p[9]});
    }
    f = fopen(argv[2], "wb");
    if (!f) return 1;
    const bool ok = fwrite(out.data(), 4, out.size(), f) == out.size();
    return fclose(f) == 0 && ok ? 0 : 1;
}
