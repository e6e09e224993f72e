// sweep_host.cpp — sweep_tri_key, sweep_sphere_key and sweep_node_test of csrc/pt_sweep.h compiled for the host, so that the numpy
// restatement of tests/sweep_ref.py can be held against the kernels' own arithmetic bit for bit without a GPU (tests/test_sweep.py).
// The functions are plain inline C++ once PT_DEV is defined away; the test copies the header's self-contained part (between its
// "self-contained: begin" and "self-contained: end" lines) into sweep_kernel_fns.inc and compiles this file with the library's
// numerics flags next to it:
//   g++ -std=c++17 -O2 -ffp-contract=off -fno-fast-math -I <dir of sweep_kernel_fns.inc> tools/sweep_host.cpp -o sweep_host
//   sweep_host <in> <out>
// in:  int32 n_tri, n_sph, n_box | n_tri pairs of 17 floats: the SWEEP8 record o.xyz r d.xyz tmax, a.xyz ab.xyz ac.xyz | n_sph pairs of
//      12 floats: the record, c.xyz rad | n_box pairs of 15 floats: the record, bound, lo.xyz hi.xyz of a node's box
// out: n_tri + n_sph floats: tau of every pair (a triangle's with bound = tmax: tau itself) | n_box pairs of 2 floats: 1 if
//      sweep_node_test enters the box, else 0; the key it sorts the box by.  inv = 1 / d per axis and r2 = r * r as sweep_lane forms them.
#include <cstdint>
#include <cstdio>
#include <vector>

#define PT_DEV static inline
struct f3 {
    float x, y, z;
    f3() {}
    f3(float a, float b, float c) : x(a), y(b), z(c) {}
};
#include "sweep_kernel_fns.inc"

int main(int argc, char** argv)
{
    if (argc < 3) { fprintf(stderr, "usage: sweep_host <in> <out>\n"); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 1;
    int32_t head[3];
    if (fread(head, 4, 3, f) != 3 || head[0] < 0 || head[1] < 0 || head[2] < 0) return 1;
    const size_t nt = (size_t)head[0], ns = (size_t)head[1], nb = (size_t)head[2];
    std::vector<float> tri(nt * 17), sph(ns * 12), box(nb * 15), out(nt + ns + 2 * nb);
    if (fread(tri.data(), 4, tri.size(), f) != tri.size() || fread(sph.data(), 4, sph.size(), f) != sph.size() ||
        fread(box.data(), 4, box.size(), f) != box.size())
        return 1;
    fclose(f);
    for (size_t i = 0; i < nt; i++) {
        const float* p = &tri[i * 17];
        const f3 o(p[0], p[1], p[2]), d(p[4], p[5], p[6]), inv(1.f / p[4], 1.f / p[5], 1.f / p[6]);
        out[i] = sweep_tri_key(o, d, inv, p[3], p[3] * p[3], p[7], p[7], f3(p[8], p[9], p[10]), f3(p[11], p[12], p[13]), f3(p[14], p[15], p[16]));
    }
    for (size_t i = 0; i < ns; i++) {
        const float* p = &sph[i * 12];
        out[nt + i] = sweep_sphere_key(f3(p[0], p[1], p[2]), f3(p[4], p[5], p[6]), p[3], p[3] * p[3], p[7], f3(p[8], p[9], p[10]), p[11]);
    }
    for (size_t i = 0; i < nb; i++) {
        const float* p = &box[i * 15];
        const f3 o(p[0], p[1], p[2]), d(p[4], p[5], p[6]), inv(1.f / p[4], 1.f / p[5], 1.f / p[6]);
        float key;
        const bool in = sweep_node_test(o, d, inv, p[3], p[3] * p[3], p[7], p[8], f3(p[9], p[10], p[11]), f3(p[12], p[13], p[14]), key);
        out[nt + ns + 2 * i] = in ? 1.f : 0.f;
        out[nt + ns + 2 * i + 1] = key;
    }
    f = fopen(argv[2], "wb");
    if (!f) return 1;
    const bool ok = fwrite(out.data(), 4, out.size(), f) == out.size();
    return fclose(f) == 0 && ok ? 0 : 1;
}
