// tri_host.cpp — tri_tri_key, tri_sphere_key and tri_node_test of csrc/pt_tri.h compiled for the host, so that the numpy restatement of
// tests/tri_ref.py can be held against the kernels' own arithmetic bit for bit without a GPU (tests/test_tri_queries.py).
// The functions are plain inline C++ once PT_DEV is defined away; the test copies the header's self-contained part (between its
// "self-contained: begin" and "self-contained: end" lines) into tri_kernel_fns.inc and compiles this file with the library's
// numerics flags next to it:
//   g++ -std=c++17 -O2 -ffp-contract=off -fno-fast-math -I <dir of tri_kernel_fns.inc> tools/tri_host.cpp -o tri_host
//   tri_host <in> <out>
// in:  int32 n_tri, n_sph, n_box | n_tri pairs of 18 floats: the query qa qb qc, the record a.xyz ab.xyz ac.xyz | n_sph pairs of 13
//      floats: the query, c.xyz rad | n_box pairs of 15 floats: the query, lo.xyz hi.xyz of a node's box
// out: n_tri records of 7 floats: the key (1 or +inf), p.xyz, q.xyz (zeros for a non-member) | n_sph records of 4 floats: the key, the
//      closest point (zeros for a non-member) | n_box floats: 1 if tri_node_test enters the box, else 0
#include <cstdint>
#include <cstdio>
#include <vector>

#define PT_DEV static inline
struct f3 {
    float x, y, z;
    f3() {}
    f3(float a, float b, float c) : x(a), y(b), z(c) {}
};
#include "tri_kernel_fns.inc"

int main(int argc, char** argv)
{
    if (argc < 3) { fprintf(stderr, "usage: tri_host <in> <out>\n"); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 1;
    int32_t head[3];
    if (fread(head, 4, 3, f) != 3 || head[0] < 0 || head[1] < 0 || head[2] < 0) return 1;
    const size_t nt = (size_t)head[0], ns = (size_t)head[1], nb = (size_t)head[2];
    std::vector<float> tri(nt * 18), sph(ns * 13), box(nb * 15), out(nt * 7 + ns * 4 + nb);
    if (fread(tri.data(), 4, tri.size(), f) != tri.size() || fread(sph.data(), 4, sph.size(), f) != sph.size() ||
        fread(box.data(), 4, box.size(), f) != box.size())
        return 1;
    fclose(f);
    for (size_t i = 0; i < nt; i++) {
        const float* v = &tri[i * 18];
        const TriLane L = tri_lane(f3(v[0], v[1], v[2]), f3(v[3], v[4], v[5]), f3(v[6], v[7], v[8]));
        f3 p(0.f, 0.f, 0.f), q(0.f, 0.f, 0.f);
        float* o = &out[i * 7];
        o[0] = tri_tri_key(L, f3(v[9], v[10], v[11]), f3(v[12], v[13], v[14]), f3(v[15], v[16], v[17]), p, q);
        const bool m = o[0] == 1.f;
        o[1] = m ? p.x : 0.f; o[2] = m ? p.y : 0.f; o[3] = m ? p.z : 0.f;
        o[4] = m ? q.x : 0.f; o[5] = m ? q.y : 0.f; o[6] = m ? q.z : 0.f;
    }
    for (size_t i = 0; i < ns; i++) {
        const float* v = &sph[i * 13];
        f3 c(0.f, 0.f, 0.f);
        float* o = &out[nt * 7 + i * 4];
        o[0] = tri_sphere_key(f3(v[0], v[1], v[2]), f3(v[3], v[4], v[5]), f3(v[6], v[7], v[8]), f3(v[9], v[10], v[11]), v[12], c);
        const bool m = o[0] == 1.f;
        o[1] = m ? c.x : 0.f; o[2] = m ? c.y : 0.f; o[3] = m ? c.z : 0.f;
    }
    for (size_t i = 0; i < nb; i++) {
        const float* v = &box[i * 15];
        const TriLane L = tri_lane(f3(v[0], v[1], v[2]), f3(v[3], v[4], v[5]), f3(v[6], v[7], v[8]));
        out[nt * 7 + ns * 4 + i] = tri_node_test(L, f3(v[9], v[10], v[11]), f3(v[12], v[13], v[14])) ? 1.f : 0.f;
    }
    f = fopen(argv[2], "wb");
    if (!f) return 1;
    const bool ok = fwrite(out.data(), 4, out.size(), f) == out.size();
    return fclose(f) == 0 && ok ? 0 : 1;
}
