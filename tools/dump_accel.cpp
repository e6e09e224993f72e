// dump_accel.cpp — writes the five device arrays pt_build_accel produces (wide, quad, tri, tripair, leafbox) of a procedural scene
// to <out_prefix>.<name>.bin, so that two builds of host/accel_build.cpp can be compared byte for byte (tests/test_dynamic.py keeps
// the hashes of the build before the refit maps were added).  PTAMD_TREE / PTAMD_LEAF act as at upload.
//   g++ -std=c++17 -O2 -I include tools/dump_accel.cpp pathtrace-on-cuda_amd/build/{accel_build,bvh_build,scenes,pt_host,obj_loader}.o -pthread -o dump_accel
//   dump_accel <kind> <lat_lon> <out_prefix>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>
#include "../include/pt_api.h"
#include "../pathtrace-on-cuda_amd/host/accel_build.h"

static bool put(const std::string& path, const void* p, size_t bytes)
{
    FILE* f = fopen(path.c_str(), "wb");
    if (!f) return false;
    const bool ok = fwrite(p, 1, bytes, f) == bytes;
    return fclose(f) == 0 && ok;
}

int main(int argc, char** argv)
{
    if (argc < 4) { fprintf(stderr, "usage: dump_accel <kind> <lat_lon> <out_prefix>\n"); return 2; }
    const int kind = atoi(argv[1]), ll = atoi(argv[2]);
    const std::string pre = argv[3];
    const int n = pt_scene_gen(kind, ll, nullptr, 0);
    if (n < 1) { fprintf(stderr, "no such scene\n"); return 1; }
    std::vector<PtPrimitive> prims((size_t)n);
    pt_scene_gen(kind, ll, prims.data(), n);
    PtFlatBVH* bvh = nullptr;
    if (pt_bvh_build_sah(prims.data(), n, &bvh)) { fprintf(stderr, "build failed\n"); return 1; }
    PtAccel a;
    pt_build_accel(pt_bvh_nodes(bvh), pt_bvh_num_nodes(bvh), pt_bvh_tris(bvh), pt_bvh_num_tris(bvh), a);
    const bool ok = put(pre + ".wide.bin", a.wide.data(), a.wide.size() * 4) && put(pre + ".quad.bin", a.quad.data(), a.quad.size() * 4) &&
                    put(pre + ".tri.bin", a.tri.data(), a.tri.size() * 4) && put(pre + ".tripair.bin", a.tripair.data(), a.tripair.size() * 4) &&
                    put(pre + ".leafbox.bin", a.leafbox.data(), a.leafbox.size() * 4);
    pt_bvh_free(bvh);
    return ok ? 0 : 1;
}
