// dump_accel.cpp — writes the five device arrays pt_build_accel produces (wide, quad, tri, tripair, leafbox) of a procedural scene
// or of the raw PtPrimitive records in a file, to <out_prefix>.<name>.bin, so that two builds of host/accel_build.cpp can be compared
// byte for byte (tests/test_dynamic.py keeps the hashes of the build before the refit maps were added) and so that a CPU test can read
// the trees of any scene as they are uploaded (tests/test_slack.py).  PTAMD_TREE / PTAMD_LEAF act as at upload.
//   g++ -std=c++17 -O2 -I include tools/dump_accel.cpp pathtrace-on-cuda_amd/build/{accel_build,bvh_build,scenes,pt_host,obj_loader}.o -pthread -o dump_accel
//   dump_accel <kind> <lat_lon> <out_prefix>
//   dump_accel --prims <file> <out_prefix>      the file: n * sizeof(PtPrimitive) bytes, as scenes_util.make_prims builds them
#include <cstdio>
#include <cstdlib>
#include <cstring>
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
    if (argc < 4) { fprintf(stderr, "usage: dump_accel <kind> <lat_lon> <out_prefix> | dump_accel --prims <file> <out_prefix>\n"); return 2; }
    const std::string pre = argv[3];
    std::vector<PtPrimitive> prims;
    if (!strcmp(argv[1], "--prims")) {
        FILE* f = fopen(argv[2], "rb");
        if (!f) { fprintf(stderr, "cannot open %s\n", argv[2]); return 1; }
        fseek(f, 0, SEEK_END);
        const long bytes = ftell(f);
        fseek(f, 0, SEEK_SET);
        if (bytes < (long)sizeof(PtPrimitive) || bytes % (long)sizeof(PtPrimitive)) { fprintf(stderr, "%s: not a whole number of PtPrimitive records\n", argv[2]); fclose(f); return 1; }
        prims.resize((size_t)bytes / sizeof(PtPrimitive));
        const bool ok = fread(prims.data(), sizeof(PtPrimitive), prims.size(), f) == prims.size();
        fclose(f);
        if (!ok) { fprintf(stderr, "%s: short read\n", argv[2]); return 1; }
    } else {
        const int kind = atoi(argv[1]), ll = atoi(argv[2]);
        const int n = pt_scene_gen(kind, ll, nullptr, 0);
        if (n < 1) { fprintf(stderr, "no such scene\n"); return 1; }
        prims.resize((size_t)n);
        pt_scene_gen(kind, ll, prims.data(), n);
    }
    const int n = (int)prims.size();
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
