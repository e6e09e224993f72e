#!/usr/bin/env python3
"""Generate tests/golden/* — run in the build container only (needs /root/reference).

TEST INFRASTRUCTURE.  Two kinds of fixture are written:

 * ref_*.npz   inputs + outputs of oracle/_ref/ptref, the partial build of the REAL
               reference (srcs/bvh.cpp, srcs/CudaPrimitive.cu, srcs/camera.cpp, include/CudaPrimitive.cuh,
               include/CudaVector.cuh, include/image.h compiled unmodified — see oracle/Makefile).  These are
               data (vectors), not reference source.
 * oracle_*.npz images / ray tables produced by the CPU restatement under the pinned
               contract (o_set_libm(1)); they pin the oracle against regressions and let
               the GPU tests run where the oracle build is unavailable.
 * ref_bxdf / ref_raycast / ref_nee / ref_image_*_b8.npz  inputs + outputs of oracle/_ref/ptref_int, the REAL reference's integrator
               headers (include/CudaUtil.cuh, include/Bxdf.cuh) as host C++ behind oracle/curand_shim.h — gen_integrator() below.
 * ref_attr.npz the same binary on scenes_util.attribute_scene (per-vertex frames and materials, glass triangles, eight lights, ties,
               slivers) — gen_attr() below.
 * anchors.json the three image means recorded in SURVEY.md Appendix A (measured by the
               survey on the reference's own source) — reproduced here with o_set_libm(0).
"""
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "pathtrace-on-cuda_amd"))
import oracle_lib as O  # noqa: E402
import ptamd  # noqa: E402
from scenes_util import ATTR_RAY_SETS, attr_nee_rows, attribute_rays, attribute_scene, leaving_parents, leaving_rays, bxdf_inputs, jittered_grid, random_rays10, random_tris48, random_spheres16, scene_rays8, test_spheres  # noqa: E402
import query_ref  # noqa: E402

G = os.path.join(ROOT, "tests", "golden")


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def gen_camera_u8():
    """ref_camera.npz / ref_u8.npz: the REAL srcs/camera.cpp (Camera ctor + SetRotation + GetForward/GetUp/GetRight) and
    include/image.h (ConverToUint8) through oracle/_ref/ptref.  Own random stream, so the other fixtures are untouched."""
    rs = np.random.RandomState(4321)
    rot = np.concatenate([
        np.array([[0, 90, 0], [0, 0, 0], [0, 180, 0], [0, 90, 360], [0, 90, -90], [0, 200, 725], [0, -30, -725],
                  [359.5, 45, 45], [-10, 135, 180], [0, 1e-3, 270], [0, 179.999, 90]], np.float32),
        np.stack([rs.uniform(-400, 400, 500), rs.uniform(-20, 200, 500), rs.uniform(-800, 800, 500)], 1).astype(np.float32)])
    np.savez_compressed(os.path.join(G, "ref_camera.npz"), rot=rot, basis=O.ref_camera(rot))
    k = np.arange(0, 257, dtype=np.float64)
    edges = (k / 255.99).astype(np.float32)                     # the values where the result steps, and their float neighbours
    vals = np.concatenate([np.linspace(0.0, 1.0, 4097, dtype=np.float32), edges, np.nextafter(edges, np.float32(-1)), np.nextafter(edges, np.float32(2)),
                           rs.uniform(0.0, 1.0, 4096).astype(np.float32)])
    vals = vals[(vals >= 0.0) & (vals <= 1.0)]                   # ACESFilm saturates to [0,1]; outside it the cast is undefined behaviour
    np.savez_compressed(os.path.join(G, "ref_u8.npz"), values=vals, u8=O.ref_u8(vals))
    print("ref_camera.npz", rot.shape, "ref_u8.npz", vals.shape)


def gen_png():
    """ref_png.npz: small images and the PNG files the REAL srcs/image.cpp (Image(W,H,C) + Image::WriteTo, the reference's own vendored
    stb_image_write.h) writes for them, through oracle/_ref/ptref pngwrite.  Data: pixels in, file bytes out."""
    import tempfile
    rs = np.random.RandomState(777)
    out = {}
    for key, (H, W, C) in {"rgb": (21, 37, 3), "gray": (5, 9, 1), "rgba": (8, 8, 4)}.items():
        px = rs.randint(0, 256, (H, W, C)).astype(np.uint8)
        px[: H // 2, :, :] = (np.arange(W)[None, :, None] * 7 % 256).astype(np.uint8)      # smooth rows too, so filters / matches get used
        with tempfile.TemporaryDirectory() as d:
            q = os.path.join(d, "o.png")
            O.ref_png_write(px, q)
            assert np.array_equal(O.ref_png_read(q), px)
            out[key] = px
            out[key + "_png"] = np.frombuffer(open(q, "rb").read(), np.uint8)
    np.savez_compressed(os.path.join(G, "ref_png.npz"), **out)
    print("ref_png.npz", {k: v.shape for k, v in out.items()})


def gen_rocrand():
    """ref_rocrand_xorwow.npz: rocRAND's own XORWOW engine (oracle/rocrand_ref.cpp, host build of /opt/rocm/include/rocrand/rocrand_xorwow.h)
    for the seeds the renderer uses: pixel offset + pass * W * H, small and beyond 2^32."""
    seeds = np.array([0, 1, 2, 255, 256 * 256, 1920 * 1080 - 1, 1920 * 1080 * 7 + 12345, 2 ** 31 - 1, 2 ** 32 - 1, 2 ** 32 + 5, 2 ** 40 + 123456789,
                      2 ** 63 + 17], dtype=np.uint64)
    raw, uni = [], []
    for s in seeds:
        r, u = O.rocrand_ref(int(s), 96)
        raw.append(r); uni.append(u)
    np.savez_compressed(os.path.join(G, "ref_rocrand_xorwow.npz"), seeds=seeds, raw=np.stack(raw), uniform=np.stack(uni))
    print("ref_rocrand_xorwow.npz", np.stack(raw).shape)

N_BXDF_RANDOM = 2048
BXDF_SEED = 4100          # + lobe


def _unit(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def bxdf_edge_block(lobe):
    """Hand-built rows (in28) at the places where eval / sample / pdf go wrong: n.wo from 1e-2 down to 1e-7 and exactly 0, on either side
    of the surface, with front face 0 and 1 (total internal reflection for lobes 2 and 3); wo equal to n; wi equal to reflect(wo), to -wo,
    exactly in the tangent plane; roughness 0, 0.0099, 0.01, 0.0101, 0.02 and 1 (the integrator's lobe threshold is 1e-2) times metallic
    0 / 1, albedo 0 / 1, specular 0 (eta 1), 0.04 and 0.2.  Two frames: the axes (dot products exact) and a rotated one."""
    rs = np.random.RandomState(BXDF_SEED + 50 + lobe)
    frames = [(np.array([0., 0, 1]), np.array([1., 0, 0]), np.array([0., 1, 0]))]
    n = _unit([0.36, -0.48, 0.8]); t = _unit(np.cross(n, [0.0, 0.0, 1.0])); frames.append((n, t, np.cross(n, t)))
    base_rough = 0.0 if lobe in (1, 3) else 0.2
    rows = []

    def add(fr, front, albedo, spec, rough, metal, wo, wi):
        n, t, b = fr
        rows.append(np.concatenate([n, t, b, [front], np.full(3, albedo), np.full(3, spec), [rough, metal], wo, wi]))

    def reflect(w, n):
        return -w + 2 * np.dot(n, w) * n

    for fr in frames:
        n, t, b = fr
        tang = _unit(0.6 * t + 0.8 * b)
        up = _unit(0.5 * n + 0.3 * t - 0.4 * b)
        # grazing wo, both sides, both faces
        for c in (1e-2, 1e-3, 1e-4, 1e-5, 1e-6, 1e-7, 0.0):
            for side in (1.0, -1.0):
                wo = side * c * n + np.sqrt(1 - c * c) * tang
                for front in (1.0, 0.0):
                    for spec in (0.04, 0.2):
                        for wi in (reflect(wo, n), -wo, _unit(-0.3 * t + 0.7 * b), up, -up):
                            add(fr, front, 0.7, spec, base_rough, 0.0, wo, wi)
        # wo equal to n (and to -n)
        for wo in (n, -n):
            for front in (1.0, 0.0):
                for wi in (n, -n, tang, up, -up):
                    add(fr, front, 0.7, 0.04, base_rough, 0.0, wo, wi)
        # material sweep at a generic wo
        wo = _unit(0.7 * n + 0.5 * t + 0.2 * b)
        for rough in (0.0, 0.0099, 0.01, 0.0101, 0.02, 1.0):
            for metal in (0.0, 1.0):
                for albedo in (0.0, 1.0):
                    for spec in (0.0, 0.04, 0.2):
                        for front in (1.0, 0.0):
                            for wi in (reflect(wo, n), up, -up, tang, -wo):
                                add(fr, front, albedo, spec, rough, metal, wo, wi)
    a = np.array(rows).astype(np.float32)
    seeds = rs.randint(0, 2 ** 31, (a.shape[0], 2)).astype(np.uint32).view(np.float32)
    return np.concatenate([a, seeds, np.zeros((a.shape[0], 2), np.float32)], 1)


def bxdf_random_block(lobe):
    a, seeds = bxdf_inputs(N_BXDF_RANDOM, np.random.RandomState(BXDF_SEED + lobe), lobe)
    return np.concatenate([a, seeds, np.zeros((a.shape[0], 2), np.float32)], 1)


def _sparse(full, base):
    """Rows of `full` whose bits differ from `base` (NaN payloads included): indices and rows."""
    d = np.nonzero((full.view(np.uint32) != base.view(np.uint32)).any(1))[0].astype(np.int32)
    return d, full[d]


def nee_rows(so):
    """2,048 rows of o_nee's in5 on the lat_lon 24 scene with the test spheres: hit points of rays cast into the scene, the same points
    pushed just under their surface, and points on and just under the light's plane."""
    rs = np.random.RandomState(4200)
    hits, prim, _ = so.raycast(scene_rays8(4000, rs))
    h = hits[prim >= 0]
    on = h[:1300, 5:8]
    under = (h[1300:1748, 5:8] - np.float32(1e-3) * h[1300:1748, 8:11]).astype(np.float32)
    lit = np.concatenate([np.stack([rs.uniform(-5, 5, 150), np.full(150, 39.98), rs.uniform(-5, 5, 150)], 1),
                          np.stack([rs.uniform(-20, 20, 150), np.full(150, 39.999), rs.uniform(-20, 20, 150)], 1)])
    pts = np.concatenate([on, under, lit]).astype(np.float32)
    assert pts.shape[0] == 2048
    seeds = rs.randint(0, 2 ** 32, (pts.shape[0], 2), dtype=np.uint64).astype(np.uint32)
    return np.concatenate([pts, seeds.view(np.float32)], 1)


INTEGRATOR_SCENES = (("cornell", 0, False), ("standin24", 1, False), ("standin24_spheres", 1, True))
N_LONG = 1024
LONG_SEED = 4300


def gen_integrator():
    """ref_bxdf / ref_raycast / ref_nee / ref_image_standin24_spheres_b8: what the REAL reference's integrator (oracle/_ref/ptref_int)
    answers.  Own random streams, so every other fixture regenerates unchanged.  Data only: table rows in, table rows out.

    ref_bxdf.npz      per lobe: the hand-built edge block (inputs stored), the sha256 of the 2,048 random rows (regenerated by
                      scenes_util.bxdf_inputs from BXDF_SEED + lobe: 2,048 x 28 random floats x 4 lobes would be 0.9 MB), the reference's
                      rows in contract mode for random + edge, and the rows that differ in glibc mode (indices + rows).
    ref_raycast.npz   per scene: the reference's HIT records for the 4,096 scene_rays8 rays that oracle_<scene>.npz already stores, and for
                      1,024 query_ref.set_c segments (stored once).  RayCast reaches no libm function besides sqrt: both modes, one answer.
    ref_nee.npz       2,048 rows in, the reference's columns out."""
    if not O.have_ref_int():
        raise SystemExit("oracle/_ref/ptref_int missing: run `make -C oracle ref` first")
    out = {}
    for lobe in range(4):
        rnd, edge = bxdf_random_block(lobe), bxdf_edge_block(lobe)
        in28 = np.concatenate([rnd, edge])
        con, gl = O.ref_int_bxdf(lobe, in28, 1), O.ref_int_bxdf(lobe, in28, 0)
        idx, rows = _sparse(gl, con)
        out.update({f"edge_in28_{lobe}": edge, f"random_sha256_{lobe}": np.array(sha(rnd)), f"contract_{lobe}": con,
                    f"glibc_idx_{lobe}": idx, f"glibc_rows_{lobe}": rows})
        print(f"ref_bxdf lobe {lobe}: {rnd.shape[0]} random + {edge.shape[0]} edge rows, {idx.size} differ between the libm modes")
    np.savez_compressed(os.path.join(G, "ref_bxdf.npz"), n_random=N_BXDF_RANDOM, seed=BXDF_SEED, **out)

    longs = query_ref.set_c(N_LONG, np.random.RandomState(LONG_SEED))
    out = {"long_rays8": longs}
    worlds = {}
    for name, kind, with_sph in INTEGRATOR_SCENES:
        nodes, tris, _ = O.bvh_build(ptamd.gen_scene(kind, 24))
        sph = test_spheres() if with_sph else None
        worlds[name] = (nodes, tris, sph)
        rays8 = np.load(os.path.join(G, f"oracle_{name}.npz"))["rays8"]
        for mode in (0, 1):
            hits = O.ref_int_raycast(nodes, tris, sph, np.concatenate([rays8, longs]), mode)
            assert mode == 0 or np.array_equal(hits.view(np.uint32), prev.view(np.uint32))
            prev = hits
        out[f"hits_{name}"], out[f"long_hits_{name}"] = hits[:len(rays8)], hits[len(rays8):]
        print(f"ref_raycast {name}: {int(hits[:len(rays8), 0].sum())} of {len(rays8)} rays hit, {int(hits[len(rays8):, 0].sum())} of {N_LONG} segments")
    np.savez_compressed(os.path.join(G, "ref_raycast.npz"), **out)

    nodes, tris, sph = worlds["standin24_spheres"]
    in5 = nee_rows(O.Scene(nodes, tris, sph))
    nee = [O.ref_int_nee(nodes, tris, sph, in5, mode) for mode in (0, 1)]
    assert np.array_equal(nee[0].view(np.uint32), nee[1].view(np.uint32))      # SamplePrimitive / GetLightColor: sqrt only
    np.savez_compressed(os.path.join(G, "ref_nee.npz"), in5=in5, out12=nee[1], cols=np.array(O.NEE_REF_COLS))
    print("ref_nee: lit rows", int((nee[1][:, 8:11].sum(1) > 0).sum()), "of", len(in5))

    img = O.ref_int_render(nodes, tris, sph, O.make_camera(64, 64), 2, 8, 1)
    np.savez_compressed(os.path.join(G, "ref_image_standin24_spheres_b8.npz"), image=img, passes=2, spp=8, max_bounce=8, spheres=sph)
    print("ref_image_standin24_spheres_b8: mean", img.mean(dtype=np.float64))
    for f in ("ref_bxdf", "ref_raycast", "ref_nee", "ref_image_standin24_spheres_b8"):
        print(f, os.path.getsize(os.path.join(G, f + ".npz")), "bytes")


ATTR_SEED = 7
ATTR_N_RAYS = 2000


def gen_attr(seed=ATTR_SEED):
    """ref_attr.npz: what the REAL reference's integrator (oracle/_ref/ptref_int, contract mode) answers on scenes_util.attribute_scene
    with the test spheres: HIT records of the four ray sets, one NEE table, one 64 x 64 frame of 2 passes x 8 spp.  Scene, rays and NEE
    rows are regenerated from the seed by the tests (scenes_util.load_ref_attr); their sha256 is stored, results only otherwise."""
    if not O.have_ref_int():
        raise SystemExit("oracle/_ref/ptref_int missing: run `make -C oracle ref` first")
    prims, groups = attribute_scene(seed)
    nodes, tris, _ = O.bvh_build(prims)
    sph = test_spheres()
    rays = attribute_rays(prims, groups, seed + 1, ATTR_N_RAYS)
    out = {"seed": seed, "lat_lon": 12, "n_rays": ATTR_N_RAYS, "prims_sha256": np.array(sha(prims)), "spheres": sph}
    for name in ATTR_RAY_SETS:
        if name == "leaving":
            rays[name] = leaving_rays(*leaving_parents(rays, out["hits_scene"], out["hits_aimed"]), seed + 2)
        for mode in (0, 1):      # RayCast reaches no libm function besides sqrt: both modes, one answer
            hits = O.ref_int_raycast(nodes, tris, sph, rays[name], mode)
            assert mode == 0 or np.array_equal(hits.view(np.uint32), prev.view(np.uint32))
            prev = hits
        out[f"hits_{name}"], out[f"rays_sha256_{name}"] = hits, np.array(sha(rays[name]))
        print(f"ref_attr {name}: {int(hits[:, 0].sum())} of {len(hits)} rays hit")
    in5 = attr_nee_rows(np.concatenate([out["hits_scene"], out["hits_aimed"]]), seed + 3)
    nee = [O.ref_int_nee(nodes, tris, sph, in5, mode) for mode in (0, 1)]
    assert np.array_equal(nee[0].view(np.uint32), nee[1].view(np.uint32))
    out.update(nee_in5_sha256=np.array(sha(in5)), nee_out12=nee[1], nee_cols=np.array(O.NEE_REF_COLS))
    print("ref_attr nee: lit rows", int((nee[1][:, 8:11].sum(1) > 0).sum()), "of", len(in5))
    img = O.ref_int_render(nodes, tris, sph, O.make_camera(64, 64), 2, 8, 1)
    out.update(image=img, passes=2, spp=8, max_bounce=8)
    np.savez_compressed(os.path.join(G, "ref_attr.npz"), **out)
    print("ref_attr: image mean", img.mean(dtype=np.float64), os.path.getsize(os.path.join(G, "ref_attr.npz")), "bytes")


def main():
    os.makedirs(G, exist_ok=True)
    if not O.have_ref():
        raise SystemExit("oracle/_ref/ptref missing: run `make -C oracle ref` first")
    if len(sys.argv) > 1 and sys.argv[1] == "rocrand":
        if not O.have_rocrand_ref():
            raise SystemExit("oracle/_build/rocrand_ref missing: run `make -C oracle rocrand` first")
        gen_rocrand()
        return
    if len(sys.argv) > 1 and sys.argv[1] == "png":
        gen_png()
        return
    if len(sys.argv) > 1 and sys.argv[1] == "integrator":
        gen_integrator()
        return
    if len(sys.argv) > 1 and sys.argv[1] == "attr":
        gen_attr()
        return
    if len(sys.argv) > 1 and sys.argv[1] == "camera_u8":
        gen_camera_u8()
        return
    gen_camera_u8()
    rs = np.random.RandomState(1234)

    # ---- G1: BVH build + flatten, real reference ----
    cornell = ptamd.gen_scene(0)
    n, t = O.ref_bvh(cornell)
    np.savez_compressed(os.path.join(G, "ref_bvh_cornell.npz"), prims=cornell, nodes=n, tris=t)
    grid = jittered_grid(50, 50, rs)            # 5000 triangles, many centroid ties
    n, t = O.ref_bvh(grid)
    np.savez_compressed(os.path.join(G, "ref_bvh_grid5000.npz"), prims=grid, nodes=n, tris=t)
    hashes = {}
    for name, kind, ll in (("standin187", 1, 187), ("standin4x187", 2, 187), ("standin24", 1, 24)):
        prims = ptamd.gen_scene(kind, ll)
        n, t = O.ref_bvh(prims)
        hashes[name] = {"kind": kind, "lat_lon": ll, "n_prims": int(prims.shape[0]), "n_nodes": int(n.size // 40),
                        "prims_sha256": sha(prims), "nodes_sha256": sha(n), "tris_sha256": sha(t)}
    json.dump(hashes, open(os.path.join(G, "ref_bvh_hashes.json"), "w"), indent=1)

    # ---- G2a: Triangle::hit / Sphere::hit / vec3, real reference ----
    tris48 = random_tris48(64, rs)
    rays = random_rays10(4096, 64, tris48, rs)
    np.savez_compressed(os.path.join(G, "ref_trihit.npz"), tris48=tris48, rays10=rays, hits=O.ref_tri_hit(tris48, rays))
    sph = random_spheres16(8, rs)
    srays = random_rays10(2048, 8, None, rs, spheres=sph)
    np.savez_compressed(os.path.join(G, "ref_sphit.npz"), sph16=sph, rays10=srays, hits=O.ref_sphere_hit(sph, srays))
    v = rs.standard_normal((2048, 7)).astype(np.float32)
    v[:, 6] = rs.uniform(0.3, 3.0, 2048).astype(np.float32)
    v[::7, 3:6] /= np.linalg.norm(v[::7, 3:6], axis=1, keepdims=True)
    np.savez_compressed(os.path.join(G, "ref_vecmath.npz"), in7=v, out21=O.ref_vecmath(v))

    # ---- anchors from SURVEY.md Appendix A ----
    json.dump({"cornell_256x256_1x16": 0.478260, "standin1_320x180_1x4": 0.294783, "standin4_320x180_1x4": 0.296273,
               "source": "SURVEY.md Appendix A (survey probe of the reference's own source, glibc libm, no FMA)"},
              open(os.path.join(G, "anchors.json"), "w"), indent=1)

    # ---- G2b/G5: oracle ray tables and images under the pinned contract ----
    O.set_libm(1)
    scenes = {
        "cornell": (ptamd.gen_scene(0), None),
        "standin24": (ptamd.gen_scene(1, 24), None),
        "standin24_spheres": (ptamd.gen_scene(1, 24), test_spheres()),
    }
    for name, (prims, sph) in scenes.items():
        nodes, tris, _ = O.bvh_build(prims)
        sc = O.Scene(nodes, tris, sph)
        rays8 = scene_rays8(4096, rs)
        hits, prim, cnt = sc.raycast(rays8)
        W = H = 64
        cam = O.make_camera(W, H)
        prm = O.make_params(W, H, passes=2, spp=8, max_bounce=12 if sph is not None else 8)
        img, icnt = sc.render(cam, prm, 8)
        np.savez_compressed(os.path.join(G, f"oracle_{name}.npz"), rays8=rays8, hits=hits, prim=prim, ray_counters=cnt,
                            image=img, image_counters=icnt, passes=2, spp=8, max_bounce=prm.max_bounce,
                            spheres=np.zeros((0, 16), np.float32) if sph is None else sph)
        print(name, "image mean", img.mean(dtype=np.float64), "hits", int((prim >= 0).sum()))
    gen_integrator()      # after the oracle_*.npz files: it takes their rays
    gen_attr()
    print("golden fixtures written to", G)


if __name__ == "__main__":
    main()
