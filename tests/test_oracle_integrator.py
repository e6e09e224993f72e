"""The oracle's integrator half against the REAL reference's integrator: include/CudaUtil.cuh and include/Bxdf.cuh compiled unmodified as
host C++ (oracle/_ref/ptref_int: oracle/ref_int_driver.cpp behind oracle/curand_shim.h, see oracle/Makefile).  Committed fixtures
(tests/golden/ref_bxdf, ref_raycast, ref_nee, ref_image_standin24_spheres_b8) always; the binary itself live where it was built.

Both libm modes are compared like with like — o_set_libm(0) with the binary's `glibc`, o_set_libm(1) with its `contract` —, so every
comparison is bit for bit, NaN equal to NaN, on every row: there is nothing to tolerate.

All three anchors of anchors.json run through the live binary (the 320 x 180 stand-ins take a few seconds each on 16 processes).
Depth 12 (MAX_BOUNCE is a compile-time 8 in the reference) stays oracle-only."""
import json
import os

import numpy as np
import pytest

import oracle_lib as O
import ptamd
from scenes_util import load_ref_bxdf, scene_rays8
from scenes_util import test_spheres as make_test_spheres

live = pytest.mark.skipif(not O.have_ref_int(), reason="oracle/_ref/ptref_int not built (reference tree absent)")
SCENES = {"cornell": (0, False), "standin24": (1, False), "standin24_spheres": (1, True)}


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def differing_rows(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    same = (bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))
    return np.nonzero(~same.reshape(same.shape[0], -1).all(1))[0]


@pytest.fixture()
def libm():
    """Sets the oracle's libm mode for a test and puts the old one back."""
    old = O.set_libm(1)

    def set_mode(mode):
        O.set_libm(mode)
    yield set_mode
    O.set_libm(old)


_WORLDS = {}


def world(name):
    if name not in _WORLDS:
        kind, with_sph = SCENES[name]
        nodes, tris, _ = O.bvh_build(ptamd.gen_scene(kind, 24))
        _WORLDS[name] = (nodes, tris, make_test_spheres() if with_sph else None)
    return _WORLDS[name]


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("lobe", [0, 1, 2, 3])
def test_bxdf_tables_equal_the_references(golden_dir, libm, lobe, mode):
    in28, contract, glibc, n_random = load_ref_bxdf(golden_dir, lobe)
    want = contract if mode else glibc
    libm(mode)
    bad = differing_rows(O.bxdf(lobe, in28), want)
    assert bad.size == 0, f"lobe {lobe}, libm {O.LIBM_MODES[mode]}: {bad.size} rows differ from the reference, first {bad[:8]} (edge block starts at {n_random})"
    # the table is worth something: finite non-zero evaluations, NaN rows and zero rows all occur
    e = want[:, :3]
    assert (np.isfinite(e).all(1) & (np.abs(e).sum(1) > 0)).sum() > 400 and (e == 0).all(1).sum() > 100
    assert in28.shape[0] - n_random > 1000


def test_the_libm_switch_of_the_reference_binary_switches(golden_dir):
    """The two modes are different functions: rows of the gltfpbr and rough-glass tables (sinf / cosf / atanf / powf) differ between them,
    the delta glass lobe (no transcendental) has none that do."""
    g = np.load(os.path.join(golden_dir, "ref_bxdf.npz"))
    assert g["glibc_idx_0"].size > 20 and g["glibc_idx_2"].size > 20 and g["glibc_idx_3"].size == 0


@pytest.mark.parametrize("name", list(SCENES))
def test_raycast_equals_the_references(golden_dir, libm, name):
    """RayCast with its order-dependent box cull: the 4,096 scene rays and the 1,024 long segments (|1/dir| < 1, where the cull drops hits
    depending on the traversal order), every HIT record."""
    g = np.load(os.path.join(golden_dir, "ref_raycast.npz"))
    rays8 = np.load(os.path.join(golden_dir, f"oracle_{name}.npz"))["rays8"]
    sc = O.Scene(*world(name))
    for mode in (0, 1):
        libm(mode)
        for what, rays, want in (("scene rays", rays8, g[f"hits_{name}"]), ("long segments", g["long_rays8"], g[f"long_hits_{name}"])):
            bad = differing_rows(sc.raycast(rays)[0], want)
            assert bad.size == 0, f"{name}, {what}: {bad.size} HIT records differ from the reference, first {bad[:8]}"
    assert (g[f"hits_{name}"][:, 0] > 0).sum() > 3000
    if name != "cornell":       # the room alone is empty: no segment inside it hits
        assert (g[f"long_hits_{name}"][:, 0] > 0).sum() > 50


def test_nee_equals_the_references(golden_dir, libm):
    g = np.load(os.path.join(golden_dir, "ref_nee.npz"))
    cols = g["cols"]
    assert list(cols) == O.NEE_REF_COLS
    sc = O.Scene(*world("standin24_spheres"))
    lit = g["out12"][:, 8:11].sum(1) > 0
    assert lit.sum() > 500 and (~lit).sum() > 500
    for mode in (0, 1):
        libm(mode)
        bad = differing_rows(sc.nee(g["in5"])[:, cols], g["out12"][:, cols])
        assert bad.size == 0, f"{bad.size} NEE rows differ from the reference, first {bad[:8]}"


def test_spheres_image_at_bounce_8_equals_the_references(golden_dir, libm):
    """All four lobes in one frame (64 x 64, 2 passes x 8 spp, the reference's MAX_BOUNCE 8, contract libm): o_render against the image
    the reference's GetColor_iter produced."""
    g = np.load(os.path.join(golden_dir, "ref_image_standin24_spheres_b8.npz"))
    nodes, tris, _ = world("standin24_spheres")
    libm(1)
    img, _ = O.Scene(nodes, tris, g["spheres"]).render(O.make_camera(64, 64), O.make_params(64, 64, int(g["passes"]), int(g["spp"]), int(g["max_bounce"])), 8)
    bad = differing_rows(img.reshape(-1, 3), g["image"].reshape(-1, 3))
    assert bad.size == 0, f"{bad.size} pixels differ from the reference's, first {bad[:8]}"
    assert np.isfinite(g["image"]).all() and g["image"].mean() > 0.1


# ---------------------------------------------------------------------------------------------------------------------------------
# live: the binary itself
# ---------------------------------------------------------------------------------------------------------------------------------
@live
def test_live_rng_is_the_rng_contract(golden_dir):
    """oracle/curand_shim.h against rocRAND's own XORWOW engine (tests/golden/ref_rocrand_xorwow.npz), every seed stored there."""
    g = np.load(os.path.join(golden_dir, "ref_rocrand_xorwow.npz"))
    for seed, raw, uni in zip(g["seeds"], g["raw"], g["uniform"]):
        r, u = O.ref_int_rng(int(seed), raw.shape[0])
        assert np.array_equal(r, raw) and np.array_equal(bits(u), bits(uni)), int(seed)


@live
def test_live_fixtures_are_what_the_binary_says(golden_dir):
    """The committed tables regenerate from the binary: one lobe table per libm mode, one ray table, the NEE table."""
    for lobe, mode in ((0, 0), (2, 1), (3, 0), (1, 1)):
        in28, contract, glibc, _ = load_ref_bxdf(golden_dir, lobe)
        assert differing_rows(O.ref_int_bxdf(lobe, in28, mode), contract if mode else glibc).size == 0, (lobe, mode)
    g = np.load(os.path.join(golden_dir, "ref_raycast.npz"))
    nodes, tris, sph = world("standin24_spheres")
    assert differing_rows(O.ref_int_raycast(nodes, tris, sph, g["long_rays8"]), g["long_hits_standin24_spheres"]).size == 0
    n = np.load(os.path.join(golden_dir, "ref_nee.npz"))
    assert differing_rows(O.ref_int_nee(nodes, tris, sph, n["in5"]), n["out12"]).size == 0


@live
def test_live_fresh_tables_against_the_oracle(libm):
    """Fresh seeded inputs, not the committed ones: BxDF rows per lobe and mode, NEE rows."""
    from scenes_util import bxdf_inputs
    rs = np.random.RandomState(2024)
    for lobe in range(4):
        a, seeds = bxdf_inputs(3000, rs, lobe)
        in28 = np.concatenate([a, seeds, np.zeros((a.shape[0], 2), np.float32)], 1)
        for mode in (0, 1):
            libm(mode)
            bad = differing_rows(O.bxdf(lobe, in28), O.ref_int_bxdf(lobe, in28, mode))
            assert bad.size == 0, (lobe, mode, bad[:8])


@live
@pytest.mark.parametrize("name", ["cornell", "standin24", "standin24_spheres"])
def test_live_paths_reproduce_the_committed_images(golden_dir, name):
    """GetColor_iter, path by path, in contract mode: oracle_cornell.npz and oracle_standin24.npz were rendered at max_bounce 8, so the
    reference must give their `image` arrays; the spheres frame at bounce 8 is the reference's own fixture."""
    file = "ref_image_standin24_spheres_b8.npz" if name == "standin24_spheres" else f"oracle_{name}.npz"
    g = np.load(os.path.join(golden_dir, file))
    assert int(g["max_bounce"]) == 8
    nodes, tris, sph = world(name)
    img = O.ref_int_render(nodes, tris, sph, O.make_camera(64, 64), int(g["passes"]), int(g["spp"]), 1)
    bad = differing_rows(img.reshape(-1, 3), g["image"].reshape(-1, 3))
    assert bad.size == 0, f"{name}: {bad.size} pixels differ, first {bad[:8]}"


@live
def test_live_cornell_anchor_in_glibc_mode(golden_dir):
    """anchors.json, Cornell 256 x 256, 1 x 16 spp: the reference's own integrator with glibc's float libm gives the survey's mean to all
    six printed digits — and the oracle's frame in mode 0, pixel for pixel."""
    a = json.load(open(os.path.join(golden_dir, "anchors.json")))
    nodes, tris, _ = world("cornell")
    cam = O.make_camera(256, 256)
    img = O.ref_int_render(nodes, tris, None, cam, 1, 16, 0, nproc=16)
    assert f"{float(img.mean(dtype=np.float64)):.6f}" == f"{a['cornell_256x256_1x16']:.6f}"
    old = O.set_libm(0)
    try:
        ref, _ = O.Scene(nodes, tris).render(cam, O.make_params(256, 256, 1, 16), 16)
    finally:
        O.set_libm(old)
    assert differing_rows(img.reshape(-1, 3), ref.reshape(-1, 3)).size == 0


@live
@pytest.mark.parametrize("key,kind", [("standin1_320x180_1x4", 1), ("standin4_320x180_1x4", 2)])
def test_live_standin_anchors_in_glibc_mode(golden_dir, key, kind):
    a = json.load(open(os.path.join(golden_dir, "anchors.json")))
    nodes, tris, _ = O.bvh_build(ptamd.gen_scene(kind, 187))
    img = O.ref_int_render(nodes, tris, None, O.make_camera(320, 180), 1, 4, 0, nproc=16)
    assert f"{float(img.mean(dtype=np.float64)):.6f}" == f"{a[key]:.6f}"


@live
def test_live_acesfilm():
    """ACESFilm (CudaUtil.cuh:383-391) on 4,096 values — 0, negatives, above 1, NaN, inf among them: through ConverToUint8 against
    o_tonemap (sample count 1), and as floats against the same expression in IEEE float32."""
    rs = np.random.RandomState(8)
    x = np.concatenate([rs.uniform(0, 1, 2000), 10.0 ** rs.uniform(-6, 4, 1500), -(10.0 ** rs.uniform(-6, 2, 584))]).astype(np.float32)
    x = np.concatenate([x, np.float32([0.0, -0.0, 1.0, 2.0, 1e30, np.nan, np.inf, -np.inf, -0.14 / 0.59, 1e-45, 3.4e38, -1.0])])
    assert x.size == 4096
    x = np.concatenate([x, np.float32([0.5, 0.25])]).reshape(-1, 3)      # ACESFilm takes a Color: pad to whole triples
    got = O.ref_int_aces(x)
    assert np.array_equal(bits(got), bits(O.aces(x)))
    assert ((got >= 0) & (got <= 1)).all()
    assert np.array_equal(O.u8(got), O.tonemap(x, 1))


@live
def test_live_raycast_big_tree(libm):
    """RayCast on the deep tree of kind 1 at lat_lon 187 (69,576 triangles): 20,000 scene rays against the oracle."""
    nodes, tris, _ = O.bvh_build(ptamd.gen_scene(1, 187))
    rays = scene_rays8(20000, np.random.RandomState(77))
    libm(1)
    hits, prim, _ = O.Scene(nodes, tris).raycast(rays)
    bad = differing_rows(hits, O.ref_int_raycast(nodes, tris, None, rays))
    assert bad.size == 0 and (prim >= 0).mean() > 0.7, bad[:8]
