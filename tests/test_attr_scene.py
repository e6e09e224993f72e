"""Parity on scenes_util.attribute_scene: a mesh with per-vertex frames and per-vertex materials, delta-glass, rough-glass and mirror
triangles, eight lights of very different areas (one of them emissive on its second vertex only), exact duplicates (ties in t), slivers
and zero-area triangles, with the three test spheres.  The three scenes of pt_scene_gen have flat frames, equal vertex materials,
opaque triangles and one lamp, so a swapped barycentric weight, a wrong vertex's material or a wrong per-light pdf changes no bit there.

On the CPU the fixture tests/golden/ref_attr.npz (written by the REAL reference's integrator, oracle/_ref/ptref_int in contract mode:
oracle/gen_golden.py gen_attr) is tied to the generator, to the oracle and, where it was built, to the binary; a census from the oracle
alone keeps the GPU tests from passing vacuously.  On the GPU every entry point that traces or shades is held against the fixture and
the oracle: bits everywhere, and for frames the bars of tests/test_gpu_reference.py and tests/test_gpu_parity.py, unchanged.

What the oracle alone says (seed 7, lat_lon 12, 354 triangles + 3 spheres, 2,000 rays per set; printed by test_census_*):
  hit share per set: scene 0.7980 (196 sphere hits), aimed 0.9910 (214), leaving 0.6935 (232), axis 0.9345 (252);
  5,940 triangle hits, 297 of them with a front-facing geometric and a back-facing interpolated normal;
  per lobe of the HIT record's material: gltfpbr 4,170, reflective 271, refractive 861, pure_refractive 638;
  2,981 hits on triangles whose mat1 opacity differs from mat0's, 679 of them on the opaque ones with a transparent vertex 1;
  152 hits on slivers, none on a zero-area triangle; 346 rays on which a duplicated pair ties exactly at the closest hit, the larger
  reference index recorded on every one; 1,628 axis rays with an origin coordinate on a leaf box face, 555 on a wall's plane;
  NEE: 2,048 rows, draws per light index 243 272 262 231 258 261 249 272, lit share 0.3770 (lit rows per light index 110 25 0 9 147
  179 165 137), 262 rows on the mat0-dark light (index 2 of the light list), none of them lit.
On an MI355X (printed by the GPU tests): 0 differing HIT records, NEE rows and AOV floats; the any-hit query returned the closest hit in
0.7055 (scene), 0.5545 (aimed), 0.8298 (leaving) and 0.5538 (axis) of the hits; the 64 x 64 frame has relRMS 0 and 1.000000 bit-identical
pixels against the reference and against the oracle under both tails, shade rounds 0 and 1 and mode 0, as have the 100 x 52 frame and the
frames after the vertex update (modes 1 and 0).  The scene has a core box at lat_lon 12: (-13.47918, -0.2469803, -10.237181) ..
(14.279181, 26.266981, 13.237181), so no second lat_lon is needed.  What these tests found when first run: pt_dbg_raycast and the surface
pass of pt_trace_rays wrote 0 for HitResult::u / v (492 of 2,000 `scene` records differed from the reference, all in floats 2 and 3);
scenes now keep the vertex u, v on the device (csrc/pt_shade.h: hit_uv).  With mat1 for mat0 in pack_surfaces, or u and v swapped in
surf_from_rec, on a scratch build: the closest-hit, AOV and image tests fail (and the NEE test with the former).
"""
import os
import re
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest

import dynamic_ref as R
import oracle_lib as O
import ptamd
from scenes_util import ATTR_RAY_SETS, attr_tri_to_input, load_ref_attr, rel_rms

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "pathtrace-on-cuda_amd")
live = pytest.mark.skipif(not O.have_ref_int(), reason="oracle/_ref/ptref_int not built (reference tree absent)")
REL_RMS_TOL = 1e-4          # BASELINE.json north_star: the bar of tests/test_gpu_reference.py and tests/test_gpu_parity.py
LOBES = ("gltfpbr", "reflective", "refractive", "pure_refractive")
M_OPACITY, M_ROUGHNESS = 26, 27      # in a HIT record: MAT starts at 17


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_bits_or_nan(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return (bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))


def differing_rows(a, b):
    same = same_bits_or_nan(a, b)
    return np.nonzero(~same.reshape(same.shape[0], -1).all(1))[0]


def lobe_of(opacity, roughness):
    """csrc/pt_bxdf.h: lobe_of (CudaUtil.cuh:221-229) on arrays: 0 gltfpbr, 1 reflective, 2 refractive, 3 pure_refractive."""
    glass = opacity < np.float32(1.0) - np.float32(1e-4)
    smooth = roughness < np.float32(1e-2)
    return np.where(glass, np.where(smooth, 3, 2), np.where(smooth, 1, 0))


_A = {}


def attr(golden_dir):
    """The fixture, the regenerated scene and rays, both BVHs' common arrays, the oracle's scene and its answers (contract mode)."""
    if not _A:
        g, prims, groups, rays, in5 = load_ref_attr(golden_dir)
        nodes, tris, depth = ptamd.build_bvh(prims)
        old = O.set_libm(1)
        try:
            so = O.Scene(nodes.tobytes(), tris, g["spheres"])
            cast = {name: so.raycast(rays[name])[:2] for name in ATTR_RAY_SETS}
            nee = so.nee(in5)
        finally:
            O.set_libm(old)
        to_input = attr_tri_to_input(prims, tris)
        group_of = {name: np.isin(to_input, groups[name]) for name in groups if name != "dup_of"}
        _A["a"] = SimpleNamespace(g=g, prims=prims, groups=groups, rays=rays, in5=in5, nodes=nodes, tris=tris, depth=depth, sph=g["spheres"], so=so,
                                  cast=cast, nee=nee, to_input=to_input, group_of=group_of, light_tris=np.nonzero(R.emissive(tris))[0])
    return _A["a"]


# ---------------------------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------------------------
def test_generator_is_deterministic_and_is_the_recipe(golden_dir):
    a = attr(golden_dir)      # load_ref_attr holds the sha256 of the scene, of every ray set and of the NEE rows against the fixture
    from scenes_util import V_ALB, V_EMIT, V_NRM, V_OPA, V_ROU, attribute_scene
    again, _ = attribute_scene(int(a.g["seed"]), int(a.g["lat_lon"]))
    assert np.array_equal(bits(again), bits(a.prims))
    other, _ = attribute_scene(int(a.g["seed"]) + 1, int(a.g["lat_lon"]))
    assert not np.array_equal(bits(other), bits(a.prims))
    gr, p = a.groups, a.prims.reshape(-1, 3, 28)
    assert {k: len(gr[k]) for k in ("walls", "mesh", "dups", "slivers", "zero", "lights")} == dict(walls=10, mesh=264, dups=40, slivers=30, zero=2, lights=8)
    assert len(a.prims) == 354
    # the walls are pt_scene_gen(0)'s, the mesh is pt_scene_gen(1, 12)'s to a few ulps (float64 sines here, sinf there)
    assert np.array_equal(bits(a.prims[gr["walls"]]), bits(ptamd.gen_scene(0)[:10]))
    mesh_ref = ptamd.gen_scene(1, 12)[12:].reshape(-1, 3, 28)
    assert np.abs(p[gr["mesh"], :, 0:3] - mesh_ref[:, :, 0:3]).max() < 1e-4
    # lights are spread through the list, not one block
    assert (np.diff(gr["lights"]) > 30).all()
    e = np.sqrt((p[:, :, V_EMIT:V_EMIT + 3].astype(np.float64) ** 2).sum(-1))
    assert np.array_equal(np.nonzero((e > 1e-4).any(1))[0], gr["lights"])
    dark = gr["dark_light"][0]
    assert e[dark, 0] == 0 and e[dark, 1] > 1 and e[dark, 2] == 0
    lp = p[gr["lights"], :, 0:3].astype(np.float64)
    cr = np.cross(lp[:, 1] - lp[:, 0], lp[:, 2] - lp[:, 0])
    area = 0.5 * np.sqrt((cr * cr).sum(1))
    assert area[:7].max() / area[:7].min() >= 100 and (cr[:, 1] > 0).sum() >= 1 and area.min() < 0.01
    assert len({tuple(x) for x in p[gr["lights"][:7], 0, V_EMIT:V_EMIT + 3]}) == 7
    # per-vertex attributes: the three normals and the three materials of a mesh triangle differ
    m = p[gr["mesh"]]
    assert (np.abs(m[:, 0, V_NRM:V_NRM + 3] - m[:, 1, V_NRM:V_NRM + 3]).max(1) > 1e-3).all()
    assert (m[:, 0, V_ALB] != m[:, 1, V_ALB]).all() and (m[:, 1, V_ALB] != m[:, 2, V_ALB]).all()
    ln = np.sqrt((m[:, :, V_NRM:V_NRM + 3].astype(np.float64) ** 2).sum(-1))
    assert 0.1 < (ln > 1.5).all(1).mean() < 0.3 and ((ln > 1.5).all(1) | (ln < 1.5).all(1)).all()
    for name, lo in (("delta_glass", 0.15), ("rough_glass", 0.15), ("v1_opacity", 0.15), ("mirror", 0.05)):
        assert len(gr["mesh_" + name]) >= lo * len(gr["mesh"]), name
    v1 = p[gr["mesh_v1_opacity"]]
    assert (v1[:, 0, V_OPA] == 1).all() and (v1[:, 1, V_OPA] == 0).all() and (v1[:, 2, V_OPA] == 1).all()
    assert (p[gr["mesh_delta_glass"], 0, V_OPA] == 0).all() and (p[gr["mesh_delta_glass"], 0, V_ROU] == 0).all()
    assert (p[gr["mesh_mirror"], 0, V_OPA] == 1).all() and (p[gr["mesh_mirror"], 0, V_ROU] < 1e-2).all()
    # duplicates: the same 81 floats but for the albedo
    d, o = p[gr["dups"]].copy(), p[gr["dup_of"]].copy()
    assert not np.array_equal(d[:, :, V_ALB:V_ALB + 3], o[:, :, V_ALB:V_ALB + 3])
    d[:, :, V_ALB:V_ALB + 3] = o[:, :, V_ALB:V_ALB + 3] = 0
    assert np.array_equal(bits(d), bits(o))
    # slivers: aspect about 1e4; zero-area triangles: area 0 exactly, NaN flat normal
    s = p[gr["slivers"], :, 0:3].astype(np.float64)
    long_edge = np.max([np.sqrt(((s[:, i] - s[:, j]) ** 2).sum(1)) for i, j in ((1, 0), (2, 1), (0, 2))], 0)
    sc = np.cross(s[:, 1] - s[:, 0], s[:, 2] - s[:, 0])
    height = np.sqrt((sc * sc).sum(1)) / long_edge
    assert ((long_edge / height > 5e3) & (long_edge / height < 2e4)).all()
    zt = a.tris[a.group_of["zero"]]
    assert len(zt) == 2 and (zt[:, R.T_AREA] == 0).all() and np.isnan(zt[:, R.T_NORMAL:R.T_NORMAL + 3]).all()
    # every direction has its components in [-1, 1] (LONG_DIRECTIONS in tests/test_query.py): the reference's answer is the contract's
    for name in ATTR_RAY_SETS:
        r = a.rays[name]
        assert r.shape == (int(a.g["n_rays"]), 8) and r.dtype == np.float32 and np.isfinite(r).all() and (np.abs(r[:, 3:6]) <= 1).all(), name
        assert (r[:, 6] == 0).all()
    ax = a.rays["axis"][:, 3:6]
    assert ((ax != 0).sum(1) == 1).all() and (np.abs(ax).sum(1) == 1).all()
    assert int(a.g["n_rays"]) >= 2000 and len(a.in5) >= 2000
    assert os.path.getsize(os.path.join(golden_dir, "ref_attr.npz")) < os.path.getsize(os.path.join(golden_dir, "ref_bvh_grid5000.npz"))


def test_product_bvh_is_the_oracles(golden_dir):
    a = attr(golden_dir)
    nodes, tris, depth = O.bvh_build(a.prims)
    assert nodes.tobytes() == a.nodes.tobytes() and depth == a.depth
    assert same_bits_or_nan(tris, a.tris).all() and tris.shape == (354, 88)
    assert np.array_equal(np.sort(a.to_input), np.arange(354))
    if O.have_ref():
        rn, rt = O.ref_bvh(a.prims)
        assert rn.tobytes() == a.nodes.tobytes() and same_bits_or_nan(rt, a.tris).all()


def test_oracle_equals_the_fixture_on_every_row_and_pixel(golden_dir):
    a = attr(golden_dir)
    for name in ATTR_RAY_SETS:
        bad = differing_rows(a.cast[name][0], a.g[f"hits_{name}"])
        assert bad.size == 0, f"{name}: {bad.size} HIT records differ from the reference, first {bad[:8]}"
        assert np.array_equal(a.cast[name][1] >= 0, a.g[f"hits_{name}"][:, 0] > 0)
    cols = a.g["nee_cols"]
    assert list(cols) == O.NEE_REF_COLS
    bad = differing_rows(a.nee[:, cols], a.g["nee_out12"][:, cols])
    assert bad.size == 0, f"{bad.size} NEE rows differ from the reference, first {bad[:8]}"
    old = O.set_libm(1)
    try:
        img, _ = a.so.render(O.make_camera(64, 64), O.make_params(64, 64, int(a.g["passes"]), int(a.g["spp"]), int(a.g["max_bounce"])), 8)
    finally:
        O.set_libm(old)
    bad = differing_rows(img.reshape(-1, 3), a.g["image"].reshape(-1, 3))
    assert bad.size == 0, f"{bad.size} pixels differ from the reference's, first {bad[:8]}"
    assert np.isfinite(a.g["image"]).all() and a.g["image"].mean() > 0.1


@live
def test_live_binary_regenerates_the_fixture(golden_dir):
    a = attr(golden_dir)
    nodes, tris = a.nodes.tobytes(), a.tris
    nodes = np.frombuffer(nodes, np.uint8)
    for name in ATTR_RAY_SETS:
        assert differing_rows(O.ref_int_raycast(nodes, tris, a.sph, a.rays[name]), a.g[f"hits_{name}"]).size == 0, name
    assert differing_rows(O.ref_int_nee(nodes, tris, a.sph, a.in5), a.g["nee_out12"]).size == 0
    img = O.ref_int_render(nodes, tris, a.sph, O.make_camera(64, 64), int(a.g["passes"]), int(a.g["spp"]), 1)
    assert differing_rows(img.reshape(-1, 3), a.g["image"].reshape(-1, 3)).size == 0


def test_scene_create_gets_as_far_as_the_device(golden_dir):
    """pt_scene_create's checks of the tree (both depth checks among them) pass: the scene is rejected neither as PT_ERR_INVALID (-1) nor
    as PT_ERR_UNSUPPORTED; without a GPU the call fails at the device (PT_ERR_DEVICE), with one it succeeds."""
    import ctypes as C
    a = attr(golden_dir)
    hdr = open(os.path.join(ROOT, "include", "pt_api.h")).read()
    codes = {k: int(v) for k, v in re.findall(r"^\s*(PT_OK|PT_ERR_INVALID|PT_ERR_UNSUPPORTED|PT_ERR_DEVICE) = (-?\d+)", hdr, re.M)}
    assert set(codes) == {"PT_OK", "PT_ERR_INVALID", "PT_ERR_UNSUPPORTED", "PT_ERR_DEVICE"}, codes
    import torch
    have_gpu = torch.cuda.is_available()
    h = C.c_void_p()
    sph = np.ascontiguousarray(a.sph, np.float32)
    rc = ptamd.lib().pt_scene_create(ptamd._ptr(a.nodes), len(a.nodes), ptamd._ptr(a.tris), len(a.tris), ptamd._ptr(sph), len(sph), 0, C.byref(h))
    if rc == codes["PT_OK"]:
        ptamd.lib().pt_scene_destroy(h)
    assert rc == (codes["PT_OK"] if have_gpu else codes["PT_ERR_DEVICE"]), (rc, ptamd.lib().pt_last_error())


def _tri_hits(a):
    """All four sets in one table: (HIT records, prim, rays) of the rows that hit a triangle."""
    hits = np.concatenate([a.cast[n][0] for n in ATTR_RAY_SETS])
    prim = np.concatenate([a.cast[n][1] for n in ATTR_RAY_SETS])
    rays = np.concatenate([a.rays[n] for n in ATTR_RAY_SETS])
    on = (prim >= 0) & (prim < len(a.tris))
    return hits[on], prim[on], rays[on]


def test_census_of_the_ray_sets(golden_dir):
    """Conditions on the oracle's own answers, so that no GPU test passes vacuously."""
    a = attr(golden_dir)
    for name in ATTR_RAY_SETS:
        prim = a.cast[name][1]
        print(f"{name}: hit share {(prim >= 0).mean():.4f}, sphere hits {(prim >= len(a.tris)).sum()}")
        assert 0.5 < (prim >= 0).mean() < 0.999, name
    hits, prim, rays = _tri_hits(a)
    t = a.tris[prim]
    # Triangle::hit culls back faces, so the geometric normal faces every ray that hits; the interpolated one need not
    geo_front = (rays[:, 3:6].astype(np.float64) * t[:, R.T_NORMAL:R.T_NORMAL + 3]).sum(1) < 0
    away = geo_front & (hits[:, 4] == 0)
    print(f"triangle hits {len(hits)}; front-facing geometric normal with a back-facing interpolated normal: {away.sum()}")
    assert geo_front.all() and away.sum() >= 50
    lobes = lobe_of(hits[:, M_OPACITY], hits[:, M_ROUGHNESS])
    counts = [int((lobes == k).sum()) for k in range(4)]
    print("triangle hits per lobe of the HIT record's material:", dict(zip(LOBES, counts)))
    assert min(counts) >= 100, counts
    m0, m1 = t[:, R.T_MAT0 + 9], t[:, R.T_MAT0 + 12 + 9]
    v1 = a.group_of["mesh_v1_opacity"][prim]
    print(f"hits on triangles whose mat1 opacity differs from mat0's: {(m0 != m1).sum()}, of them opaque with a transparent vertex 1: {v1.sum()}")
    assert (m0 != m1).sum() >= 50 and v1.sum() >= 50
    assert (hits[v1, M_OPACITY] == 1).all()      # mat0 decides
    sl = a.group_of["slivers"][prim]
    print(f"hits on slivers: {sl.sum()}")
    assert sl.sum() >= 20
    assert not a.group_of["zero"][prim].any()      # a zero-area triangle is never hit


def test_census_of_the_ties(golden_dir):
    """Rays of the `aimed` set on which both triangles of a duplicated pair pass Triangle::hit with the same t, that t being the closest
    hit's: the record is that of the larger reference index."""
    a = attr(golden_dir)
    ref_of = np.full(len(a.prims), -1)
    ref_of[a.to_input] = np.arange(len(a.tris))
    pairs = np.stack([ref_of[a.groups["dups"]], ref_of[a.groups["dup_of"]]], 1)
    tris48 = np.concatenate([a.tris[:, 0:9], a.tris[:, R.T_N:R.T_N + 9], a.tris[:, R.T_T:R.T_T + 9], a.tris[:, R.T_B:R.T_B + 9],
                             a.tris[:, R.T_MAT0:R.T_MAT0 + 12]], 1)
    rays = a.rays["aimed"]
    hits, prim = a.cast["aimed"]
    n = len(rays)
    decisive = 0
    for lo, hi in np.sort(pairs, 1):
        rows = []
        for k in (lo, hi):
            r10 = np.concatenate([np.full((n, 1), k, np.float32), rays[:, 0:6], rays[:, 6:8], np.zeros((n, 1), np.float32)], 1)
            rows.append(O.tri_hit(tris48, r10))
        tie = (rows[0][:, 0] > 0) & (rows[1][:, 0] > 0) & (bits(rows[0][:, 1]) == bits(rows[1][:, 1])) & (bits(hits[:, 1]) == bits(rows[0][:, 1])) & (hits[:, 0] > 0)
        tie &= np.isin(prim, (lo, hi))
        assert (prim[tie] == hi).all(), (lo, hi, prim[tie])
        assert np.array_equal(bits(hits[tie, 20:23]), bits(np.broadcast_to(a.tris[hi, R.T_MAT0 + 3:R.T_MAT0 + 6], (int(tie.sum()), 3))))
        assert not np.array_equal(a.tris[lo, R.T_MAT0 + 3:R.T_MAT0 + 6], a.tris[hi, R.T_MAT0 + 3:R.T_MAT0 + 6])
        decisive += int(tie.sum())
    print(f"rays on which a duplicated pair ties exactly at the closest hit: {decisive}")
    assert decisive >= 20


def test_census_of_the_axis_rays(golden_dir):
    """Axis-aligned rays whose origin lies in the plane of a face of a reference leaf box, or of a wall."""
    a = attr(golden_dir)
    leaf = R.is_leaf(a.nodes)
    r = a.rays["axis"]
    ax = np.argmax(np.abs(r[:, 3:6]), 1)
    on_leaf = np.zeros(len(r), bool)
    on_wall = np.zeros(len(r), bool)
    for k in range(3):
        faces = np.unique(np.concatenate([a.nodes["bMin"][leaf, k], a.nodes["bMax"][leaf, k]]))
        on_leaf |= np.isin(r[:, k], faces) & (ax != k)
        on_wall |= np.isin(r[:, k], np.float32([-20, 20] if k != 1 else [0, 40]))
    print(f"axis rays with an origin coordinate on a leaf box face: {on_leaf.sum()}, on a wall's plane: {on_wall.sum()}")
    assert on_leaf.sum() >= 500 and on_wall.sum() >= 200


def test_census_of_the_nee_table(golden_dir):
    a = attr(golden_dir)
    assert a.so.num_lights == 8 and len(a.light_tris) == 8
    idx = a.nee[:, 0].view(np.int32)
    counts = np.bincount(idx, minlength=8)
    lit = a.nee[:, 8:11].sum(1) > 0
    dark_index = int(np.nonzero(a.group_of["dark_light"][a.light_tris])[0][0])
    print(f"NEE rows {len(idx)}; draws per light index {counts.tolist()}; lit share {lit.mean():.4f}; rows on the mat0-dark light (index {dark_index}): {counts[dark_index]}")
    print("lit rows per light index", np.bincount(idx[lit], minlength=8).tolist())
    assert len(counts) == 8 and counts.min() >= 100
    assert lit.mean() >= 0.25 and (~lit).mean() >= 0.25
    assert counts[dark_index] >= 20 and not lit[idx == dark_index].any()
    # the light list is in reference order, not in input order, and the areas differ by more than 100 x
    area = a.tris[a.light_tris, R.T_AREA]
    assert area.max() / area.min() > 100
    assert (np.bincount(idx[lit], minlength=8) > 0).sum() >= 6      # light from most lamps arrives somewhere


# ---------------------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def _gpu():
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    old = O.set_libm(1)      # the pinned contract: correctly rounded float transcendentals
    yield
    O.set_libm(old)


def _scene(a):
    return ptamd.Scene(a.nodes, a.tris, a.sph)


def _assert_closest(got, want_hits, prim_o, what):
    """(t, prim, surface) of a closest-hit query: the reference's HIT records, the oracle's primitive."""
    t, prim, surf = got
    bad = differing_rows(surf, want_hits)
    assert bad.size == 0, f"{what}: {bad.size} HIT records differ from the reference, first {bad[:8]}"
    assert np.array_equal(prim, prim_o), f"{what}: {(prim != prim_o).sum()} prims differ, first at {np.nonzero(prim != prim_o)[0][:5]}"
    assert np.array_equal(bits(t), bits(want_hits[:, 1])), what
    miss = want_hits[:, 0] == 0
    assert (t[miss] == 0).all() and (prim[miss] == -1).all() and (surf[miss] == 0).all(), what


def _assert_any(any_t, any_prim, closest_t, closest_prim, rays, n_prims, what):
    """tests/test_query.py: _assert_any."""
    hit = closest_prim >= 0
    assert np.array_equal(any_prim >= 0, hit), f"{what}: {((any_prim >= 0) != hit).sum()} rays decide differently from the closest-hit query"
    assert (any_prim[~hit] == -1).all() and (any_t[~hit] == 0).all(), what
    assert (any_prim < n_prims).all(), what
    assert (any_t[hit] <= rays[hit, 7]).all() and (any_t[hit] >= 0).all(), what
    assert (any_t[hit] >= closest_t[hit]).all(), what


@pytest.mark.gpu
@pytest.mark.parametrize("name", ATTR_RAY_SETS)
def test_closest_hit_is_the_references(_gpu, golden_dir, name):
    """pt_dbg_raycast and pt_trace_rays (closest, with the 29-float surface record) against the reference's HIT records: every bit, NaN
    equal to NaN; the primitive is the oracle's (the tie rule)."""
    a = attr(golden_dir)
    sc = _scene(a)
    rays, want, prim_o = a.rays[name], a.g[f"hits_{name}"], a.cast[name][1]
    hits_d, prim_d = sc.raycast(rays)
    bad = differing_rows(hits_d, want)
    assert bad.size == 0, f"{name}, pt_dbg_raycast: {bad.size} HIT records differ from the reference, first {bad[:8]}"
    assert np.array_equal(prim_d, prim_o)
    _assert_closest(sc.trace_rays(rays, surface=True), want, prim_o, f"{name}, pt_trace_rays")
    t, prim = sc.trace_rays(rays)
    assert np.array_equal(prim, prim_o) and np.array_equal(bits(t), bits(want[:, 1]))


CHILD = r"""
import sys
import numpy as np
import ptamd
from scenes_util import ATTR_RAY_SETS, load_ref_attr
g, prims, groups, rays, in5 = load_ref_attr(sys.argv[1])
nodes, tris, _ = ptamd.build_bvh(prims)
sc = ptamd.Scene(nodes, tris, g["spheres"])
allrays = np.concatenate([rays[n] for n in ATTR_RAY_SETS])
t, prim, surf = sc.trace_rays(allrays, surface=True)
at, aprim = sc.trace_rays(allrays, any_hit=True)
np.savez(sys.argv[2], t=t, prim=prim, surf=surf, at=at, aprim=aprim)
"""


@pytest.mark.gpu
def test_binary_tree_fallback_is_the_references(_gpu, golden_dir, tmp_path):
    """The binary-tree walk of the query kernels, forced by PTAMD_QUERY_QUAD=0 in a fresh process (read when a scene is created)."""
    a = attr(golden_dir)
    out = str(tmp_path / "child.npz")
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([PKG, os.path.join(ROOT, "tests"), os.environ.get("PYTHONPATH", "")]), PTAMD_QUERY_QUAD="0")
    subprocess.run([sys.executable, "-c", CHILD, golden_dir, out], check=True, env=env, timeout=600)
    c = np.load(out)
    rays = np.concatenate([a.rays[n] for n in ATTR_RAY_SETS])
    want = np.concatenate([a.g[f"hits_{n}"] for n in ATTR_RAY_SETS])
    prim_o = np.concatenate([a.cast[n][1] for n in ATTR_RAY_SETS])
    _assert_closest((c["t"], c["prim"], c["surf"]), want, prim_o, "PTAMD_QUERY_QUAD=0")
    _assert_any(c["at"], c["aprim"], c["t"], c["prim"], rays, len(a.tris) + len(a.sph), "PTAMD_QUERY_QUAD=0")


@pytest.mark.gpu
@pytest.mark.parametrize("name", ATTR_RAY_SETS)
def test_any_hit_decides_as_the_closest_hit_does(_gpu, golden_dir, name):
    a = attr(golden_dir)
    sc = _scene(a)
    rays, want, prim_o = a.rays[name], a.g[f"hits_{name}"], a.cast[name][1]
    at, aprim = sc.trace_rays(rays, any_hit=True)
    print(f"{name}: any-hit returned the closest in {(aprim == prim_o)[prim_o >= 0].mean():.4f} of the hits")
    _assert_any(at, aprim, want[:, 1], prim_o, rays, len(a.tris) + len(a.sph), name)
    # the same with tmax cut to just before and just behind the closest hit: a tie must not be lost, a culled twin must not be found
    hit = prim_o >= 0
    for scale, expect in ((np.float32(0.999), False), (np.float32(1.001), True)):
        cut = rays[hit].copy()
        cut[:, 7] = want[hit, 1] * scale
        ct, cprim = sc.trace_rays(cut)
        ct2, cprim2 = sc.trace_rays(cut, any_hit=True)
        _assert_any(ct2, cprim2, ct, cprim, cut, len(a.tris) + len(a.sph), f"{name}, tmax = {scale} t")
        if expect:
            assert (cprim >= 0).all()
        else:      # the closest primitive lies behind tmax now (and so does its twin): whatever is found is another one
            assert (cprim != prim_o[hit])[want[hit, 1] > 0].all()


@pytest.mark.gpu
def test_nee_table_is_the_references(_gpu, golden_dir):
    a = attr(golden_dir)
    got = _scene(a).nee(a.in5)
    cols = a.g["nee_cols"]
    bad = differing_rows(got[:, cols], a.g["nee_out12"][:, cols])
    assert bad.size == 0, f"{bad.size} NEE rows differ from the reference (light index, point, pdf, light colour, next draw), first {bad[:8]}"
    bad = differing_rows(got, a.nee)
    assert bad.size == 0, f"{bad.size} NEE rows differ from the oracle (cosA, tmax, shadow ray's primitive), first {bad[:8]}"


@pytest.mark.gpu
def test_aov_is_the_oracles_first_hits(_gpu, golden_dir):
    """Albedo is mat0's, the normal is the interpolated one turned towards the ray (tests/test_denoise.py's yardstick)."""
    import denoise_ref as D
    a = attr(golden_dir)
    sc = _scene(a)
    for W, H in ((64, 48), (100, 52)):
        got, prim = sc.aov(ptamd.make_camera(W, H), ptamd.default_params(passes=3, first_pass=5))
        want, wprim = D.aov_from_oracle(a.so, O.make_camera(W, H), W, H, 3, 5)
        assert np.array_equal(prim, wprim), (W, H)
        assert same_bits_or_nan(got, want).all(), (W, H, np.argwhere(~same_bits_or_nan(got, want))[:5])
        on_mesh = np.isin(wprim, np.nonzero(a.group_of["mesh"] | a.group_of["dups"])[0])
        assert on_mesh.mean() > 0.05      # the camera sees the mesh


def _check_image(img_g, img_r, what):
    """_check_image of tests/test_gpu_reference.py and tests/test_gpu_parity.py (the two are the same bars)."""
    rr = rel_rms(img_g, img_r)
    same = (bits(img_g) == bits(img_r)).all(-1)
    print(f"{what}: relRMS {rr:.3e}, bit-identical pixels {same.mean():.6f}")
    assert np.isfinite(img_g).all()
    assert rr <= REL_RMS_TOL, f"{what}: relative RMS {rr:.3e} > {REL_RMS_TOL}"
    assert same.mean() >= 0.999, f"{what}: only {same.mean():.5f} of pixels bit-identical"


_ORACLE_FRAMES = {}


def _oracle_frame(a, so, key, W, H, prm, cam=None):
    if key not in _ORACLE_FRAMES:
        ocam = O.make_camera(W, H) if cam is None else O.make_camera(W, H, pos=cam[0], rot=cam[1], fovy_deg=cam[2])
        _ORACLE_FRAMES[key], _ = so.render(ocam, O.make_params(W, H, prm.passes, prm.spp_per_pass, prm.max_bounce, first_pass=prm.first_pass), 16)
    return _ORACLE_FRAMES[key]


@pytest.mark.gpu
@pytest.mark.parametrize("tail", ["tail_in_wf_drain", "pipeline_to_the_end"])
def test_image_is_the_references_and_the_oracles(_gpu, golden_dir, monkeypatch, tail):
    """64 x 64, 2 passes x 8 spp, MAX_BOUNCE 8: the frame of the reference's GetColor_iter (fixture) and the oracle's.  Both render tails
    (PTAMD_DRAIN is read when a scene is created), both shading schedules of the pipeline, and the one-kernel mode 0."""
    if tail == "pipeline_to_the_end":
        monkeypatch.setenv("PTAMD_DRAIN", "0")
    else:
        monkeypatch.delenv("PTAMD_DRAIN", raising=False)
    a = attr(golden_dir)
    g = a.g
    assert int(g["max_bounce"]) == 8
    prm = ptamd.default_params(passes=int(g["passes"]), spp_per_pass=int(g["spp"]), max_bounce=8)
    ref_o = _oracle_frame(a, a.so, "fixture frame", 64, 64, prm)
    sc = _scene(a)
    cam = ptamd.make_camera(64, 64)
    for mode, rounds in ((1, 0), (1, 1), (0, 1)):
        sc.set_mode(mode)
        sc.set_shade_rounds(rounds)
        img = sc.render(cam, prm)
        _check_image(img, g["image"], f"{tail}, mode {mode}, shade rounds {rounds}, against the reference")
        _check_image(img, ref_o, f"{tail}, mode {mode}, shade rounds {rounds}, against the oracle")


CAMERAS = (((0.0, 20.0, 60.0), (0.0, 90.0, 0.0), 45.0), ((3.0, 24.0, 52.0), (0.0, 94.0, 0.0), 40.0))


@pytest.mark.gpu
def test_other_doors_lead_to_the_same_pixels(_gpu, golden_dir):
    """pt_render_window, pt_render_views_host and pt_render_rays_host against pt_render of this scene: bit for bit."""
    a = attr(golden_dir)
    sc = _scene(a)
    W, H = 100, 52
    prm = ptamd.default_params(passes=2, spp_per_pass=4)
    cams = [ptamd.make_camera(W, H, pos=p, rot_deg=r, fovy_deg=f) for p, r, f in CAMERAS]
    frames = [sc.render(c, prm) for c in cams]
    assert not np.array_equal(bits(frames[0]), bits(frames[1]))
    _check_image(frames[0], _oracle_frame(a, a.so, "doors", W, H, prm), "pt_render, 100 x 52")
    for win in ((5, 3, 37, 29), (40, 10, 100, 52), (51, 17, 52, 18)):
        got = sc.render_window(cams[0], prm, win)
        assert same_bits_or_nan(got, frames[0][win[1]:win[3], win[0]:win[2]]).all(), win
    views = sc.render_views(cams, prm)
    for v in range(2):
        assert same_bits_or_nan(views[v], frames[v]).all(), f"view {v}"
    acc = np.zeros((H * W, 3), np.float32)
    for k in range(prm.passes):
        rays, seeds, stride = ptamd.camera_rays(cams[1], k)
        one = ptamd.default_params(passes=1, spp_per_pass=4, first_pass=k)
        got = sc.render_rays(rays, one, seeds, stride)
        assert same_bits_or_nan(got.reshape(H, W, 3), sc.render(cams[1], one)).all(), f"pass {k}"
        acc = acc + got
    assert same_bits_or_nan(acc.reshape(H, W, 3), frames[1]).all()


def _rigid(a, deg=25.0, shift=(2.0, 1.5, -1.0)):
    """The mesh, its duplicates, the zero-area triangles and the two lights in mid-air, rotated by deg about y through the centroid of the moved
    vertices and shifted, in float32; the frames of the moved triangles rotated with them (dynamic_ref.rotate_frames).  Duplicates move
    with their originals, so the ties stay ties."""
    import math
    moved = a.group_of["mesh"] | a.group_of["dups"] | a.group_of["zero"]
    for k in (4, 6):      # the smallest light and the tilted one
        moved = moved | np.isin(a.to_input, a.groups["lights"][k])
    pos = R.positions(a.tris)
    c = pos[moved].reshape(-1, 3).mean(0).astype(np.float32)
    p = pos - c
    cs, sn = np.float32(math.cos(math.radians(deg))), np.float32(math.sin(math.radians(deg)))
    x, y, z = p[..., 0], p[..., 1], p[..., 2]
    rot = np.stack([cs * x + sn * z + np.float32(shift[0]), y + np.float32(shift[1]), -sn * x + cs * z + np.float32(shift[2])], -1).astype(np.float32) + c
    new_pos = np.where(moved[:, None, None], rot, pos).astype(np.float32).reshape(-1, 9)
    old_frames = np.concatenate([a.tris[:, R.T_N:R.T_N + 9], a.tris[:, R.T_T:R.T_T + 9], a.tris[:, R.T_B:R.T_B + 9]], 1)
    with np.errstate(invalid="ignore"):
        frames = np.where(moved[:, None], R.rotate_frames(a.tris, deg), old_frames).astype(np.float32)
    return moved, np.ascontiguousarray(new_pos), np.ascontiguousarray(frames)


@pytest.mark.gpu
def test_vertex_update_with_new_frames_equals_a_fresh_upload(_gpu, golden_dir):
    """A rigid move with new per-vertex frames through pt_scene_update_vertices (device pointers) against pt_scene_create of the moved
    scene as dynamic_ref restates it: every array tests/test_dynamic.py compares, `lights` among them, and the render."""
    import torch
    a = attr(golden_dir)
    moved, new_pos, frames = _rigid(a)
    tris2 = R.restate_tris(a.tris, new_pos, frames)
    nodes2 = R.refit_nodes(a.nodes, tris2)
    sc = _scene(a)
    before = {n: sc.dbg_array(n) for n in ("surf", "lights", "core")}
    refs = (sc.dbg_array("nodes").reshape(-1, 16)[:, 12:16].view(np.uint32).copy(), sc.dbg_array("quad").reshape(-1, 16)[:, 4:8].copy())
    sc.update_vertices(torch.from_numpy(new_pos).cuda(), frames=torch.from_numpy(frames).cuda())
    torch.cuda.synchronize()
    fresh = ptamd.Scene(nodes2, tris2, a.sph)
    got = {n: sc.dbg_array(n) for n in ptamd.SCENE_ARRAYS}
    want = {n: fresh.dbg_array(n) for n in ptamd.SCENE_ARRAYS}
    for n in ("surf", "lights", "leafbox", "spheres"):
        assert got[n].shape == want[n].shape and same_bits_or_nan(got[n], want[n]).all(), (n, np.nonzero(~same_bits_or_nan(got[n], want[n]))[0][:5])
    assert np.array_equal(bits(got["leafbox"].reshape(-1, 8)), bits(R.leaf_boxes(nodes2)))
    tri = got["tri"].reshape(-1, 12)
    prim, leaf = tri[:, 3].view(np.int32), tri[:, 7].view(np.int32)
    assert np.array_equal(np.sort(prim), np.arange(len(tris2)))
    want_tri, want_pair = R.tri_records(tris2, nodes2, prim, leaf)
    assert same_bits_or_nan(got["tri"], want_tri.ravel()).all() and same_bits_or_nan(got["tripair"], want_pair.ravel()).all()
    # the two traversal trees, walked in numpy as tests/test_dynamic.py walks them (_check_trees): every child box the padded exact
    # bounds of the moved triangles below it (binary tree) or a container of them (4-wide tree), every triangle reached exactly once
    # (slivers, zero-area triangles and duplicates included), power-of-two scales, the links as they were at upload
    pos3 = new_pos.reshape(-1, 3, 3)
    bad, seen, _ = R.walk_nodes(got["nodes"], got["tri"], pos3)
    assert not bad, ("nodes: boxes that are not the padded exact bounds", bad[:5])
    assert (seen == 1).all(), "nodes: triangles not reached exactly once"
    qbad, qseen, scales_ok = R.walk_quad(got["quad"], got["tri"], pos3)
    assert not qbad, ("quad: boxes that do not contain the padded bounds", qbad[:5])
    assert (qseen == 1).all() and scales_ok
    assert np.array_equal(got["nodes"].reshape(-1, 16)[:, 12:16].view(np.uint32), refs[0])
    assert np.array_equal(got["quad"].reshape(-1, 16)[:, 4:8], refs[1])
    surf = got["surf"].reshape(-1, 48)
    assert same_bits_or_nan(surf[:, 9:36], frames).all()                   # N0 N1 N2 T0 T1 T2 B0 B1 B2 as given
    assert not same_bits_or_nan(got["surf"], before["surf"]).all() and not np.array_equal(bits(got["lights"]), bits(before["lights"]))
    lights = got["lights"].reshape(-1, 16)
    assert np.array_equal(bits(lights[:, 0:9]), bits(tris2[a.light_tris, 0:9])) and np.array_equal(bits(lights[:, 12]), bits(tris2[a.light_tris, R.T_AREA]))
    print("core box at upload:", before["core"].tolist())
    if before["core"].size:
        assert np.array_equal(got["core"], R.core_box(a.tris, new_pos.reshape(-1, 3, 3)))
    # queries and renders
    so2 = O.Scene(nodes2.tobytes(), tris2, a.sph)
    rays = np.concatenate([a.rays["scene"], a.rays["axis"]])
    hits_o, prim_o, _ = so2.raycast(rays)
    hits_u, prim_u = sc.raycast(rays)
    assert np.array_equal(prim_u, prim_o) and differing_rows(hits_u, hits_o).size == 0
    assert not np.array_equal(prim_o, np.concatenate([a.cast["scene"][1], a.cast["axis"][1]]))      # the move is seen
    in5 = a.in5[:1024]
    assert differing_rows(sc.nee(in5), so2.nee(in5)).size == 0
    W, H = 64, 48
    cam, prm = ptamd.make_camera(W, H), ptamd.default_params(passes=3, spp_per_pass=4)
    ref = _oracle_frame(a, so2, "moved", W, H, prm)
    for mode in (1, 0):
        sc.set_mode(mode)
        fresh.set_mode(mode)
        img = sc.render(cam, prm)
        assert same_bits_or_nan(img, fresh.render(cam, prm)).all(), f"mode {mode}: updated scene against a fresh upload"
        _check_image(img, ref, f"after the move, mode {mode}, against the oracle")


@pytest.mark.gpu
def test_scene_has_a_core_box(_gpu, golden_dir):
    """The queue order by ray class (csrc/pt_scene.hip: core_box) is on for this scene at lat_lon 12, so the image tests above run with
    it; the box is the one dynamic_ref.core_box states."""
    a = attr(golden_dir)
    core = _scene(a).dbg_array("core")
    print("core box:", core.tolist())
    assert core.size == 6
    small = R.core_box(a.tris, R.positions(a.tris))
    assert np.array_equal(core, small)
