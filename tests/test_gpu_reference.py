"""The HIP path against the REAL reference's integrator, on a real MI355X: the tables and images that include/CudaUtil.cuh and
include/Bxdf.cuh themselves produced (oracle/_ref/ptref_int in contract mode: correctly rounded float transcendentals), read from
tests/golden/ only.  The reference tree is not needed here; tests/test_oracle_integrator.py is where the fixtures are tied to the binary.

Where the kernels were written against the CPU oracle, a slip copied from it would pass tests/test_gpu_parity.py; it does not pass here."""
import os

import numpy as np
import pytest

import ptamd
from scenes_util import load_ref_bxdf, rel_rms

pytestmark = pytest.mark.gpu

REL_RMS_TOL = 1e-4          # BASELINE.json north_star, as tests/test_gpu_parity.py
SCENES = {"cornell": (0, False), "standin24": (1, False), "standin24_spheres": (1, True)}


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def differing_rows(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    same = (bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))
    return np.nonzero(~same.reshape(same.shape[0], -1).all(1))[0]


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    yield


def _spheres(golden_dir, name):
    return np.load(os.path.join(golden_dir, "ref_image_standin24_spheres_b8.npz"))["spheres"] if SCENES[name][1] else None


def _scene(golden_dir, name):
    return ptamd.Scene.from_prims(ptamd.gen_scene(SCENES[name][0], 24), _spheres(golden_dir, name))


@pytest.mark.parametrize("lobe", [0, 1, 2, 3])
def test_bxdf_tables_match_the_reference(golden_dir, lobe):
    """pt_dbg_bxdf against the reference's eval_* / sample_* / sample_*_pdf, 2,048 random rows and the hand-built edge block.  The device
    rounds its transcendentals once where the contract rounds through double: at most 2 rows per lobe may differ (the allowance of
    test_bxdf_tables_match_oracle), none of them in the edge block."""
    in28, contract, _, n_random = load_ref_bxdf(golden_dir, lobe)
    bad = differing_rows(ptamd.dbg_bxdf(lobe, in28), contract)
    edge = bad[bad >= n_random]
    assert edge.size == 0, f"lobe {lobe}: edge-block rows {(edge - n_random).tolist()[:20]} differ from the reference ({edge.size} in all)"
    assert bad.size <= 2, f"lobe {lobe}: {bad.size} of {len(contract)} rows differ from the reference, first {bad[:8]}"


@pytest.mark.parametrize("name", list(SCENES))
def test_closest_hit_matches_the_reference(golden_dir, name):
    """pt_dbg_raycast and pt_trace_rays(CLOSEST, surface) against the reference's RayCast.  Rays with |1/dir| >= 1: every bit of the HIT
    record.  Longer directions: the reference's box cull drops hits depending on its traversal order and the device returns the closest
    hit in [0, tmax] (include/pt_api.h), so where the reference has a hit the device has one no farther."""
    g = np.load(os.path.join(golden_dir, "ref_raycast.npz"))
    rays = np.concatenate([np.load(os.path.join(golden_dir, f"oracle_{name}.npz"))["rays8"], g["long_rays8"]])
    want = np.concatenate([g[f"hits_{name}"], g[f"long_hits_{name}"]])
    with np.errstate(divide="ignore"):
        inv = np.float32(1) / rays[:, 3:6]
    unit = np.sqrt((inv.astype(np.float64) ** 2).sum(1)) >= 1.0
    assert unit[:4096].all() and (~unit).sum() > 800
    sc = _scene(golden_dir, name)
    hits_d, _ = sc.raycast(rays)
    t, prim, surf = sc.trace_rays(rays, surface=True)
    for what, got in (("pt_dbg_raycast", hits_d), ("pt_trace_rays", surf)):
        bad = differing_rows(got[unit], want[unit])
        assert bad.size == 0, f"{name}, {what}: {bad.size} HIT records differ from the reference, first {np.nonzero(unit)[0][bad[:8]]}"
        ref_hit = ~unit & (want[:, 0] > 0)
        assert (got[ref_hit, 0] > 0).all() and (got[ref_hit, 1] <= want[ref_hit, 1]).all() and (got[ref_hit, 1] >= 0).all(), f"{name}, {what}: long segments"
    assert np.array_equal(bits(t[unit]), bits(want[unit, 1])) and np.array_equal(prim >= 0, surf[:, 0] > 0)


def test_nee_table_matches_the_reference(golden_dir):
    g = np.load(os.path.join(golden_dir, "ref_nee.npz"))
    cols = g["cols"]
    got = _scene(golden_dir, "standin24_spheres").nee(g["in5"])
    bad = differing_rows(got[:, cols], g["out12"][:, cols])
    assert bad.size == 0, f"{bad.size} NEE rows differ from the reference (light index, point, pdf, light colour, next draw), first {bad[:8]}"


def _check_image(img_g, img_r, what):
    rr = rel_rms(img_g, img_r)
    same = (bits(img_g) == bits(img_r)).all(-1)
    print(f"{what}: relRMS {rr:.3e}, bit-identical pixels {same.mean():.6f}")
    assert np.isfinite(img_g).all()
    assert rr <= REL_RMS_TOL, f"{what}: relative RMS {rr:.3e} > {REL_RMS_TOL}"
    assert same.mean() >= 0.999, f"{what}: only {same.mean():.5f} of pixels bit-identical"


@pytest.mark.parametrize("tail", ["tail_in_wf_drain", "pipeline_to_the_end"])
@pytest.mark.parametrize("name", list(SCENES))
def test_image_matches_the_references(golden_dir, monkeypatch, name, tail):
    """64 x 64, 2 passes x 8 spp, the reference's MAX_BOUNCE 8: the frame its GetColor_iter gives.  For cornell and standin24 that is the
    `image` of oracle_<scene>.npz (test_live_paths_reproduce_the_committed_images), for the spheres scene the reference's own fixture.
    Both render tails (PTAMD_DRAIN is read when a scene is created) and both shading schedules."""
    if tail == "pipeline_to_the_end":
        monkeypatch.setenv("PTAMD_DRAIN", "0")
    else:
        monkeypatch.delenv("PTAMD_DRAIN", raising=False)
    file = "ref_image_standin24_spheres_b8.npz" if name == "standin24_spheres" else f"oracle_{name}.npz"
    g = np.load(os.path.join(golden_dir, file))
    assert int(g["max_bounce"]) == 8
    sc = _scene(golden_dir, name)
    cam = ptamd.make_camera(64, 64)
    prm = ptamd.default_params(passes=int(g["passes"]), spp_per_pass=int(g["spp"]), max_bounce=8)
    for rounds in (0, 1):
        sc.set_shade_rounds(rounds)
        _check_image(sc.render(cam, prm), g["image"], f"{name}, {tail}, shade rounds {rounds}")
