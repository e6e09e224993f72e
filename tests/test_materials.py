"""Materials and lights of an uploaded scene (pt_scene_update_materials, pt_scene_update_materials_host,
pt_scene_update_sphere_materials, pt_scene_nee_prune): the C-ABI surface, the argument checks and the numpy yardstick
(tests/materials_ref.py) on the CPU; on the GPU every array a render reads, the two kernel arguments and every kind of render
after an update, against a FRESH upload of the same triangles with the new materials — whose own parity with the oracle and the
reference the rest of the suite pins — and, for one scene, against the CPU oracle.

Comparison is by bits; there is no tolerance.  One thing is stated here once: two NaNs count as equal whatever their sign and
payload.  A zero-area triangle has a NaN normal (0 / 0), which the host writes as -NaN and the device as +NaN; scenes_util.
attribute_scene has two such triangles, set (b) makes lights of a seeded 30 % of all triangles, and a path that samples such a light
carries the NaN into its pixel in either scene.  tests/test_dynamic.py compares its arrays the same way."""
import ctypes as C
import os

import numpy as np
import pytest

import dynamic_ref as R
import materials_ref as M
import ptamd
from scenes_util import attribute_scene, scene_rays8
from scenes_util import test_spheres as make_test_spheres

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("pt_scene_update_materials", "pt_scene_update_materials_host", "pt_scene_update_sphere_materials", "pt_scene_nee_prune")
ARRAYS = ("nodes", "quad", "tri", "tripair", "leafbox", "surf", "lights", "spheres", "core")
CAMERAS = (((0.0, 20.0, 60.0), (0.0, 90.0, 0.0), 45.0), ((0.0, 20.0, 53.0), (0.0, 93.5, 0.0), 45.0))
FRAMES = ((64, 48), (100, 52))
PASSES, SPP = 3, 4
SEED = 20
SCENES = ("cornell", "standin16", "standin40", "attribute")


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def params(**kw):
    return ptamd.default_params(**{**dict(passes=PASSES, spp_per_pass=SPP), **kw})


_BUILT = {}


def _build(name):
    """(nodes, tris, spheres) of a test scene."""
    if name not in _BUILT:
        prims = {"cornell": lambda: ptamd.gen_scene(0), "standin16": lambda: ptamd.gen_scene(1, 16), "standin40": lambda: ptamd.gen_scene(1, 40),
                 "attribute": lambda: attribute_scene(7)[0]}[name]()
        nodes, tris, _ = ptamd.build_bvh(prims)
        _BUILT[name] = (nodes, tris, make_test_spheres())
    return _BUILT[name]


# ---------------------------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_exported_declared_and_bound():
    l = C.CDLL(ptamd.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "pt_api.h")).read()
    bound = {n for n, _, _ in ptamd.API}
    for name in NEW_SYMBOLS:
        assert hasattr(l, name), name
        assert f" {name}(" in hdr and name in bound, name
    for name in ("update_materials", "update_sphere_materials"):
        assert callable(getattr(ptamd.Scene, name))
    assert isinstance(ptamd.Scene.nee_prune, property)
    assert "Materials and lights of an uploaded scene" in hdr


def test_bad_arguments_are_rejected_before_any_device_call():
    """A fake scene and fake device addresses: never dereferenced, and no HIP call is made, when an argument is bad."""
    l = ptamd.lib()
    scene, d_mat = C.c_void_p(1 << 40), C.c_void_p((1 << 40) + (1 << 20))
    sph = make_test_spheres()
    buf = np.zeros(12, np.float32)
    cases = [
        ("update_materials: NULL scene", lambda: l.pt_scene_update_materials(None, d_mat, None)),
        ("update_materials: NULL d_mat12", lambda: l.pt_scene_update_materials(scene, None, None)),
        ("update_materials_host: NULL scene", lambda: l.pt_scene_update_materials_host(None, ptamd._ptr(buf))),
        ("update_materials_host: NULL h_mat12", lambda: l.pt_scene_update_materials_host(scene, None)),
        ("update_sphere_materials: NULL scene", lambda: l.pt_scene_update_sphere_materials(None, ptamd._ptr(sph), 3)),
        ("update_sphere_materials: NULL array", lambda: l.pt_scene_update_sphere_materials(scene, None, 3)),
    ]
    for what, call in cases:
        assert call() == -1, what
        assert "pt_scene_" + what.split(":")[0] + ":" in l.pt_last_error().decode(), (what, l.pt_last_error())
    assert l.pt_scene_nee_prune(None) == 0


class _FakeScene:
    n_tris, device, _h = 5, 0, C.c_void_p(1 << 40)


def test_wrapper_checks_shape_dtype_and_device_on_the_host():
    import torch
    fake = _FakeScene()
    up = ptamd.Scene.update_materials
    for mat in (np.zeros((4, 12), np.float32), np.zeros((5, 11), np.float32), np.zeros(60, np.float32)):
        with pytest.raises(ptamd.PtError):
            up(fake, mat)
    for mat in (torch.zeros((5, 12)), torch.zeros((5, 12), dtype=torch.float64), torch.zeros((4, 12)), torch.zeros((12, 5)).t(), [0.0] * 60):
        with pytest.raises(ptamd.PtError):      # a CPU tensor, a wrong dtype, a wrong size, not contiguous, not an array
            up(fake, mat)


def test_apply_materials_leaves_every_other_float_alone():
    _, tris, _ = _build("standin16")
    for name, mat in M.material_sets(tris, SEED):
        t2 = M.apply_materials(tris, mat)
        other = np.ones(tris.shape[1], bool)
        for o in M.T_MATS:
            other[o:o + 12] = False
            assert np.array_equal(bits(t2[:, o:o + 12]), bits(mat)), name
        assert other.sum() == 88 - 36 and np.array_equal(bits(t2[:, other]), bits(tris[:, other])), name
    assert np.array_equal(bits(M.apply_materials(tris, M.set_e(tris))), bits(tris))      # the stock scenes: one material per triangle


@pytest.mark.parametrize("kind,lat_lon,want", [(0, 187, 2), (1, 16, 2), (2, 16, 2)])
def test_light_rule_on_the_stock_scenes(kind, lat_lon, want):
    """The float32 rule gives the lights the float64 reading of the same test (dynamic_ref.emissive) gives: the stock emittances are
    far from the threshold.  Their number is what pt_scene_create reports for these scenes (the GPU tests compare it as well)."""
    _, tris, _ = ptamd.build_bvh(ptamd.gen_scene(kind, lat_lon))
    got = M.lights_of(tris)
    assert np.array_equal(got, R.emissive(tris)) and int(got.sum()) == want
    assert np.array_equal(M.is_light(M.materials(tris)), got)
    assert M.light_records(tris).shape == (want, 16)
    assert M.emittance_ok(M.materials(tris), make_test_spheres())


def test_material_sets_are_what_the_tests_need():
    f = np.float32
    probe = np.zeros((6, 12), f)
    probe[:, 0] = (1.1e-4, 0.9e-4, np.nan, np.inf, -1.0, 2e8)
    assert M.is_light(probe).tolist() == [True, False, False, True, True, True]
    assert [M.emittance_ok(probe[i:i + 1]) for i in range(6)] == [True, True, False, False, False, False]
    for name in SCENES:
        _, tris, _ = _build(name)
        n = len(tris)
        sets = dict(M.material_sets(tris, SEED))
        counts = {k: int(M.is_light(v).sum()) for k, v in sets.items()}
        assert counts["c"] == 1 and M.is_light(sets["c"])[-1] and counts["d"] == 0, name
        assert counts["a"] == counts["e"] == int(M.is_light(M.materials(tris)).sum()), name
        lit = M.is_light(sets["b"])
        assert 0.2 * n < counts["b"] < 0.5 * n + 9 and all(lit[i] for i in M.FORCED + (n - 1,) if i < n), name
        a, b = M.straddle_pair(tris, SEED)
        assert lit[a] and not lit[b] and sets["b"][a, 0] == f(1.1e-4) and sets["b"][b, 0] == f(0.9e-4), name
        # no emittance is closer than 10 % to the threshold
        ln = np.sqrt((np.concatenate(list(sets.values()))[:, 0:3].astype(np.float64) ** 2).sum(1))
        assert not ((ln > 0.9001e-4) & (ln < 1.0999e-4)).any(), name
    assert len(_build("standin40")[1]) == 3132 and len(_build("standin16")[1]) == 492 and len(_build("cornell")[1]) == 12


# ---------------------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def _gpu():
    import torch
    import oracle_lib as O
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    O.set_libm(1)            # the pinned contract: correctly rounded float transcendentals
    yield


def _same(g, w):
    g, w = np.ascontiguousarray(g), np.ascontiguousarray(w)
    if g.shape != w.shape:
        return np.zeros(1, bool)
    if w.dtype == np.float32:
        return (g.view(np.uint32) == w.view(np.uint32)) | (np.isnan(g) & np.isnan(w))
    return g == w


def _assert_same(got, want, what):
    same = _same(got, want)
    assert same.all(), (what, np.asarray(got).shape, np.asarray(want).shape, np.argwhere(~same)[:5].tolist())


def _state(sc):
    st = {a: sc.dbg_array(a) for a in ARRAYS}
    st["num_lights"], st["nee_prune"] = np.int64(sc.num_lights), np.int64(sc.nee_prune)
    return st


def _assert_state(got, want, what, names=ARRAYS):
    assert int(got["num_lights"]) == int(want["num_lights"]), (what, "num_lights", got["num_lights"], want["num_lights"])
    assert int(got["nee_prune"]) == int(want["nee_prune"]), (what, "nee_prune", got["nee_prune"], want["nee_prune"])
    for a in names:
        assert got[a].shape == want[a].shape, (what, a, got[a].shape, want[a].shape)
        _assert_same(got[a], want[a], (what, a))


def _fresh(name, mat, spheres=None):
    nodes, tris, sph = _build(name)
    tris2 = R.restate_tris(M.apply_materials(tris, mat), R.positions(tris))      # normal and area restated from the current positions
    return ptamd.Scene(nodes, tris2, sph if spheres is None else spheres), tris2


@pytest.mark.gpu
@pytest.mark.parametrize("name", SCENES)
def test_arrays_after_each_set_are_the_fresh_scenes(_gpu, name):
    """Sets (a) .. (e) in that order on ONE scene, through the device entry point and, on a second scene, through the host one: after
    each, all nine arrays with their sizes, the light count and the pruning flag are those of a fresh upload, and the two scenes hold
    the same bytes.  After (e) the scene is the scene never updated — except that in scenes_util.attribute_scene one light has an
    emissive SECOND vertex only: an update gives a triangle ONE material, its mat0, so that triangle is no light afterwards, and the
    `lights` array is the uploaded one without its record."""
    import torch
    nodes, tris, sph = _build(name)
    dev_sc, host_sc = ptamd.Scene(nodes, tris, sph), ptamd.Scene(nodes, tris, sph)
    never = _state(ptamd.Scene(nodes, tris, sph))
    assert int(never["num_lights"]) == int(M.lights_of(tris).sum()) and never["lights"].size == 16 * never["num_lights"]
    counts = []
    for label, mat in M.material_sets(tris, SEED):
        dev_sc.update_materials(torch.from_numpy(mat).cuda())
        host_sc.update_materials(mat)
        fresh, tris2 = _fresh(name, mat)
        got, want = _state(dev_sc), _state(fresh)
        _assert_state(got, want, f"{name} ({label}) against a fresh upload")
        _assert_state(_state(host_sc), got, f"{name} ({label}) host against device entry point")
        # ... and the yardstick itself: the light records and the material floats from numpy
        _assert_same(got["lights"].reshape(-1, 16), M.light_records(tris2), f"{name} ({label}) light records from numpy")
        _assert_same(got["surf"].reshape(-1, 48)[:, 36:48], mat, f"{name} ({label}) surface floats 36..47")
        assert int(got["nee_prune"]) == 1 and int(got["num_lights"]) == int(M.is_light(mat).sum())
        counts.append(int(got["num_lights"]))
    assert counts[2] == 1 and counts[3] == 0 and counts[1] > 0.2 * len(tris) and counts[4] == counts[0]
    final = _state(dev_sc)
    if name == "attribute":
        second_vertex_only = M.lights_of(tris) & ~M.is_light(M.materials(tris))
        assert second_vertex_only.sum() == 1 and counts[4] == int(never["num_lights"]) - 1
        keep = ~second_vertex_only[M.lights_of(tris)]
        _assert_same(final["lights"].reshape(-1, 16), never["lights"].reshape(-1, 16)[keep], "attribute (e): the lights that have an emissive mat0")
        for a in ARRAYS:
            if a != "lights":
                _assert_same(final[a], never[a], ("attribute (e) against the scene never updated", a))
    else:
        _assert_state(final, never, f"{name} (e) against the scene never updated")


def _every_render(sc, name):
    """Every kind of render and query of one scene, as a dict of arrays."""
    out = {}
    rays = scene_rays8(3000, np.random.RandomState(11))
    for W, H in FRAMES:
        cam, prm = ptamd.make_camera(W, H), params()
        for mode in (1, 0):
            sc.set_mode(mode)
            out[f"render {W}x{H} mode {mode}"] = sc.render(cam, prm)
        sc.set_mode(1)
        cams = [ptamd.make_camera(W, H, pos=p, rot_deg=r, fovy_deg=f) for p, r, f in CAMERAS]
        out[f"views {W}x{H}"] = sc.render_views(cams, prm)
        out[f"window {W}x{H}"] = sc.render_window(cam, prm, (5, 3, 37, 29))
        cr, seeds, stride = ptamd.camera_rays(cam, 0)
        out[f"render_rays {W}x{H}"] = sc.render_rays(cr, params(passes=1), seeds, stride)
        aov, prim = sc.aov(cam, prm)
        out[f"aov {W}x{H}"], out[f"aov prim {W}x{H}"] = aov, prim
    t, prim, surf = sc.trace_rays(rays, surface=True)
    out["trace t"], out["trace prim"], out["trace surface"] = t, prim, surf
    hit = prim >= 0
    pts = surf[hit][:1500, 5:8]
    seeds = np.random.RandomState(12).randint(0, 2**32, (pts.shape[0], 2), dtype=np.uint64).astype(np.uint32)
    out["nee in"] = np.concatenate([pts, seeds.view(np.float32)], 1)
    out["nee"] = sc.nee(out["nee in"])
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("label", ["a", "b"])
@pytest.mark.parametrize("name", SCENES)
def test_every_entry_point_after_an_update_is_the_fresh_scenes(_gpu, name, label):
    nodes, tris, sph = _build(name)
    mat = dict(M.material_sets(tris, SEED))[label]
    sc = ptamd.Scene(nodes, tris, sph)
    before = sc.render(ptamd.make_camera(*FRAMES[0]), params())
    sc.update_materials(mat)
    fresh, tris2 = _fresh(name, mat)
    got, want = _every_render(sc, name), _every_render(fresh, name)
    assert got.keys() == want.keys()
    for k in want:
        _assert_same(got[k], want[k], f"{name} ({label}) {k}")
    assert (got["trace prim"] >= 0).mean() > 0.7
    assert not _same(got[f"render {FRAMES[0][0]}x{FRAMES[0][1]} mode 1"], before).all()      # the new materials are visible
    if name == "standin16" and label == "b":
        # ... and the CPU oracle on tris'
        import oracle_lib as O
        so = O.Scene(nodes.tobytes(), tris2, sph)
        for W, H in FRAMES:
            ref, _ = so.render(O.make_camera(W, H), O.make_params(W, H, PASSES, SPP), 16)
            assert np.isfinite(ref).all()
            for mode in (1, 0):
                _assert_same(got[f"render {W}x{H} mode {mode}"], ref, f"{W}x{H} mode {mode} against the oracle")
        ref_nee = so.nee(got["nee in"])
        assert (ref_nee[:, 8:11].sum(1) > 0).sum() > 100
        _assert_same(got["nee"], ref_nee, "nee against the oracle")


@pytest.mark.gpu
@pytest.mark.parametrize("order", ["move, then materials", "materials, then move"])
def test_order_with_the_vertex_update(_gpu, order):
    """A material update after a vertex update makes its light records from the MOVED positions (the scene's position mirror, which
    every vertex update refreshes), and a vertex update after a material update moves the NEW lights.  Without the mirror's refresh
    in dyn_surf the first order fails: the mirror then still holds the uploaded positions, and set (b) makes lights of about 140
    triangles of the mesh, every one of which the move displaces."""
    import torch
    name = "standin16"
    nodes, tris, sph = _build(name)
    mat = M.set_b(tris, SEED)
    pos = torch.from_numpy(R.positions(tris)).cuda()
    moved = R.move_rigid_wobble(pos, torch.from_numpy(R.mesh_mask(tris)).cuda(), torch).reshape(-1, 9).contiguous()
    assert (M.is_light(mat) & R.mesh_mask(tris)).sum() > 100
    sc = ptamd.Scene(nodes, tris, sph)
    if order.startswith("move"):
        sc.update_vertices(moved)
        sc.update_materials(mat)
    else:
        sc.update_materials(mat)
        sc.update_vertices(moved)
    tris2 = R.restate_tris(M.apply_materials(tris, mat), moved.cpu().numpy())
    fresh = ptamd.Scene(R.refit_nodes(nodes, tris2), tris2, sph)
    # a fresh upload builds its own traversal tree over the moved triangles: the arrays that do not depend on it
    _assert_state(_state(sc), _state(fresh), order, ("surf", "lights", "leafbox", "spheres"))
    _assert_same(sc.dbg_array("lights").reshape(-1, 16), M.light_records(tris2), order + ": light records from numpy")
    cam, prm = ptamd.make_camera(*FRAMES[1]), params()
    _assert_same(sc.render(cam, prm), fresh.render(cam, prm), order + ": render")
    unmoved, _ = _fresh(name, mat)
    assert not _same(sc.dbg_array("lights"), unmoved.dbg_array("lights")).all()


@pytest.mark.gpu
def test_a_scene_without_a_light(_gpu):
    name = "standin16"
    nodes, tris, sph = _build(name)
    sc = ptamd.Scene(nodes, tris, sph)
    cam, prm = ptamd.make_camera(*FRAMES[0]), params()
    first = sc.render(cam, prm)
    rays = scene_rays8(2000, np.random.RandomState(3))
    sc.update_materials(M.set_d(tris))
    assert sc.num_lights == 0 and sc.dbg_array("lights").size == 0
    with pytest.raises(ptamd.PtError, match=r"\(-2\)"):
        sc.render(cam, prm)
    with pytest.raises(ptamd.PtError, match=r"\(-2\)"):
        sc.nee(np.zeros((4, 5), np.float32))
    fresh, _ = _fresh(name, M.set_d(tris))
    assert fresh.num_lights == 0
    with pytest.raises(ptamd.PtError, match=r"\(-2\)"):
        fresh.render(cam, prm)
    for g, w, what in zip(sc.trace_rays(rays, surface=True), fresh.trace_rays(rays, surface=True), ("t", "prim", "surface")):
        _assert_same(g, w, "trace_rays without a light: " + what)
    for g, w, what in zip(sc.aov(cam, prm), fresh.aov(cam, prm), ("aov", "prim")):
        _assert_same(g, w, "aov without a light: " + what)
    sc.update_materials(M.set_e(tris))
    assert sc.num_lights == 2
    _assert_same(sc.render(cam, prm), first, "render after the lights came back")


@pytest.mark.gpu
def test_pruning_flag_follows_the_emittances(_gpu):
    name = "standin16"
    nodes, tris, sph = _build(name)
    sc = ptamd.Scene(nodes, tris, sph)
    assert sc.nee_prune == 1
    base = M.materials(tris)
    for bad in (np.inf, np.nan, -1.0, 2e8):
        mat = base.copy()
        mat[200, 1] = bad
        assert not M.emittance_ok(mat, sph)
        sc.update_materials(mat)
        fresh, _ = _fresh(name, mat)
        assert sc.nee_prune == 0 and fresh.nee_prune == 0, bad
        _assert_state(_state(sc), _state(fresh), f"emittance {bad}")
        sc.update_materials(base)
        assert sc.nee_prune == 1, bad
    # the same through the spheres
    for bad in (np.inf, np.nan, -1.0, 2e8):
        s2 = sph.copy()
        s2[1, 5] = bad
        sc.update_sphere_materials(s2)
        fresh = ptamd.Scene(nodes, tris, s2)
        assert sc.nee_prune == 0 and fresh.nee_prune == 0, bad
        _assert_same(sc.dbg_array("spheres"), fresh.dbg_array("spheres"), f"sphere emittance {bad}")
        sc.update_sphere_materials(sph)
        assert sc.nee_prune == 1, bad
    # a bad triangle keeps the flag down whatever the spheres are, and the other way round
    mat = base.copy()
    mat[7, 0] = 2e8
    sc.update_materials(mat)
    sc.update_sphere_materials(sph)
    assert sc.nee_prune == 0
    s2 = sph.copy()
    s2[0, 4] = -1.0
    sc.update_sphere_materials(s2)
    sc.update_materials(base)
    assert sc.nee_prune == 0
    sc.update_sphere_materials(sph)
    assert sc.nee_prune == 1
    # a new sphere material: rendered as a fresh upload renders it; update_spheres then compares against the NEW materials
    new = sph.copy()
    new[:, 0:3] += np.float32([[-3, 2, 4], [2, 3, -1], [4, -6, 5]])
    new[2, 7:10] = (0.9, 0.3, 0.2)      # albedo
    new[0, 4:7] = (3.0, 2.0, 1.0)       # an emissive sphere
    new[1, 13] = 1.0                    # opacity
    sc.update_sphere_materials(new)
    fresh = ptamd.Scene(nodes, tris, new)
    _assert_state(_state(sc), _state(fresh), "new sphere materials")
    cam, prm = ptamd.make_camera(*FRAMES[0]), params()
    _assert_same(sc.render(cam, prm), fresh.render(cam, prm), "render with new sphere materials")
    assert not _same(sc.render(cam, prm), ptamd.Scene(nodes, tris, sph).render(cam, prm)).all()
    again = new.copy()
    again[:, 0:3] += 1.0
    sc.update_spheres(again)
    _assert_same(sc.dbg_array("spheres"), again.ravel(), "update_spheres with the new materials")
    old = sph.copy()
    with pytest.raises(ptamd.PtError, match="material"):
        sc.update_spheres(old)
    with pytest.raises(ptamd.PtError):
        sc.update_sphere_materials(new[:2])
    with pytest.raises(ptamd.PtError):
        ptamd.Scene(nodes, tris).update_sphere_materials(new)      # a scene without spheres
    _assert_same(sc.dbg_array("spheres"), again.ravel(), "rejected calls change nothing")


@pytest.mark.gpu
def test_device_bytes_follow_the_lights(_gpu):
    name = "standin40"
    nodes, tris, sph = _build(name)
    sets = dict(M.material_sets(tris, SEED))
    a, b = ptamd.Scene(nodes, tris, sph), ptamd.Scene(nodes, tris, sph)
    bytes0 = a.device_bytes
    seen = []
    for label in ("a", "a", "b", "b", "c", "d", "b", "e"):
        for sc in (a, b):
            sc.update_materials(sets[label])
        assert a.device_bytes == b.device_bytes, label
        seen.append(a.device_bytes)
    n_b = int(M.is_light(sets["b"]).sum())
    assert seen[0] > bytes0                      # the first update of either kind: the maps of the build and the positions
    assert seen[1] == seen[0]                    # the same set again
    assert seen[2] >= seen[1] + (n_b - 2) * 68   # the count grew: 64 bytes of record and 4 of map per light
    assert seen[3:] == [seen[2]] * 5             # nothing shrinks, and no more lights than before allocates nothing
    # a vertex update afterwards finds everything it needs
    a.update_vertices(R.positions(tris).reshape(-1, 9))
    assert a.device_bytes == seen[-1]
    assert a.dbg_array("lights").size == 16 * a.num_lights == 16 * 2


@pytest.mark.gpu
def test_tensor_filled_on_a_side_stream(_gpu):
    """The update is enqueued on a non-default stream behind the kernel that fills its input there, with no synchronisation between."""
    import torch
    name = "standin40"
    nodes, tris, sph = _build(name)
    mat = M.set_b(tris, SEED)
    dev = torch.device("cuda:0")
    src = torch.from_numpy(mat).to(dev)
    torch.cuda.synchronize()
    sc = ptamd.Scene(nodes, tris, sph)
    st = torch.cuda.Stream(dev)
    with torch.cuda.stream(st):
        t = torch.zeros((len(tris), 12), dtype=torch.float32, device=dev)
        t.add_(src)
        sc.update_materials(t, stream_ptr=st.cuda_stream)
    st.synchronize()
    ref = ptamd.Scene(nodes, tris, sph)
    ref.update_materials(mat)
    _assert_state(_state(sc), _state(ref), "tensor on a side stream against the numpy path")
    cam, prm = ptamd.make_camera(*FRAMES[0]), params()
    _assert_same(sc.render(cam, prm), ref.render(cam, prm), "render")
